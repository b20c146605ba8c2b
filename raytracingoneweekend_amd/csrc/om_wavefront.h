// om_wavefront.h — host interface of the two render pipelines: the wavefront and the
// megakernel (§5.1), and of the ray queries.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/ottomarcher.h"
#include "om_layout.h"

namespace omw {

// One batch's device work buffers: ping-pong path queues, result slots, per-bounce counts.
struct QueueSet {
    float4* q[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};  // ping-pong queues: o|depthf, d|first_id, cur|seg
    uint4* qr[2] = {nullptr, nullptr};   // rng lo, rng hi, path slot, pad
    float4* res = nullptr;       // colour.xyz, depth
    uint32_t* res_id = nullptr;  // obj id (0xFFFFFFFF = no sample)
    uint32_t* counts = nullptr;  // per bounce, per queue segment: live rays
    float2* hit = nullptr;       // split march pipeline: (closest, winner) per queue slot
    void release();
};

// Device work buffers of one context; grown on demand, never shrunk.  kMaxSets queue sets
// let that many batches be in flight at once (overlapped schedule): batch
// i uses set i % S on stream i % S (stream 0 = the caller's stream, the others `side`).
constexpr int kMaxSets = 4;
struct Buffers {
    uint64_t cap = 0;            // paths per batch (per set)
    uint32_t counts_n = 0;       // count words per set
    int nsets = 0;               // sets allocated at `cap`
    QueueSet set[kMaxSets];
    uint32_t* n0 = nullptr;      // fixed spp: per listed pixel, the call-start Stats.n (Gen::n0); adaptive: live lists + plans
    uint64_t n0_cap = 0;
    hipStream_t side[kMaxSets] = {};  // streams 1.. of the overlapped schedule
    std::vector<hipEvent_t> ev;  // cross-stream ordering events (timing disabled)
    void release();
};

// Optional device timing (om_set_timing): HIP event pairs on the launch stream.  Mode 1
// brackets every launch (tagged with its OM_KT_* class) and the call; mode 2 brackets only
// the call (OM_KT_BOUNCE_SPAN, with its bounce-family launch count): two events per call.
struct Timer {
    int mode = 0;
    std::vector<hipEvent_t> ev;   // pool, pairs (2i, 2i+1)
    std::vector<int> cls;         // class of pair i since the last read (-1: open)
    std::vector<uint32_t> nl;     // launches inside pair i
    bool on() const { return mode != 0; }
    // Opens pair i (recorded on `st`) and returns i; pairs may nest (a call around its launches).
    int begin(hipStream_t st) {
        if (!on()) return -1;
        const size_t i = cls.size();
        while (ev.size() < 2 * i + 2) {
            hipEvent_t e = nullptr;
            if (hipEventCreate(&e) != hipSuccess) { mode = 0; return -1; }
            ev.push_back(e);
        }
        (void)hipEventRecord(ev[2 * i], st);
        cls.push_back(-1);
        nl.push_back(0);
        return (int)i;
    }
    void end(int i, int c, hipStream_t st, uint32_t launches = 1) {
        if (!on() || i < 0) return;
        (void)hipEventRecord(ev[2 * i + 1], st);
        cls[i] = c;
        nl[i] = launches;
    }
    void clear() { cls.clear(); nl.clear(); }
    void release() { for (auto e : ev) (void)hipEventDestroy(e); ev.clear(); clear(); }
};

struct Launch {
    OmSceneDev S;
    OmCamDev C;
    OmParamsDev P;
    const float2* jitter;
    om_pixel_stats* stats;
    const uint32_t* pixels;      // device list of row-major pixel indices (tile order); megakernel: null = the full frame
    uint32_t n_pixels;
    bool stats_by_pixel;         // stats[pixel] (full frame) instead of stats[k]
    unsigned long long* counters;
    bool count;
    int trace_mode;              // the ctx's kernel choice as a TR_* value (om_layout.h), before the world decides
    uint32_t tail_bounce;        // first bounce run by the persistent tail kernel (0 = default)
    uint32_t streams;            // batches in flight (queue sets, streams), 1 = serial, <= kMaxSets
    uint32_t ad_batches;         // adaptive calls: batches per stream per call (0 = OM_WF_ADAPTIVE_BATCHES)
    uint32_t ad_paths_log2;      // adaptive calls: log2 of the target paths per batch (0 = OM_WF_ADAPTIVE_PATHS_LOG2)
    Timer* timer;                // per-launch event timing (may be off)
    const uint32_t* tile_off;    // primary-ray candidate lists per 8x8 tile (null = traverse the BVH)
    const uint16_t* tile_idx;
    const float* tile_tnear;     // per leaf record: lower bound of a primary ray's t to its box (lists sorted by it)
    unsigned long long* progress_host;   // om_progress word (pinned host) or null; device side counters[OMC_PROGRESS]
};

// Renders P.sample_count samples of every listed pixel; returns 0 or a HIP error text.
hipError_t render(Buffers& B, const Launch& L, hipStream_t stream, std::string& err);
// The same as one render_kernel launch (om_megakernel.hip); of L it reads neither the wavefront's
// schedule knobs nor the tile lists.
hipError_t render_megakernel(const Launch& L, hipStream_t stream, std::string& err);

// f(std::bool_constant<b[0]>{}, std::bool_constant<b[1]>{}, ...): runtime flags as template arguments.
// f is instantiated for every combination; it leaves out the ones never launched with if constexpr.
template <size_t N, class F, class... C>
void with_flags(const bool (&b)[N], F&& f, C... c) {
    if constexpr (sizeof...(C) == N) f(c...);
    else if (b[sizeof...(C)]) with_flags(b, f, c..., std::true_type{});
    else with_flags(b, f, c..., std::false_type{});
}

// One radiance query (om_ray_color*_device): ray_color of n caller-given rays through
// the wavefront's queues, tails and schedule knobs.
struct PathQuery {
    OmSceneDev S;
    OmParamsDev P;               // tmin, tmax, march_steps, max_depth, skey; the rest 0
    const om_ray* rays;          // device, n records
    const uint64_t* rng;         // device, n PathRng states; null: (skey, stream_base + i, sample)
    uint32_t n;
    uint32_t stream_base, sample;
    om_radiance* out;            // device, n records
    unsigned long long* counters;
    bool count;
    int trace_mode;              // as Launch::trace_mode
    uint32_t tail_bounce;        // as Launch::tail_bounce
    uint32_t paths_log2;         // log2 of the paths per batch (0 = 2^25, the renderer's)
    Timer* timer;
};
// Queues the batches of Q on `stream`, through queue set 0 of B.
hipError_t ray_color(Buffers& B, const PathQuery& Q, hipStream_t stream, std::string& err);

// One frame call from caller-given rays (om_render_rays*_device): P.sample_count samples
// of the listed pixels, ray_color of rays[s * n_pixels + k] added to stats[pixel of k] in sample order.
struct FrameRays {
    OmSceneDev S;
    OmParamsDev P;               // as a render's; the camera-only fields (wf_m1, hf_m1, tiles_x) unused
    const om_ray* rays;          // device, sample_count * n_pixels records, sample-major
    const uint64_t* rng;         // device, the same layout; null: (skey, pixel, Stats.n at the sample)
    const uint32_t* pixels;      // device, n_pixels row-major pixel indices; null: the whole frame in order
    uint32_t n_pixels;
    om_pixel_stats* stats;       // device, the frame, by pixel
    unsigned long long* counters;
    bool count;
    int trace_mode;              // as Launch::trace_mode
    uint32_t tail_bounce;        // as Launch::tail_bounce
    uint32_t paths_log2;         // as PathQuery::paths_log2
    Timer* timer;
    unsigned long long* progress_host;   // as Launch::progress_host
};
// Queues the batches of Q on `stream`, through queue set 0 of B.
hipError_t render_rays(Buffers& B, const FrameRays& Q, hipStream_t stream, std::string& err);

// One batch of ray queries: closest-hit (om_hit_rays*_device) when `occluded` is
// null, any-hit (om_occluded_rays_device, §5.16) otherwise.
struct Query {
    OmSceneDev S;
    float tmin, tmax;
    uint32_t march_steps;
    const om_ray* rays;          // device, n records
    const om_ray_window* windows = nullptr;   // device, n records; null: [tmin, tmax] for every ray
    om_hit* hits = nullptr;      // device, n records (closest-hit)
    uint8_t* occluded = nullptr; // device, n bytes (any-hit)
    uint32_t n;
    unsigned long long* counters;
    bool count;
    int trace_mode;              // as Launch::trace_mode
};
// Traces Q.n rays in one persistent launch on `stream` (at most query_max_grid() workgroups).
hipError_t query(const Query& Q, hipStream_t stream);
uint32_t query_max_grid();       // on the current device
// What renders and queries with this trace_mode run on scene S (om_get_tree_info): the BVH2 regime
// as an OM_TREE_* value (OM_TREE_NONE: a variant that walks no BVH2) and the dynamic LDS bytes a
// workgroup requests for it.
void tree_regime(int trace_mode, const OmSceneDev& S, int32_t* regime, uint32_t* lds_bytes);

}  // namespace omw
