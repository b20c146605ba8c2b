// om_wavefront.hip — wavefront path tracer: the bounce recursion of
// ray_color (render_thread.rs:128-143) flattened into per-bounce launches over SoA
// path queues in HBM:
//
//   bounce 0    one lane per (sample, pixel): camera ray (render_thread.rs:183-192),
//               closest hit (hits.rs:270-365), HitRecord + Material::scatter / sky
//               (render_thread.rs:105-126); survivors are compacted into queue 1,
//               finished paths write (colour, depth, id) to their result slot
//   bounce b    the same from queue b: trace + shade + compaction in ONE kernel (the
//               path state is read once and written once per bounce; no hit buffer)
//   tail        from bounce T on the queues hold few paths: one resident launch runs every
//               remaining path to completion, the paths dealt in 64-path units evenly over
//               the chip's workgroups and wave slots (no ~40 near-empty launch pairs)
//   accumulate  one lane per pixel: Stats::add over the batch's samples IN SAMPLE
//               ORDER (render_thread.rs:23-39): bit-identical to the sequential
//               reference and to the megakernel.
//
// Queues are SEGMENTED: workgroup s owns segment s of every queue and compacts its
// survivors into segment s of the next queue with a ballot + LDS scan — no global
// atomics (one contended queue counter capped the first version at ~88 wave-appends
// per microsecond, MI355X_MICROARCH.md row 'dequeue').  Paths are sample-major
// (slot = s_local * n_pixels + k over a tile-ordered pixel list), so a wave holds 64
// neighbouring pixels of one sample: coherent rays.
#include "om_wavefront.h"

#include <algorithm>
#include <type_traits>

#include "om_device.h"
#include "om_trace.h"
#include "om_tuning.h"
#include "om_deal.h"

using namespace omd;

namespace omw {

void QueueSet::release() {
    for (int a = 0; a < 2; ++a) {
        for (int b = 0; b < 3; ++b) { if (q[a][b]) (void)hipFree(q[a][b]); q[a][b] = nullptr; }
        if (qr[a]) (void)hipFree(qr[a]); qr[a] = nullptr;
    }
    if (res) (void)hipFree(res);
    if (res_id) (void)hipFree(res_id);
    if (counts) (void)hipFree(counts);
    if (hit) (void)hipFree(hit);
    res = nullptr; res_id = nullptr; counts = nullptr; hit = nullptr;
}

void Buffers::release() {
    for (auto& s : set) s.release();
    if (n0) (void)hipFree(n0);
    n0 = nullptr; n0_cap = 0;
    for (auto& st : side) { if (st) (void)hipStreamDestroy(st); st = nullptr; }

    for (auto e : ev) (void)hipEventDestroy(e);
    ev.clear();
    cap = 0; counts_n = 0; nsets = 0;
}

namespace {

constexpr uint32_t kNoSample = 0xFFFFFFFFu;
#define OM_WAVES_ATTR __attribute__((amdgpu_waves_per_eu(OM_WF_WAVES, OM_WF_WAVES)))   // occupancy request (waves per SIMD)
constexpr int kBlk = OM_WF_BLOCK;                                 // workgroup = one queue segment
constexpr int kStackDepth = (int)kB2Stack;                        // BVH2 per-lane LDS stack bound (entries)
// f32 BVH2 nodes staged in LDS sit OM_B2_NODE_STRIDE bytes apart (om_tuning.h)
constexpr uint32_t kB2Stride = OM_B2_NODE_STRIDE;
static_assert(kB2Stride % 16u == 0u && kB2Stride >= sizeof(OmBvh2Node), "16-B aligned node slots");
// stage_scene turns a child index into a slot offset in 16-B units (index * kB2Stride / 16): for
// every tree the budget admits, the scaled code must still read as a node, not as a leaf
static_assert(kB2LdsBudget / sizeof(OmBvh2Node) * (kB2Stride / 16u) < OM_LEAF, "scaled BVH2 child codes stay below OM_LEAF");
// the staged node: the ray-ordered copy (om_b2_planes.h, OM_B2_PLANES) or the node as it is in memory
// (a slot below 80 B, tools/ablate.sh p64, has no room for it and stages the plain node)
constexpr bool kB2Planes = OM_B2_PLANES != 0 && kB2Stride >= sizeof(OmBvh2NodeS);
using B2Staged = std::conditional<kB2Planes, OmBvh2NodeS, OmBvh2Node>::type;
static_assert(kB2Stride >= sizeof(B2Staged), "the staged node fits its slot");
// Variant flag of this file, above TR_BARY and dropped by tr_base like it: the kernel stages and
// reads the plain node even with OM_B2_PLANES.  The first launch (k_bounce<FIRST>) sets it: the
// three per-ray plane addresses of the ordered read are live over its traversals beside the
// camera state and cost it 12 B of scratch per lane, for a gain of 1 % of that launch; with the
// flag its code is the code it had (64 VGPRs, no scratch).
constexpr int TR_PLAIN_NODES = 32;
static_assert(TR_PLAIN_NODES > TR_BARY && (TR_PLAIN_NODES & (TR_BARY | (TR_BARY - 1))) == 0, "a flag of its own");
constexpr bool b2_ordered(int trf) { return kB2Planes && (trf & TR_PLAIN_NODES) == 0; }
// LDS bytes of the lane stack: S.b2_stack entries per lane (the tree's internal depth, 9 for
// S-traced: 9 KiB per 512-lane workgroup instead of 24 KiB at the 24-entry bound).
template <int TR>
__host__ __device__ inline uint32_t stack_bytes(const OmSceneDev& S) {
    if (tr_base(TR) == TR_BVH2_WIDE) return kBlk * S.b2w_stack * 4u;          // u32 entries
    return kBlk * ((tr_base(TR) == TR_BVH4_LDS || tr_base(TR) == TR_BVH4_GLOBAL) ? S.b4_stack : S.b2_stack) * 2u;
}
// LDS bytes of a BVH2 staged whole (TR_BVH2_LDS): padded nodes + leaf table
__host__ __device__ inline uint32_t b2_stage_bytes(const OmSceneDev& S) {
    return (S.n_b2nodes * kB2Stride + S.n_b2leaves * 4u + 15u) & ~15u;
}
constexpr uint32_t kTailSpb = OM_WF_TAIL_SPB;                     // marched tail: queue segments per workgroup
constexpr uint32_t kTailWgsPerCu = OM_WF_TAIL_WGS_PER_CU;         // traced tail: resident workgroups per CU
constexpr uint32_t kWaves = kBlk / 64;                            // waves of a workgroup
static_assert(kBlk % 64 == 0 && kTailWgsPerCu >= 1u, "whole waves; a tail grid");
// traced worlds: the launch of bounce 0 runs bounce 1 as well (om_tuning.h, k_bounce's FUSE); the
// first queue it writes is then bounce 2's
constexpr bool kFuseB1 = OM_WF_FUSE_B1 != 0;
// Per-bounce launches (bounce 0's included) before the tail kernel takes over: without the fused
// launch also the first bounce of the tail, with it one bounce later (tail_first), so that the
// launch counts per batch are the same either way.  On the balanced tail an earlier start measures faster
// (C1, 1 workgroup per CU: T = 8 / 10 / 12 / 16 -> 7307 / 7297 / 7281 / 7227 Msamples/s, means of
// three runs, parent 7125); the threshold stays where tests/test_gpu_production_shapes.py pins the
// launch counts of the bench's shapes
constexpr uint32_t kTailDefault = 16;
// marched worlds: bounce 0 as k_march + k_bounce<HIT>, every later segment in the lane-refilling
// tail (om_tuning.h)
constexpr uint32_t kTailMarched = OM_WF_TAIL_MARCHED;
// BVH2s read through L2 (S-10k): 10 (C3, r03_v24/v25: T = 6 / 8 / 10 / 12 / 16 / 20 -> 3318 / 3523 /
// 3553 / 3517 / 3416 / 3351 Msamples/s, means of two to four runs; on the balanced tail T = 6 / 8 /
// 10 / 12 -> 4608 / 4615 / 4556 / 4482, parent 4330: pinned like kTailDefault)
constexpr uint32_t kTailL2 = 10;
// batches above 2^25 paths (C4's 4K frame: 16 spp = 133M paths) keep more paths per late bounce,
// so the per-bounce launches stay efficient longer: 24 (C4, r03_v26: T = 12 / 16 / 20 / 24 ->
// 6956 / 7240 / 7304 / 7374 Msamples/s, means of two runs; on the balanced tail 7692 / 7698 / 7691 /
// 7668, parent 7564: flat)
constexpr uint32_t kTailBigBatch = 24;
__host__ __device__ inline uint32_t hyb_nodes(const OmSceneDev& S) {
    constexpr uint32_t kCap = OM_WF_HYB_BYTES / (uint32_t)sizeof(OmBvh2NodeH);
    return S.b2_lds_bytes ? 0u : (S.n_b2nodes < kCap ? S.n_b2nodes : kCap);
}
// the wide BVH2's nodes: behind the n_b2nodes half nodes of b2h's buffer (om_layout.h, om_upload_world)
static_assert(sizeof(OmBvh2NodeW) == sizeof(OmBvh2NodeH), "wide and half nodes share a buffer");
__host__ __device__ inline const OmBvh2NodeW* wide_nodes(const OmSceneDev& S) { return (const OmBvh2NodeW*)(S.b2h + S.n_b2nodes); }
// the wide BVH2's breadth-first prefix in LDS (om_tuning.h OM_WF_HYBW_BYTES)
__host__ __device__ inline uint32_t hybw_nodes(const OmSceneDev& S) {
    constexpr uint32_t kCap = OM_WF_HYBW_BYTES / (uint32_t)sizeof(OmBvh2NodeW);
    return S.n_b2wnodes < kCap ? S.n_b2wnodes : kCap;
}
__host__ __device__ inline uint32_t hyb4_nodes(const OmSceneDev& S) {
    constexpr uint32_t kCap = OM_WF_HYB4_BYTES / (uint32_t)sizeof(OmBvh4NodeH);
    return S.b4_lds_bytes ? 0u : (S.n_b4nodes < kCap ? S.n_b4nodes : kCap);
}
// k_march's instance for a marched set of exactly C2's shape (2 spheres, 1 box, 1 torus: S-marched):
// the SDF-only fields staged in LDS once per workgroup, every march step unrolled with no count
// guards; other marched sets read the scene arrays.  Traced parts TR_BRUTE /
// TR_BVH2_LDS only.
using MarchedC2Lds = MarchedExactLds<2, 1, 1>;
enum { MV_ARRAYS = 0, MV_EXACT_C2_LDS = 1 };
template <int TR>
__host__ __device__ constexpr bool exact_view_built() { return TR == TR_BRUTE || TR == TR_BVH2_LDS; }   // (not the TR_BARY forms)
// Bounce 0's deal of a batch of `paths` camera samples over nseg workgroups (om_deal.h): whole
// 64-sample blocks, so that a bounce-0 wave is exactly one 8x8 tile of one sample (tile-ordered
// pixel lists hold whole tiles).  Its capacity() is the segment capacity of the batch's queues.
__host__ __device__ inline Deal batch_deal(uint64_t paths, uint32_t nseg) { return make_deal(paths, nseg, OM_WF_DEAL_BLOCKS); }

extern __shared__ __attribute__((aligned(16))) uint4 wf_lds[];

struct Seg {
    uint32_t nseg;    // segments (= bounce workgroups)
    uint32_t segcap;  // paths per segment
};

// Adaptive calls: per stream and batch, the stream's live pixels listed for the
// batch (c, counted by the previous k_accumulate's compaction) and the call's samples rendered
// before it (done).  The batch's sample count is a function of the two, evaluated by every kernel
// of the batch (ad_batch), so the host never reads the count back.
struct AdPlan { uint32_t c, done; };
struct AdCfg {
    uint32_t sample_count;   // samples of the call
    uint32_t batches;        // batches per stream per call
    uint32_t paths;          // target paths per batch (c x b)
};
__host__ __device__ inline uint32_t ad_batch(uint32_t c, uint32_t done, uint32_t j, const AdCfg& A) {
    if (c == 0u || done >= A.sample_count || j >= A.batches) return 0u;
    const uint32_t rem = A.sample_count - done, left = A.batches - j;
    const uint32_t even = (rem + left - 1u) / left, want = A.paths / c;
    const uint32_t b = even > want ? even : want;
    return b < rem ? b : rem;
}
// a batch's adaptive list: the live list, its plan, the stream's next list and plan
struct AdList {
    const uint32_t* list;    // null: fixed-spp batch over the whole pixel list
    const AdPlan* plan;
    uint32_t* list_next;
    AdPlan* plan_next;
    AdCfg A;
    uint32_t j;              // batch index within the stream's call
};

// One SoA path queue: o|depthf, d|first_id, throughput|segment, rng s|rng k|slot|-.
// (SoA, not 64-B AoS records: AoS measured -22% on C1, r05_sort)
struct Queue {
    float4* q0; float4* q1; float4* q2; uint4* qr;
};

// Primary-ray source of bounce 0 (render_thread.rs:176-192).
struct Gen {
    OmCamDev C;
    const float2* jitter;
    const om_pixel_stats* stats;
    const uint32_t* pixels;      // tile-ordered pixel list
    uint32_t n_pixels, by_pixel, batch;
    const uint32_t* n0;          // concurrent fixed-spp calls: per listed pixel, Stats.n at the call start
    uint32_t done;               // samples of the call before this batch (with n0)
    AdList ad;                   // adaptive calls: the stream's live list (ad.list null otherwise)
    const uint32_t* tile_off;    // primary-ray candidate lists (null: traverse)
    const uint16_t* tile_idx;
    const float* tile_tnear;
};

// Path source of a ray_color batch (k_paths): the caller's rays and RNG states, from the batch's
// first path on.
struct RaySrc {
    const om_ray* rays;
    const uint64_t* rng;         // PathRng states (low word s, high word k); null: path_rng(skey, stream0 + i, sample)
    uint32_t n;                  // paths of the batch
    uint32_t stream0, sample;
};

// Path source of a render_rays batch (k_frame_paths): a rectangle of the call's sample-major ray
// table, `range` listed pixels from the batch's first one times `samples` samples from its first.
struct FrameSrc {
    const om_ray* rays;          // the ray of the batch's first pixel and sample; sample rows ray_stride apart
    const uint64_t* rng;         // PathRng states, the same layout; null: path_rng(skey, pixel, Stats.n + s_local)
    uint64_t ray_stride;         // listed pixels of the call
    const om_pixel_stats* stats; // the frame, by pixel
    const uint32_t* pixels;      // the batch's first list entry; null: pixel = pixel0 + kk
    uint32_t pixel0;
    uint32_t range, samples;     // range * samples paths; range is the result slots' sample stride
};

// A path between bounces: ray_color's loop state (render_thread.rs:128-143).
struct Path {
    F3 o, d, cur;
    float depthf;
    uint32_t first_id, seg, slot;
    Rng g;
};

// The path-state loads and stores carry the non-temporal hint: each 16-B lane record is read
// once per bounce and written once, so the streaming queues do not evict the leaf records and
// nodes the trace re-reads from the vector L1.  Component loads keep the scalar register shapes
// (a native 4-vector load moved k_bounce into scratch spills in r01); the compiler still merges
// them into global_load/store_dwordx4 ... nt.  C1: 7096 / 7114 vs 7094 / 7068 Msamples/s (r03_v13).
template <class V>
__device__ __forceinline__ V ld4(const V* q) {
    V v;
    v.x = __builtin_nontemporal_load(&q->x); v.y = __builtin_nontemporal_load(&q->y);
    v.z = __builtin_nontemporal_load(&q->z); v.w = __builtin_nontemporal_load(&q->w);
    return v;
}
__device__ __forceinline__ void load_ray(const Queue& Q, uint64_t i, Path& p) {
    const float4 a = ld4(Q.q0 + i), b = ld4(Q.q1 + i);
    p.o = f3(a.x, a.y, a.z); p.depthf = a.w;
    p.d = f3(b.x, b.y, b.z); p.first_id = __float_as_uint(b.w);
}
__device__ __forceinline__ void load_rest(const Queue& Q, uint64_t i, Path& p) {
    const float4 c = ld4(Q.q2 + i);
    const uint4 r = ld4(Q.qr + i);
    p.cur = f3(c.x, c.y, c.z); p.seg = __float_as_uint(c.w);
    p.g.s = r.x; p.g.k = r.y; p.slot = r.z;
}
template <class V>
__device__ __forceinline__ void st4(V* q, V v) {
    __builtin_nontemporal_store(v.x, &q->x); __builtin_nontemporal_store(v.y, &q->y);
    __builtin_nontemporal_store(v.z, &q->z); __builtin_nontemporal_store(v.w, &q->w);
}
__device__ __forceinline__ void store_path(const Queue& Q, uint64_t i, const Path& p) {
    st4(Q.q0 + i, make_float4(p.o.x, p.o.y, p.o.z, p.depthf));
    st4(Q.q1 + i, make_float4(p.d.x, p.d.y, p.d.z, __uint_as_float(p.first_id)));
    st4(Q.q2 + i, make_float4(p.cur.x, p.cur.y, p.cur.z, __uint_as_float(p.seg)));
    st4(Q.qr + i, make_uint4(p.g.s, p.g.k, p.slot, 0u));
}

// Scene data a workgroup traces against: the BVH2/BVH4 nodes + leaf table staged in LDS behind
// the per-lane stack ([stack][nodes][leaf table]), or (TR_BVH2_GLOBAL) the breadth-first prefix
// of the half-precision nodes in LDS and the rest read through L2.
struct Tracer {
    const B2Staged* b2n;     // TR_BVH2_LDS: f32 nodes in LDS (ray-ordered with OM_B2_PLANES)
    const OmBvh2NodeH* h2l;  // TR_BVH2_GLOBAL: half nodes [0, nl) staged in LDS
    const OmBvh2NodeH* h2g;  //                 every half node, through L2
    uint32_t nl;
    const OmBvh2NodeW* w2l;  // TR_BVH2_WIDE: wide nodes [0, nl) staged in LDS
    const OmBvh2NodeW* w2g;  //               every wide node, through L2
    uint32_t* stk32;         //               its u32 lane stack
    const OmBvh4Node* b4n;
    const OmBvh4NodeH* h4l;  // TR_BVH4_GLOBAL: half nodes [0, nl) staged in LDS
    const OmBvh4NodeH* h4g;  //                 every half node, through L2
    const uint32_t* bl;
    const OmAffineTest* recs;
    uint16_t* stk;
};

template <int TRF, uint32_t STACKS = 1>
__device__ __forceinline__ Tracer stage_scene(const OmSceneDev& S) {   // every thread of the block calls it
    constexpr int TR = tr_base(TRF);                                    // (staging does not depend on TR_BARY)
    Tracer t;
    t.stk = (uint16_t*)wf_lds + threadIdx.x;
    t.b2n = (const B2Staged*)S.b2nodes; t.b4n = S.b4nodes; t.bl = S.b2leaves; t.recs = S.srecs;
    t.h2l = S.b2h; t.h2g = S.b2h; t.nl = 0;
    t.h4l = S.b4h; t.h4g = S.b4h;
    t.w2l = wide_nodes(S); t.w2g = wide_nodes(S); t.stk32 = (uint32_t*)wf_lds + threadIdx.x;
    if (TR == TR_BVH4_GLOBAL && hyb4_nodes(S)) {
        t.nl = hyb4_nodes(S);
        uint4* dst = wf_lds + STACKS * stack_bytes<TR>(S) / 16u;
        const uint4* sn = (const uint4*)S.b4h;
        for (uint32_t i = threadIdx.x; i < t.nl * (uint32_t)(sizeof(OmBvh4NodeH) / 16u); i += kBlk) dst[i] = sn[i];
        __syncthreads();
        t.h4l = (const OmBvh4NodeH*)dst;
    }
    if (TR == TR_BVH2_WIDE && hybw_nodes(S)) {
        t.nl = hybw_nodes(S);
        uint4* dst = wf_lds + STACKS * stack_bytes<TR>(S) / 16u;
        const uint4* sn = (const uint4*)wide_nodes(S);
        for (uint32_t i = threadIdx.x; i < t.nl * (uint32_t)(sizeof(OmBvh2NodeW) / 16u); i += kBlk) dst[i] = sn[i];
        __syncthreads();
        t.w2l = (const OmBvh2NodeW*)dst;
    }
    if (TR == TR_BVH2_GLOBAL && hyb_nodes(S)) {
        t.nl = hyb_nodes(S);
        uint4* dst = wf_lds + STACKS * stack_bytes<TR>(S) / 16u;
        const uint4* sn = (const uint4*)S.b2h;
        for (uint32_t i = threadIdx.x; i < t.nl * (uint32_t)(sizeof(OmBvh2NodeH) / 16u); i += kBlk) dst[i] = sn[i];
        __syncthreads();
        t.h2l = (const OmBvh2NodeH*)dst;
    }
    if (TR == TR_BVH2_LDS || TR == TR_BVH4_LDS) {
        // uint4 words per node in memory / per node slot in LDS (BVH2: padded to kB2Stride)
        constexpr uint32_t wn = TR == TR_BVH2_LDS ? (uint32_t)(sizeof(OmBvh2Node) / 16u) : (uint32_t)(sizeof(OmBvh4Node) / 16u);
        constexpr uint32_t ws = TR == TR_BVH2_LDS ? kB2Stride / 16u : wn;
        const uint32_t nn = (TR == TR_BVH2_LDS ? S.n_b2nodes : S.n_b4nodes) * wn;
        const uint4* sn = TR == TR_BVH2_LDS ? (const uint4*)S.b2nodes : (const uint4*)S.b4nodes;
        uint4* dst = wf_lds + STACKS * stack_bytes<TR>(S) / 16u;
        if constexpr (TR == TR_BVH2_LDS && b2_ordered(TRF)) {
            // the node's 64 B into its slot by coalesced 16-B words, as below; then one node per
            // thread and turn, in place (read whole, then written): every (child, axis) as
            // [lo, hi, lo], the codes scaled as below (b2s_order)
            for (uint32_t i = threadIdx.x; i < nn; i += kBlk) dst[(i / wn) * ws + i % wn] = sn[i];
            __syncthreads();
            for (uint32_t n = threadIdx.x; n < S.n_b2nodes; n += kBlk) {
                OmBvh2NodeS* slot = (OmBvh2NodeS*)(dst + n * ws);
                const OmBvh2Node raw = *(const OmBvh2Node*)slot;
                *slot = b2s_order(raw, ws);
            }
        } else {
            for (uint32_t i = threadIdx.x; i < nn; i += kBlk) {
                uint4 v = sn[i];
                // BVH2 child codes (words 0 and 2: c0, c1) of internal nodes become slot offsets in
                // 16-B units, so the traversal addresses a node with a shift (traced_bvh2's CUNIT)
                if (TR == TR_BVH2_LDS && (i % wn) % 2u == 0u && v.w < OM_LEAF) v.w *= ws;
                dst[(i / wn) * ws + i % wn] = v;
            }
        }
        uint32_t* ldst = (uint32_t*)(dst + nn / wn * ws);
        for (uint32_t i = threadIdx.x; i < S.n_b2leaves; i += kBlk) ldst[i] = S.b2leaves[i];
        __syncthreads();
        t.b2n = (const B2Staged*)dst; t.b4n = (const OmBvh4Node*)dst; t.bl = ldst;
    }
    return t;
}

// Closest hit of one ray (hits.rs:270-365): -> (closest, global prim index or -1).
// MARCH is a compile-time split: the sphere-tracing code (3 SDFs + unstuck) would
// otherwise set the register budget of every traced-only scene.
// The traced section of variant TR over the window [tmin, closest]: -> global prim index or -1,
// closest = the winner's root.  (Wk::ANY: the first accepted primitive, om_trace.h.)
template <int TRF, class Wk>
__device__ __forceinline__ int trace_traced(const OmSceneDev& S, const Tracer& T, F3 o, F3 d, float tmin, float& closest, Wk& w) {
    constexpr int TR = tr_base(TRF);
    static_assert(Wk::BARY == tr_bary(TRF), "the work policy carries the variant's TR_BARY flag");
    if (TR == TR_BVH4_LDS) return traced_bvh4<kBlk>(S, T.b4n, T.bl, T.recs, T.stk, o, d, tmin, closest, w);
    if (TR == TR_BVH4_GLOBAL)
        return traced_bvh4<kBlk, Wk, true>(S, T.h4l, T.bl, T.recs, T.stk, o, d, tmin, closest, w, T.h4g, T.nl);
    if (TR == TR_BVH2_LDS) {
        if constexpr (b2_ordered(TRF))
            return traced_bvh2<kStackDepth, kBlk, Wk, false, OmBvh2NodeS, 16>(S, (const OmBvh2NodeS*)T.b2n, T.bl, T.recs, T.stk, o, d, tmin, closest, w);
        else
            return traced_bvh2<kStackDepth, kBlk, Wk, false, OmBvh2Node, 16>(S, (const OmBvh2Node*)T.b2n, T.bl, T.recs, T.stk, o, d, tmin, closest, w);
    }
    if (TR == TR_BVH2_GLOBAL)
        return traced_bvh2<kStackDepth, kBlk, Wk, true>(S, T.h2l, T.bl, T.recs, T.stk, o, d, tmin, closest, w, T.h2g, T.nl);
    if (TR == TR_BVH2_WIDE)
        return traced_bvh2<(int)kB2WideStack, kBlk, Wk, true>(S, T.w2l, T.bl, T.recs, T.stk32, o, d, tmin, closest, w, T.w2g, T.nl);
    if (TR == TR_SBVH_GLOBAL) return traced_sbvh(S, S.snodes, S.srecs, o, d, tmin, closest, w);
    if (TR == TR_BVH) return traced_bvh(S, o, d, tmin, closest, w);
    return traced_brute<TR == TR_CULLED>(S, o, d, tmin, closest, w);
}

template <int TR, bool MARCH, class Wk>
__device__ __forceinline__ int trace(const OmSceneDev& S, const OmParamsDev& P, const Tracer& T, F3 o, F3 d,
                                     float& closest, Wk& w) {
    closest = P.tmax;
    int best = trace_traced<TR>(S, T, o, d, P.tmin, closest, w);
    if (MARCH) {
        float tm;
        const int mg = march(S, o, d, P.tmin, P.tmax, closest, P.march_steps, tm, w);
        if (mg >= 0) { best = mg; closest = tm; }
    }
    return best;
}

// handle_hit + ray_color's termination rules (render_thread.rs:105-143) for one
// segment.  Returns true when the path continues (p advanced to the next segment);
// otherwise the sample's (colour, depth, id) is written to its result slot.
template <bool MARCH, bool USER = MARCH>
__device__ __forceinline__ bool shade_path(const OmSceneDev& S, const OmParamsDev& P, uint32_t cap, Path& p,
                                           float closest, int best, float4* __restrict__ res,
                                           uint32_t* __restrict__ res_id) {
    float seg_depth; uint32_t seg_id;
    if (best >= 0) {                                                   // handle_hit, Some(hr)
        F3 point, normal;
        finalize<MARCH, USER>(S, best, p.o, p.d, P.tmin, closest, point, normal);
        F3 nd, att;
        scatter(S.mats[best], p.d, normal, p.g, nd, att);
        p.cur = mul(p.cur, att);
        p.o = point; p.d = unit(nd);
        seg_depth = closest; seg_id = (uint32_t)best + 1u;
    } else {                                                           // None: sky (render_thread.rs:118-120)
        const float t = 0.5f * (p.d.y + 1.0f);
        p.cur = mul(p.cur, f3((1.0f - t) + 0.5f * t, (1.0f - t) + 0.7f * t, (1.0f - t) + 1.0f * t));
        seg_depth = INFINITY; seg_id = 0u;
    }
    bool finished = false;
    F3 result = p.cur;
    float rdepth = 0.0f; uint32_t rid = 0;
    if (p.seg == 0u) {
        p.depthf = seg_depth; p.first_id = seg_id;
        if (isinf(seg_depth)) { finished = true; rdepth = INFINITY; rid = 0u; }         // :133-135
    } else if (isinf(seg_depth)) {
        finished = true; rdepth = p.depthf; rid = p.first_id;                            // :138-140
    }
    if (!finished && p.seg + 1u >= cap) {                                          // :142 -Color::ZERO
        finished = true; result = f3(-0.0f, -0.0f, -0.0f); rdepth = p.depthf; rid = p.first_id;
    }
    if (finished) {
        res[p.slot] = make_float4(result.x, result.y, result.z, rdepth);
        res_id[p.slot] = rid;
        return false;
    }
    p.seg += 1u;
    return true;
}

// Camera sample i of the batch (render_thread.rs:176-192): -> p (a fresh path) and its
// pixel; false (and no sample recorded in res_id) when the sample is not taken.
// `stride` is the batch's pixel count: the whole list (fixed spp) or the stream's live list.
__device__ __forceinline__ bool gen_path(const OmParamsDev& P, const Gen& R, uint32_t stride, uint64_t i, Path& p,
                                         uint32_t& pixel, uint32_t* __restrict__ res_id) {
    const uint32_t s_local = (uint32_t)i / stride, kk = (uint32_t)i - s_local * stride;
    const uint32_t k = R.ad.list ? R.ad.list[kk] : kk;
    pixel = R.pixels[k];
    // the sample index is the pixel's Stats.n (jitters[pixel.stats.n], render_thread.rs:188).
    // Concurrent fixed-spp calls take it from the call-start snapshot plus the samples of the
    // batches before this one, so a batch never waits for the previous batch's accumulate.
    // Serial and adaptive calls read the live Stats: an adaptive stream's pixels are its own, and
    // its previous batch's accumulate has run on the same stream.
    uint32_t s;
    bool live;
    if (R.n0) {
        const uint32_t v = R.n0[k];
        s = (v & 0x7FFFFFFFu) + R.done + s_local;
        live = s < P.spp_total && !(v >> 31);
    } else {
        const om_pixel_stats& ps = R.stats[R.by_pixel ? pixel : k];
        s = ps.n + s_local;
        live = s < P.spp_total && !(P.adaptive && (ps.flags & 1u));
    }
    if (!live) {
        res_id[i] = kNoSample;
        return false;
    }
    p.g = path_rng(P.skey, pixel, s);
    const uint32_t line = pixel / P.width;
    gen_camera_ray(R.C, P, R.jitter, (float)(pixel - P.width * line), (float)line, s, p.g, p.o, p.d);
    p.cur = f3(1.0f, 1.0f, 1.0f); p.depthf = 0.0f; p.first_id = 0u; p.seg = 0u; p.slot = (uint32_t)i;
    return true;
}

// ---------------------------------------------------------------- bounce
// Workgroup s: the paths of segment s of queue `in` (FIRST: the 64-sample blocks of the batch
// that batch_deal gives workgroup s) -> survivors into segment s of `out`.
// HIT (split march pipeline): no trace here; the (closest, winner) of every path of the
// segment was written to `hitbuf` (queue-slot order) by k_march.
// Work distribution: every wave takes 64-path chunks of the segment from an
// LDS counter and appends its survivors with one LDS atomic, so the 8 waves never wait for each
// other.  Queue order within a segment then depends on which wave finishes first; results are
// keyed by slot and the RNG by (pixel, sample), never by queue position.
// FUSE (traced worlds' FIRST launch under OM_WF_FUSE_B1): the lanes whose path
// goes on after bounce 0 trace and shade bounce 1 in place, on the staged tree, and only then are
// compacted: `out` is bounce 2's queue, and the 64 B a bounce-1 path would be written and read
// back with never reach HBM.  A wave with no survivor (a tile of sky) skips the second segment.
template <int TR, bool COUNT, bool MARCH, bool FIRST, bool HIT = false, bool USER = MARCH>
__global__ __launch_bounds__(kBlk) OM_WAVES_ATTR void k_bounce(OmSceneDev S, OmParamsDev P, Seg G, Gen R, Queue in,
                                                 const uint32_t* __restrict__ count_in, Queue out,
                                                 uint32_t* __restrict__ count_out, float4* __restrict__ res,
                                                 uint32_t* __restrict__ res_id, unsigned long long* __restrict__ counters,
                                                 const float2* __restrict__ hitbuf, uint32_t* __restrict__ tail_next) {
    constexpr bool FUSE = FIRST && !MARCH && !HIT && kFuseB1;
    const uint64_t seg0 = (uint64_t)blockIdx.x * G.segcap;
    uint32_t n, stride = R.n_pixels;
    Deal dl{};                              // FIRST: the batch's deal; n counts this workgroup's blocks
    if (FIRST) {
        // the batch's traced tail claims paths from this word: zeroed here, launches ahead of it
        // on the same stream (no memset, no launch of its own)
        if (tail_next && blockIdx.x == 0 && threadIdx.x == 0) *tail_next = 0u;
        uint64_t paths = (uint64_t)R.n_pixels * R.batch;
        if (R.ad.list) {                    // adaptive: the stream's live list x the planned samples
            const AdPlan pl = uniform_load(R.ad.plan);
            stride = pl.c;
            paths = (uint64_t)pl.c * ad_batch(pl.c, pl.done, R.ad.j, R.ad.A);
        }
        dl = batch_deal(paths, G.nseg);
        n = dl.blocks_of(blockIdx.x);
    } else {
        n = count_in[blockIdx.x];
    }
    if (n == 0) {
        if (threadIdx.x == 0) count_out[blockIdx.x] = 0u;
        return;
    }
    __shared__ uint32_t q_next, q_out;
    if (threadIdx.x == 0) { q_next = kBlk / 64u; q_out = 0u; }
    __syncthreads();
    // (FIRST: the plain staged nodes, TR_PLAIN_NODES above)
    constexpr int TRS = FIRST ? (TR | TR_PLAIN_NODES) : TR;
    const Tracer T = HIT ? Tracer{} : stage_scene<TRS>(S);
    const uint32_t cap = depth_cap(P);
    WorkT<COUNT, false, tr_bary(TR)> w;
    uint32_t segs = 0;
    const uint32_t lane = __lane_id();
    const uint32_t chunks = FIRST ? n : (n + 63u) / 64u;
    for (uint32_t chunk = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); chunk < chunks;) {   // wave-uniform
        // FIRST: camera sample i of the batch (the deal's chunk-th block of this workgroup, the
        // batch's last block partial); else slot i of the in queue
        // (FUSE: a batch has at most 2^OM_WF_MAX_PATHS_LOG2 samples, so the sum fits 32 bits, and no
        // 64-bit lane index is kept in registers over the chunk loop)
        const uint64_t i = FUSE  ? (uint64_t)((uint32_t)(dl.block(blockIdx.x, chunk) * 64u) + lane)
                         : FIRST ? dl.block(blockIdx.x, chunk) * 64u + lane : seg0 + chunk * 64u + lane;
        bool keep = false;                 // the lane holds a live path
        Path p;
        uint32_t p_pixel = 0;
        if (FIRST ? i < dl.paths : chunk * 64u + lane < n) {
            if (FIRST) {
                // FUSE: the divisor of gen_path's i / stride made opaque per chunk, so that the
                // reciprocal of that division is worked out here (a dozen instructions per 64
                // paths) and not kept in a vector register over the chunk loop, where it spilled
                uint32_t st = stride;
                if (FUSE) asm volatile("" : "+s"(st));
                keep = gen_path(P, R, st, i, p, p_pixel, res_id);
            } else {
                load_ray(in, i, p);
                load_rest(in, i, p);       // issued before the trace: its latency hides behind it
                keep = true;
            }
        }
        // FIRST with candidate lists: bounce 0's closest hit from the tile's list (ahead of the segment
        // loop, whose trace is the tree's)
        float closest = 0.0f;
        int best = -1;
        const bool listed = FIRST && !HIT && (tr_base(TR) == TR_BVH2_LDS || tr_base(TR) == TR_BVH2_GLOBAL || tr_base(TR) == TR_BVH2_WIDE) && R.tile_off;
        if (listed && keep) {
            const uint32_t line = p_pixel / P.width;
            const uint32_t tile = (p_pixel - line * P.width) / 8u + (line / 8u) * P.tiles_x;
            closest = P.tmax;
            // a wave within one tile (all but where partial tiles meet) reads its list
            // and records with scalar loads
            const uint32_t t0 = __builtin_amdgcn_readfirstlane(tile);
            if (__ballot(tile != t0) == 0)
                best = traced_tiles<true>(S, R.tile_off, R.tile_idx, t0, p.o, p.d, P.tmin, closest, w, R.tile_tnear);
            else
                best = traced_tiles(S, R.tile_off, R.tile_idx, tile, p.o, p.d, P.tmin, closest, w);
            if (MARCH) {
                float tm;
                const int mg = march(S, p.o, p.d, P.tmin, P.tmax, closest, P.march_steps, tm, w);
                if (mg >= 0) { best = mg; closest = tm; }
            }
        }
        // one segment; FUSE: a second one for the wave's paths that go on, before any of them is queued
        // (one loop, so that the tree's trace and shade_path are in the kernel once)
#pragma clang loop unroll(disable)
        for (uint32_t sg = 0u;; ++sg) {
            if (keep) {
                if (HIT) {
                    const float2 h = hitbuf[i];
                    closest = h.x; best = __float_as_int(h.y);
                } else if (!(listed && sg == 0u)) {
                    best = trace<TRS, MARCH>(S, P, T, p.o, p.d, closest, w);
                }
                keep = shade_path<MARCH, USER>(S, P, cap, p, closest, best, res, res_id);
                if (COUNT) segs++;
            }
            if (!FUSE || sg == 1u || __ballot(keep) == 0) break;   // wave-uniform
        }
        const uint64_t m = __ballot(keep);
        uint32_t obase = 0u, nc = 0u;
        if (lane == 0) {
            obase = m ? atomicAdd(&q_out, (uint32_t)__popcll(m)) : 0u;
            nc = atomicAdd(&q_next, 1u);
        }
        obase = __builtin_amdgcn_readfirstlane(obase);
        chunk = __builtin_amdgcn_readfirstlane(nc);
        // the lane's rank among the wave's survivors (FUSE: counted by the mbcnt pair, no lane mask
        // kept in registers over the chunk loop)
        const uint32_t rank = FUSE ? __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))
                                   : (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (keep) store_path(out, seg0 + obase + rank, p);
    }
    __syncthreads();
    if (threadIdx.x == 0) count_out[blockIdx.x] = q_out;
    if (COUNT) {
        flush_counter(counters, OMC_SEGMENTS, segs);
        flush_counter(counters, OMC_PRIM_TESTS, w.prim);
        flush_counter(counters, OMC_PRE_TESTS, w.pre);
        flush_counter(counters, OMC_MARCH, w.march);
    }
}

// ---------------------------------------------------------------- split march pipeline
// k_raygen: the 64-sample blocks of the batch that batch_deal gives workgroup s; the taken samples
// are compacted into segment s of `out` (bounce 0 of the split pipeline reads them from there).
template <bool COUNT>
__global__ __launch_bounds__(kBlk) OM_WAVES_ATTR void k_raygen(OmParamsDev P, Seg G, Gen R, Queue out,
                                                 uint32_t* __restrict__ count_out, uint32_t* __restrict__ res_id) {
    const uint64_t seg0 = (uint64_t)blockIdx.x * G.segcap;
    uint64_t paths = (uint64_t)R.n_pixels * R.batch;
    uint32_t stride = R.n_pixels;
    if (R.ad.list) {                        // adaptive: the stream's live list x the planned samples
        const AdPlan pl = uniform_load(R.ad.plan);
        stride = pl.c;
        paths = (uint64_t)pl.c * ad_batch(pl.c, pl.done, R.ad.j, R.ad.A);
    }
    const Deal dl = batch_deal(paths, G.nseg);
    const uint32_t nblk = dl.blocks_of(blockIdx.x);
    __shared__ uint32_t q_out;
    if (threadIdx.x == 0) q_out = 0u;
    __syncthreads();
    const uint32_t lane = __lane_id();
    for (uint32_t c = threadIdx.x >> 6; c < nblk; c += kBlk / 64u) {   // wave c of the workgroup: its blocks c, c + 8, ...
        const uint64_t i = dl.block(blockIdx.x, c) * 64u + lane;   // (the batch's last block is partial)
        Path p;
        uint32_t pixel;
        const bool keep = i < dl.paths && gen_path(P, R, stride, i, p, pixel, res_id);
        const uint64_t m = __ballot(keep);
        uint32_t obase = 0u;
        if (lane == 0 && m) obase = atomicAdd(&q_out, (uint32_t)__popcll(m));
        obase = __builtin_amdgcn_readfirstlane(obase);
        if (keep) store_path(out, seg0 + obase + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)), p);
    }
    __syncthreads();
    if (threadIdx.x == 0) count_out[blockIdx.x] = q_out;
}

// k_march: closest traced hit + unstuck + sphere tracing (hits.rs:270-365) of every path of
// segment s of `in`, with LANE REFILL: a lane whose march ends writes (closest, winner) to
// hit[slot] and waits until OM_WF_REFILL lanes of its wave are idle; they then take the
// segment's next paths together (wave-aggregated LDS counter).  The wave's march iterations
// are then no longer the max over 64 paths' step counts.
template <int TR, bool COUNT, class M, class Wk>
__device__ __forceinline__ void march_lanes(const OmSceneDev& S, const OmParamsDev& P, const Tracer& T, const M& m,
                                            const Queue& in, uint64_t seg0, uint32_t n, uint32_t& next,
                                            float2* __restrict__ hit, Wk& w) {
    const uint32_t lane = __lane_id();
    uint32_t j = threadIdx.x;
    bool act = j < n, marching = false;
    bool dry = !act;                                   // the segment has no path left for this lane
    F3 o = f3(0.0f, 0.0f, 0.0f), d = o;
    float t = 0.0f, closest = 0.0f;
    int best = -1;
    uint32_t iters = 0;
    auto start = [&]() {
        const float4 a = in.q0[seg0 + j], b = in.q1[seg0 + j];
        o = f3(a.x, a.y, a.z); d = f3(b.x, b.y, b.z);
        best = trace<TR, false>(S, P, T, o, d, closest, w);
        marching = march_begin(m, o, d, P.tmin, t);
        iters = P.march_steps;
    };
    if (act) start();
    for (;;) {
#pragma unroll
        for (int u = 0; u < OM_MARCH_UNROLL; ++u) {     // march steps between refill checks
            if (act) {
                int gi = -1;
                const int r = marching ? march_step(S, m, o, d, P.tmax, closest, t, iters, gi, w) : 2;
                if (r != 0) {
                    if (r == 1) { best = gi; closest = t; }
                    hit[seg0 + j] = make_float2(closest, __int_as_float(best));
                    act = false;
                }
            }
        }
        // refill the idle lanes together once enough of them wait (or nothing else runs):
        // a refill runs the trace and unstuck, which costs several march steps
        const uint64_t want = __ballot(!act && !dry), busy = __ballot(act);
        if (want && (__popcll(want) >= OM_WF_REFILL || busy == 0)) {
            uint32_t base = 0u;
            if (lane == 0) base = atomicAdd(&next, (uint32_t)__popcll(want));
            base = __builtin_amdgcn_readfirstlane(base);
            if (!act && !dry) {
                j = base + (uint32_t)__popcll(want & ((1ull << lane) - 1ull));
                if (j < n) { act = true; start(); } else dry = true;
            }
        }
        if (__ballot(act) == 0) break;
    }
}

template <int TR, bool COUNT, int VIEW>
__global__ __launch_bounds__(kBlk) OM_WAVES_ATTR void k_march(OmSceneDev S, OmParamsDev P, Seg G, Queue in,
                                                const uint32_t* __restrict__ count_in, float2* __restrict__ hit,
                                                unsigned long long* __restrict__ counters) {
    const uint32_t n = count_in[blockIdx.x];
    if (n == 0) return;
    const uint64_t seg0 = (uint64_t)blockIdx.x * G.segcap;
    __shared__ uint32_t next;
    if (threadIdx.x == 0) next = kBlk;
    __syncthreads();
    const Tracer T = stage_scene<TR>(S);
    WorkT<COUNT, false, tr_bary(TR)> w;
    if constexpr (VIEW == MV_EXACT_C2_LDS) {
        __shared__ MarchedC2Lds::Block mblock;
        march_lanes<TR, COUNT>(S, P, T, MarchedC2Lds(S, &mblock), in, seg0, n, next, hit, w);
    } else {
        march_lanes<TR, COUNT>(S, P, T, MarchedArrays(S), in, seg0, n, next, hit, w);
    }
    if (COUNT) {
        flush_counter(counters, OMC_PRIM_TESTS, w.prim);
        flush_counter(counters, OMC_PRE_TESTS, w.pre);
        flush_counter(counters, OMC_MARCH, w.march);
    }
}

// ---------------------------------------------------------------- tail
// Every path of queue `in`, each run to completion, lanes refilled as their paths end, in a
// single loop:
//   traced worlds  (k_tail) a resident grid over the whole queue: the paths are numbered through
//                  the exclusive prefix of the segment counts and dealt in 64-path units evenly
//                  over workgroups and wave slots.  One segment (trace +
//                  shade) per iteration; a lane whose path ended takes the next undealt path at
//                  once, so it never waits for the longest path of its wave;
//   marched worlds (k_tail_march) workgroup b owns segments [b*kTailSpb, (b+1)*kTailSpb): the
//                  k_march scheme (march_lanes) inside the tail: OM_MARCH_UNROLL march steps per
//                  iteration, a lane whose march ended shades and starts its next segment, lanes
//                  whose path ended are refilled together once OM_WF_REFILL of them wait.
// (r04: C2 +8.3% over the r03 nested loop, in which every lane ran its path to completion before
// it took another; C1 and C3 within 0.3%.)
// Path idx of the ns segments from s0 on, numbered through pre[0 .. ns] (exclusive prefix of their
// counts, in LDS): segment by binary search.  Empty segments repeat a prefix value; the search
// keeps the last of them, the one that holds idx.
struct TailSrc {
    const Queue& in;
    const uint32_t* pre;
    uint32_t s0, ns, segcap;
    __device__ __forceinline__ bool load(uint32_t idx, Path& p) const {
        uint32_t lo = 0, hi = ns;                           // pre[lo] <= idx < pre[hi]
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (pre[mid] <= idx) lo = mid; else hi = mid;
        }
        const uint64_t i = (uint64_t)(s0 + lo) * segcap + (idx - pre[lo]);
        load_ray(in, i, p);
        load_rest(in, i, p);
        return true;                                        // (a queued path is always live)
    }
};
template <int TR, bool COUNT, class M, class Src, class Wk>
__device__ __forceinline__ uint32_t tail_march_lanes(const OmSceneDev& S, const OmParamsDev& P, const Tracer& T, const M& m,
                                                     const Src& src, uint32_t total, uint32_t& next,
                                                     float4* __restrict__ res, uint32_t* __restrict__ res_id, Wk& w) {
    const uint32_t lane = __lane_id();
    const uint32_t cap = depth_cap(P);
    uint32_t idx = threadIdx.x, segs = 0, iters = 0;
    bool have = idx < total, dry = !have, marching = false, act = false;
    // The march steps need only the ray; the rest of the path (throughput, first hit, segment,
    // slot, RNG) is parked in LDS until the next shade (18 KB per workgroup), so it does not sit
    // in registers across the march loop: C2's tail spilled 40 B per lane with it in registers,
    // 12 B parked (C2 3301 vs 3275 Msamples/s, r04_ab8).
    __shared__ uint32_t rest[9][kBlk];
    Path p;
    float t = 0.0f, closest = 0.0f;
    int best = -1;
    auto park = [&]() {
        const uint32_t i = threadIdx.x;
        rest[0][i] = __float_as_uint(p.cur.x); rest[1][i] = __float_as_uint(p.cur.y); rest[2][i] = __float_as_uint(p.cur.z);
        rest[3][i] = __float_as_uint(p.depthf); rest[4][i] = p.first_id; rest[5][i] = p.seg; rest[6][i] = p.slot;
        rest[7][i] = p.g.s; rest[8][i] = p.g.k;
    };
    auto unpark = [&]() {
        const uint32_t i = threadIdx.x;
        p.cur = f3(__uint_as_float(rest[0][i]), __uint_as_float(rest[1][i]), __uint_as_float(rest[2][i]));
        p.depthf = __uint_as_float(rest[3][i]); p.first_id = rest[4][i]; p.seg = rest[5][i]; p.slot = rest[6][i];
        p.g.s = rest[7][i]; p.g.k = rest[8][i];
    };
    auto begin = [&]() {                                    // closest traced hit + unstuck of the segment
        park();
        best = trace<TR, false>(S, P, T, p.o, p.d, closest, w);
        marching = march_begin(m, p.o, p.d, P.tmin, t);
        iters = P.march_steps;
        act = true;
    };
    if (have) { have = src.load(idx, p); if (have) begin(); }
    for (;;) {
#pragma unroll
        for (int u = 0; u < OM_WF_TAIL_UNROLL; ++u) {         // march steps between checks
            if (act) {
                int gi = -1;
                const int r = marching ? march_step(S, m, p.o, p.d, P.tmax, closest, t, iters, gi, w) : 2;
                if (r != 0) {
                    if (r == 1) { best = gi; closest = t; }
                    act = false;
                }
            }
        }
        // march ended: handle_hit, next segment or done -- for the wave's ended lanes together, once
        // OM_WF_TAIL_SHADE of them wait or none marches
        // (the ballots are taken before the branch, with every lane active: inside it only the
        // ended lanes run, whose act is false, so a ballot of act there would always be 0)
        const bool ended = have && !act;
        const uint64_t em = __ballot(ended), am = __ballot(act);
        if (ended && (OM_WF_TAIL_SHADE <= 1 || __popcll(em) >= OM_WF_TAIL_SHADE || am == 0)) {
            if (COUNT) segs++;
            unpark();
            if (shade_path<true, M::USER>(S, P, cap, p, closest, best, res, res_id)) begin();
            else have = false;
        }
        const uint64_t want = __ballot(!have && !dry), busy = __ballot(have);
        if (want && (__popcll(want) >= OM_WF_TAIL_REFILL || busy == 0)) {
            uint32_t base = 0u;
            if (lane == 0) base = atomicAdd(&next, (uint32_t)__popcll(want));
            base = __builtin_amdgcn_readfirstlane(base);
            if (!have && !dry) {
                idx = base + (uint32_t)__popcll(want & ((1ull << lane) - 1ull));
                if (idx < total) { have = src.load(idx, p); if (have) begin(); } else dry = true;
            }
        }
        if (__ballot(have || !dry) == 0) break;             // (a lane not dry is refilled next time round)
    }
    return segs;
}

template <int TR, bool COUNT, int VIEW = MV_ARRAYS, uint32_t SPB = kTailSpb>
__global__ __launch_bounds__(kBlk) __attribute__((amdgpu_waves_per_eu(OM_WF_TAIL_MARCH_WAVES, OM_WF_TAIL_MARCH_WAVES)))
void k_tail_march(OmSceneDev S, OmParamsDev P, Seg G, Queue in,
                                               const uint32_t* __restrict__ count_in, float4* __restrict__ res,
                                               uint32_t* __restrict__ res_id, unsigned long long* __restrict__ counters) {
    __shared__ uint32_t pre[SPB + 1];
    __shared__ uint32_t next;
    const uint32_t s0 = blockIdx.x * SPB;
    if (threadIdx.x == 0) {
        uint32_t acc = 0;
        for (uint32_t k = 0; k < SPB; ++k) {
            pre[k] = acc;
            acc += s0 + k < G.nseg ? count_in[s0 + k] : 0u;
        }
        pre[SPB] = acc;
        next = kBlk;
    }
    __syncthreads();
    const uint32_t total = pre[SPB];
    if (total == 0) return;
    const Tracer T = stage_scene<TR>(S);
    const TailSrc src{in, pre, s0, SPB, G.segcap};
    WorkT<COUNT, false, tr_bary(TR)> w;
    uint32_t segs = 0;
    if constexpr (VIEW == MV_EXACT_C2_LDS) {
        __shared__ MarchedC2Lds::Block mblock;
        segs = tail_march_lanes<TR, COUNT>(S, P, T, MarchedC2Lds(S, &mblock), src, total, next, res, res_id, w);
    } else {
        segs = tail_march_lanes<TR, COUNT>(S, P, T, MarchedArrays(S), src, total, next, res, res_id, w);
    }
    if (COUNT) {
        flush_counter(counters, OMC_SEGMENTS, segs);
        flush_counter(counters, OMC_PRIM_TESTS, w.prim);
        flush_counter(counters, OMC_PRE_TESTS, w.pre);
        flush_counter(counters, OMC_MARCH, w.march);
    }
}

// The traced tail.  gridDim.x workgroups, all resident (the host sizes the grid from the CU count);
// every one of them
//   1. scans count_in[0 .. G.nseg) into pre[0 .. G.nseg] (dynamic LDS at byte pre_off, behind what
//      stage_scene fills) and leaves before staging when the queue is empty;
//   2. takes its share of the first gridDim.x * kWaves units of 64 consecutive paths: unit u runs
//      in workgroup u % gridDim.x on wave slot (u / gridDim.x + workgroup) % kWaves, so a light
//      tail puts one or two dense waves in each workgroup, on different slots in neighbouring
//      workgroups, instead of filling slots 0, 1, .. of a few;
//   3. (queues longer than the grid's lanes) refills ended lanes from *next, the queue set's claim
//      counter (zeroed by the batch's bounce 0): one atomic per wave and iteration for all of the
//      wave's idle lanes, and none once the counter has passed the end of the queue.
// No workgroup waits for another, and no barrier follows the staging barrier.
template <int TR, bool COUNT>
__global__ __launch_bounds__(kBlk) OM_WAVES_ATTR
void k_tail(OmSceneDev S, OmParamsDev P, Seg G, Queue in, const uint32_t* __restrict__ count_in, uint32_t pre_off,
            uint32_t* __restrict__ next, float4* __restrict__ res, uint32_t* __restrict__ res_id,
            unsigned long long* __restrict__ counters) {
    uint32_t* pre = (uint32_t*)wf_lds + pre_off / 4u;
    __shared__ uint32_t wave_sum[kWaves];
    const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
    // thread t scans counts [t*per, (t+1)*per): its sum, the wave's inclusive scan of the sums,
    // the waves' totals through LDS
    const uint32_t per = (G.nseg + kBlk - 1u) / kBlk;
    const uint32_t c0 = threadIdx.x * per, c1 = c0 + per < G.nseg ? c0 + per : G.nseg;
    uint32_t mine = 0;
    for (uint32_t k = c0; k < c1; ++k) mine += count_in[k];
    uint32_t incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = __shfl_up(incl, off, 64);
        if (lane >= (uint32_t)off) incl += v;
    }
    if (lane == 63u) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t acc = incl - mine, total = 0;
#pragma unroll
    for (uint32_t k = 0; k < kWaves; ++k) {
        const uint32_t v = wave_sum[k];
        if (k < wave) acc += v;
        total += v;
    }
    if (total == 0) return;                                   // (uniform over the grid)
    for (uint32_t k = c0; k < c1; ++k) { pre[k] = acc; acc += count_in[k]; }
    if (threadIdx.x == 0) pre[G.nseg] = total;
    __syncthreads();
    const Tracer T = stage_scene<TR>(S);
    const uint32_t cap = depth_cap(P);
    const TailSrc src{in, pre, 0u, G.nseg, G.segcap};
    WorkT<COUNT, false, tr_bary(TR)> w;
    uint32_t segs = 0;
    const uint32_t lanes = gridDim.x * kBlk;                  // paths [0, lanes) are dealt, the rest claimed
    const uint32_t round = (wave + kWaves - blockIdx.x % kWaves) % kWaves;
    uint32_t idx = (round * gridDim.x + blockIdx.x) * 64u + lane;
    bool have = idx < total;
    bool more = total > lanes;                                // wave-uniform: undealt paths may remain
    Path p;
    if (have) src.load(idx, p);
    for (;;) {
        if (have) {
            float closest;
            const int best = trace<TR, false>(S, P, T, p.o, p.d, closest, w);
            if (COUNT) segs++;
            have = shade_path<false>(S, P, cap, p, closest, best, res, res_id);
        }
        if (more) {                                           // the ended lanes' next paths at once
            const uint64_t want = __ballot(!have);
            if (want) {
                const uint32_t nw = (uint32_t)__popcll(want);
                uint32_t base = 0u;
                if (lane == 0) base = atomicAdd(next, nw);
                base = lanes + __builtin_amdgcn_readfirstlane(base);
                if (!have) {
                    idx = base + (uint32_t)__popcll(want & ((1ull << lane) - 1ull));
                    have = idx < total;
                    if (have) src.load(idx, p);
                }
                more = base + nw < total;
            }
        }
        if (__ballot(have) == 0) break;
    }
    if (COUNT) {
        flush_counter(counters, OMC_SEGMENTS, segs);
        flush_counter(counters, OMC_PRIM_TESTS, w.prim);
        flush_counter(counters, OMC_PRE_TESTS, w.pre);
        flush_counter(counters, OMC_MARCH, w.march);
    }
}

// ---------------------------------------------------------------- ray queries
// k_query: FrozenHittableList::hit (hits.rs:270-334) for n caller-given rays, one om_hit each: the
// trace and the HitRecord code of the bounce kernels, with no camera, shading or queue (DESIGN.md
// §5.15).  Persistent: at most a resident grid of workgroups, each staging the scene once
// (stage_scene's tree copy is the cost floor of a small launch) and then taking the ray blocks
// b, b + gridDim.x, ...  Lanes past n in the last block only skip the trace; nothing after the
// staging synchronises the workgroup.
// The direction is used as given (the `Ray { orig, dir }` literal): a unit direction is the
// documented precondition (Ray::new, ray.rs:12); the march's step and the traversal's culls
// assume it, and results for non-unit directions are unspecified.  Non-finite rays take the
// reference loop (see the ray loop).
// Rays (24 B) and hits (32 B) are streamed once each with the non-temporal hint, like the path
// queues, so they do not evict nodes and leaf records from the vector L1; buffers aligned to
// 8 / 16 B (wave-uniform test) move as dwordx2 / dwordx4.
//
// Per-ray windows (WIN; om_ray_window, 8 B per ray, read once like the rays): ray i
// is answered for [tmin_i, tmax_i] instead of the call's window.  The tree culls derive
// t_lo = tmin / 2 - 1e-3, which is above tmin for tmin < -2e-3, and nothing in them is specified for a
// NaN bound; so a lane whose window has tmin < 0 or a NaN bound (window_edge) takes the reference
// loop, as a lane with a non-finite ray does.  Every other window is one the culls are conservative
// for: t_hi = tmax * 1.0001 + 1e-3 >= tmax for every tmax that can hold a root >= tmin >= 0 (+inf
// included), and a window with tmin > tmax accepts nothing in either form.
__device__ __forceinline__ bool window_edge(float tmin, float tmax) { return !(tmin >= 0.0f) || tmax != tmax; }
// A query ray beyond the reach of the slab test takes the reference loop as well: with the origin d
// (largest axis distance) from the box of the bounded primitives (the root of the global BVH, which
// every kernel's upload holds), of diagonal R, the slab test's own rounding reaches the inflation's
// floor of 1e-3 once 2 sqrt(3) d + R passes OM_SLAB_REACH (om_tuning.h).  A NaN origin
// compares false and keeps the non-finite path.
__device__ __forceinline__ bool far_origin(const OmSceneDev& S, F3 o) {
    if (S.n_bvh_nodes == 0) return false;
    const OmBvhNode N = S.bvh[0];
    return beyond_slab_reach(N.lo, N.hi, o.x, o.y, o.z);
}
__device__ __forceinline__ void load_query_window(const om_ray_window* __restrict__ win, uint64_t i, float& tmin, float& tmax) {
    if (((uintptr_t)win & 7u) == 0u) {
        const float2* w2 = (const float2*)(win + i);
        tmin = __builtin_nontemporal_load(&w2->x); tmax = __builtin_nontemporal_load(&w2->y);
    } else {
        const float* w = (const float*)(win + i);
        tmin = __builtin_nontemporal_load(w); tmax = __builtin_nontemporal_load(w + 1);
    }
}
__device__ __forceinline__ void load_query_ray(const om_ray* __restrict__ rays, uint64_t i, F3& o, F3& d) {
    const float* r = (const float*)(rays + i);
    if (((uintptr_t)rays & 7u) == 0u) {
        const float2* r2 = (const float2*)r;
        float2 a, b, c;
        a.x = __builtin_nontemporal_load(&r2[0].x); a.y = __builtin_nontemporal_load(&r2[0].y);
        b.x = __builtin_nontemporal_load(&r2[1].x); b.y = __builtin_nontemporal_load(&r2[1].y);
        c.x = __builtin_nontemporal_load(&r2[2].x); c.y = __builtin_nontemporal_load(&r2[2].y);
        o = f3(a.x, a.y, b.x); d = f3(b.y, c.x, c.y);
    } else {
        o = f3(__builtin_nontemporal_load(r), __builtin_nontemporal_load(r + 1), __builtin_nontemporal_load(r + 2));
        d = f3(__builtin_nontemporal_load(r + 3), __builtin_nontemporal_load(r + 4), __builtin_nontemporal_load(r + 5));
    }
}
__device__ __forceinline__ void store_query_hit(om_hit* __restrict__ hits, uint64_t i, float t, F3 p, F3 n, uint32_t obj) {
    if (((uintptr_t)hits & 15u) == 0u) {
        float4* h = (float4*)(hits + i);
        st4(h, make_float4(t, p.x, p.y, p.z));
        st4(h + 1, make_float4(n.x, n.y, n.z, __uint_as_float(obj)));
    } else {
        float* h = (float*)(hits + i);
        __builtin_nontemporal_store(t, h);
        __builtin_nontemporal_store(p.x, h + 1); __builtin_nontemporal_store(p.y, h + 2); __builtin_nontemporal_store(p.z, h + 3);
        __builtin_nontemporal_store(n.x, h + 4); __builtin_nontemporal_store(n.y, h + 5); __builtin_nontemporal_store(n.z, h + 6);
        __builtin_nontemporal_store(__uint_as_float(obj), h + 7);
    }
}

// A lane of the persistent k_query counts over every block its workgroup takes, up to 2^32 / (grid x
// 512) rays of any cost, so its totals and the wave's sum are kept in 64 bits (WorkT's u32 fields
// hold one ray's counts); a render kernel's lane counts a bounded number of segments and sums in 32.
__device__ __forceinline__ void flush_counter64(unsigned long long* ctr, int slot, unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (__lane_id() == 0 && v) atomicAdd(&ctr[slot], v);
}

template <int TR, bool MARCH, bool USER, bool COUNT, bool WIN>
__device__ __forceinline__ void query_rays(const OmSceneDev& S, const OmParamsDev& P, const om_ray* __restrict__ rays,
                                           const om_ray_window* __restrict__ windows, uint32_t n, om_hit* __restrict__ hits,
                                           unsigned long long* __restrict__ counters) {
    const Tracer T = stage_scene<TR>(S);
    unsigned long long segs = 0, n_prim = 0, n_pre = 0, n_march = 0;
    const uint32_t nblocks = (uint32_t)(((uint64_t)n + kBlk - 1u) / kBlk);
    for (uint32_t b = blockIdx.x; b < nblocks; b += gridDim.x) {      // (b + gridDim.x <= 2^23 + 2^23: no wrap)
        const uint64_t i = (uint64_t)b * kBlk + threadIdx.x;
        if (i >= n) continue;
        WorkT<COUNT, false, tr_bary(TR)> w;                      // this ray's work
        F3 o, d;
        load_query_ray(rays, i, o, d);
        float closest;
        int best;
        // The tree traversals answer a non-finite ray with nonfinite_hit's closed form, which is the
        // reference loop's answer when a component is NaN but not always when one is infinite (an
        // infinite root is rejected where a NaN root is accepted).  A query can be handed any ray,
        // so such rays (never a whole wave in practice) run the reference loop itself.
        constexpr int T0 = tr_base(TR);
        constexpr bool kShortcut = T0 == TR_BVH2_LDS || T0 == TR_BVH2_GLOBAL || T0 == TR_BVH4_LDS || T0 == TR_BVH4_GLOBAL || T0 == TR_BVH2_WIDE;
        float tmin = P.tmin, tmax = P.tmax;
        if (WIN) load_query_window(windows, i, tmin, tmax);
        if ((kShortcut && !isfinite(o.x + o.y + o.z + d.x + d.y + d.z)) || (WIN && window_edge(tmin, tmax)) || far_origin(S, o)) {
            closest = tmax;
            best = traced_brute<false>(S, o, d, tmin, closest, w);
        } else {
            closest = tmax;
            best = trace_traced<TR>(S, T, o, d, tmin, closest, w);
        }
        if (MARCH) {                                             // trace<TR, true>'s march, once for both branches
            float tm;
            const int mg = march(S, o, d, tmin, tmax, closest, P.march_steps, tm, w);
            if (mg >= 0) { best = mg; closest = tm; }
        }
        if (COUNT) { segs++; n_prim += w.prim; n_pre += w.pre; n_march += w.march; }
        F3 point = f3(0.0f, 0.0f, 0.0f), normal = point;
        if (best >= 0) finalize<MARCH, USER>(S, best, o, d, tmin, closest, point, normal);
        else closest = INFINITY;
        store_query_hit(hits, i, closest, point, normal, (uint32_t)(best + 1));
    }
    if (COUNT) {
        flush_counter64(counters, OMC_SEGMENTS, segs);
        flush_counter64(counters, OMC_PRIM_TESTS, n_prim);
        flush_counter64(counters, OMC_PRE_TESTS, n_pre);
        flush_counter64(counters, OMC_MARCH, n_march);
    }
}
template <int TR, bool MARCH, bool USER, bool COUNT>
__global__ __launch_bounds__(kBlk) OM_WAVES_ATTR void k_query(OmSceneDev S, OmParamsDev P, const om_ray* __restrict__ rays,
                                                uint32_t n, om_hit* __restrict__ hits,
                                                unsigned long long* __restrict__ counters) {
    query_rays<TR, MARCH, USER, COUNT, false>(S, P, rays, nullptr, n, hits, counters);
}
// k_query with one window per ray (om_hit_rays_windows_device)
template <int TR, bool MARCH, bool USER, bool COUNT>
__global__ __launch_bounds__(kBlk) OM_WAVES_ATTR void k_query_windows(OmSceneDev S, OmParamsDev P, const om_ray* __restrict__ rays,
                                                        const om_ray_window* __restrict__ windows, uint32_t n,
                                                        om_hit* __restrict__ hits, unsigned long long* __restrict__ counters) {
    query_rays<TR, MARCH, USER, COUNT, true>(S, P, rays, windows, n, hits, counters);
}

// k_occluded: FrozenHittableList::hit(ray, tmin, tmax).is_some() for n rays, one byte each (0 / 1),
// DESIGN.md §5.16.  k_query's frame (persistent grid, one staging, no later barrier) around the
// any-hit forms of the traversals (WorkT<., true>): a lane leaves its traversal at the first accepted
// exact test and then idles until its wave's block is done.  The answer does not depend on the
// order of the tests: until the first acceptance every test sees closest = tmax, exactly the
// reference loop's state before its first acceptance, and after one the result is Some whatever
// follows.  The march runs only for lanes no traced primitive answered, with closest = tmax; there
// is no HitRecord, so no finalize and no SDF normals.
// The window is per lane either way (`windows` null: the call's, a wave-uniform switch); window_edge
// windows and non-finite rays take the reference loop for every variant.
// Each lane stores its own byte: any n and any alignment of `out` touch exactly [out, out + n).
template <int TR, bool MARCH, bool COUNT>
__global__ __launch_bounds__(kBlk) OM_WAVES_ATTR void k_occluded(OmSceneDev S, OmParamsDev P, const om_ray* __restrict__ rays,
                                                   const om_ray_window* __restrict__ windows, uint32_t n,
                                                   uint8_t* __restrict__ out, unsigned long long* __restrict__ counters) {
    const Tracer T = stage_scene<TR>(S);
    const uint32_t nblocks = (uint32_t)(((uint64_t)n + kBlk - 1u) / kBlk);
    for (uint32_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const uint64_t i = (uint64_t)b * kBlk + threadIdx.x;
        WorkT<COUNT, true, tr_bary(TR)> w;
        if (i < n) {
            F3 o, d;
            load_query_ray(rays, i, o, d);
            float tmin = P.tmin, tmax = P.tmax;
            if (windows) load_query_window(windows, i, tmin, tmax);
            float closest = tmax;
            int best;
            if (!isfinite(o.x + o.y + o.z + d.x + d.y + d.z) || window_edge(tmin, tmax) || far_origin(S, o)) best = traced_brute<false>(S, o, d, tmin, closest, w);
            else best = trace_traced<TR>(S, T, o, d, tmin, closest, w);
            if (MARCH && best < 0) {
                float tm;
                best = march(S, o, d, tmin, tmax, tmax, P.march_steps, tm, w);
            }
            out[i] = best >= 0 ? (uint8_t)1 : (uint8_t)0;
        }
        // counted per block, where every lane of the wave is back: no 64-bit totals stay live across
        // the traversals as in k_query (24 B less scratch in most marched counting variants)
        if (COUNT) {
            flush_counter64(counters, OMC_SEGMENTS, i < n ? 1ull : 0ull);
            flush_counter64(counters, OMC_PRIM_TESTS, w.prim);
            flush_counter64(counters, OMC_PRE_TESTS, w.pre);
            flush_counter64(counters, OMC_MARCH, w.march);
        }
    }
}

// ---------------------------------------------------------------- path queries
// k_paths: segment 0 of ray_color (render_thread.rs:128-143) for the caller's rays of one batch
// (om_ray_color*): bounce 0 of the wavefront with (rays[i], rng state) in the place
// of gen_path.  The batch's 64-path blocks are dealt over the workgroups as bounce 0 deals camera
// samples (batch_deal), a path's result slot is its index in the batch, and the survivors are
// compacted into segment s of `out`, bounce 1's queue, by k_bounce's ballot and LDS counters; the
// per-bounce launches and the tails take them from there unchanged.  There are no tile lists and no
// fused second segment: these are not camera rays, and a wave of them is no 8x8 tile.
// A ray can be any ray.  A lane whose origin is beyond the slab test's reach (far_origin) runs the
// reference loop for segment 0, as in query_rays.  A ray with a NaN or infinite component is not
// traced at all: its path ends here with the record (colour NaN, depth +inf, obj 0) and counts no
// segment.  Such a path would stay non-finite in every later segment, and in a world with a
// MarchedBox each of them can cost 2^22 SDF evaluations: the box's sdf of a NaN point is <= 0 (fmaxf /
// fminf drop the NaN, as f32::max / min do: len(max(q, 0)) = 0, min(max(q.x, q.y, q.z), 0) <= 0), so
// unstuck's loop (hits.rs:360-363, endless in the reference) runs to march_begin's safety cap.  One
// garbage ray would then hold the device for max_depth times that.  Marched worlds march segment 0
// here (march(), as k_query<., MARCH>), and their survivors go to the marched tail or the k_march launches.
// The RNG state of path i is rng[i] (low word the Weyl counter, high word the key) or, with rng
// null, path_rng(P.skey, stream0 + i, sample): a pixel index that wraps mod 2^32.
template <int TR, bool COUNT, bool MARCH, bool USER>
__global__ __launch_bounds__(kBlk) OM_WAVES_ATTR void k_paths(OmSceneDev S, OmParamsDev P, Seg G, RaySrc R, Queue out,
                                                uint32_t* __restrict__ count_out, float4* __restrict__ res,
                                                uint32_t* __restrict__ res_id, unsigned long long* __restrict__ counters,
                                                uint32_t* __restrict__ tail_next) {
    // the traced tail's claim counter, as k_bounce<FIRST> zeroes it
    if (tail_next && blockIdx.x == 0 && threadIdx.x == 0) *tail_next = 0u;
    const uint64_t seg0 = (uint64_t)blockIdx.x * G.segcap;
    const Deal dl = batch_deal(R.n, G.nseg);
    const uint32_t chunks = dl.blocks_of(blockIdx.x);
    if (chunks == 0) {
        if (threadIdx.x == 0) count_out[blockIdx.x] = 0u;
        return;
    }
    __shared__ uint32_t q_next, q_out;
    if (threadIdx.x == 0) { q_next = kBlk / 64u; q_out = 0u; }
    __syncthreads();
    const Tracer T = stage_scene<TR>(S);
    const uint32_t cap = depth_cap(P);
    WorkT<COUNT, false, tr_bary(TR)> w;
    uint32_t segs = 0;
    const uint32_t lane = __lane_id();
    for (uint32_t chunk = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); chunk < chunks;) {   // wave-uniform
        // (a batch has at most 2^OM_WF_MAX_PATHS_LOG2 paths: the index fits 32 bits)
        const uint32_t i = (uint32_t)(dl.block(blockIdx.x, chunk) * 64u) + lane;
        bool keep = false;
        Path p;
        bool live = i < R.n;
        if (live) {
            load_query_ray(R.rays, i, p.o, p.d);
            // (per component, x * 0 is 0 or NaN: finite components whose sum would overflow stay finite rays)
            if (!(p.o.x * 0.0f + p.o.y * 0.0f + p.o.z * 0.0f + p.d.x * 0.0f + p.d.y * 0.0f + p.d.z * 0.0f == 0.0f)) {   // not traced (above)
                const float qnan = __uint_as_float(0x7FC00000u);
                res[i] = make_float4(qnan, qnan, qnan, INFINITY);
                res_id[i] = 0u;
                live = false;
            }
        }
        if (live) {
            if (R.rng) {
                const uint32_t* st = (const uint32_t*)(R.rng + i);
                p.g.s = __builtin_nontemporal_load(st); p.g.k = __builtin_nontemporal_load(st + 1);
            } else {
                p.g = path_rng(P.skey, R.stream0 + i, R.sample);
            }
            p.cur = f3(1.0f, 1.0f, 1.0f); p.depthf = 0.0f; p.first_id = 0u; p.seg = 0u; p.slot = i;
            float closest = P.tmax;
            int best;
            if (far_origin(S, p.o))
                best = traced_brute<false>(S, p.o, p.d, P.tmin, closest, w);
            else
                best = trace_traced<TR>(S, T, p.o, p.d, P.tmin, closest, w);
            if (MARCH) {                                             // trace<TR, true>'s march, once for both branches
                float tm;
                const int mg = march(S, p.o, p.d, P.tmin, P.tmax, closest, P.march_steps, tm, w);
                if (mg >= 0) { best = mg; closest = tm; }
            }
            keep = shade_path<MARCH, USER>(S, P, cap, p, closest, best, res, res_id);
            if (COUNT) segs++;
        }
        const uint64_t m = __ballot(keep);
        uint32_t obase = 0u, nc = 0u;
        if (lane == 0) {
            obase = m ? atomicAdd(&q_out, (uint32_t)__popcll(m)) : 0u;
            nc = atomicAdd(&q_next, 1u);
        }
        obase = __builtin_amdgcn_readfirstlane(obase);
        chunk = __builtin_amdgcn_readfirstlane(nc);
        const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (keep) store_path(out, seg0 + obase + rank, p);
    }
    __syncthreads();
    if (threadIdx.x == 0) count_out[blockIdx.x] = q_out;
    if (COUNT) {
        flush_counter(counters, OMC_SEGMENTS, segs);
        flush_counter(counters, OMC_PRIM_TESTS, w.prim);
        flush_counter(counters, OMC_PRE_TESTS, w.pre);
        flush_counter(counters, OMC_MARCH, w.march);
    }
}

// k_radiance: res[i], res_id[i] of a finished batch -> out[i] (om_radiance, 20 B).  A 20-B record
// is 16-B aligned only at every fourth index, so there is no vector store per record as
// store_query_hit has for its 32-B hits: each field is one non-temporal dword store, for any 4-B
// alignment of `out` (a wave's five stores cover 1280 contiguous bytes).
__global__ __launch_bounds__(256) void k_radiance(const float4* __restrict__ res, const uint32_t* __restrict__ res_id,
                                                  uint32_t n, om_radiance* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 r = ld4(res + i);
    const uint32_t id = __builtin_nontemporal_load(res_id + i);
    float* o = (float*)(out + i);
    __builtin_nontemporal_store(r.x, o); __builtin_nontemporal_store(r.y, o + 1); __builtin_nontemporal_store(r.z, o + 2);
    __builtin_nontemporal_store(r.w, o + 3);
    __builtin_nontemporal_store(__uint_as_float(id), o + 4);
}

// k_frame_paths: k_paths for a frame (om_render_rays*).  The batch is the rectangle F
// of the caller's sample-major ray table; path i of it is sample s_local = i / F.range of listed
// pixel kk = i % F.range, its result slot is i, which is where k_accumulate's fixed-list form reads
// sample s_local of list entry kk, and its ray is F.rays[s_local * F.ray_stride + kk].  A sample is
// taken by gen_path's serial rule on the live Stats (the previous batch's k_accumulate ran on this
// stream): Stats.n + s_local < spp_total and, in adaptive calls, not done.  One that is not taken
// stores kNoSample and loads neither ray nor state.  With F.rng null the path draws from
// path_rng(P.skey, pixel, Stats.n + s_local).  Staging, far origins, non-finite rays, the march of
// segment 0, compaction and counters are k_paths's.
template <int TR, bool COUNT, bool MARCH, bool USER>
__global__ __launch_bounds__(kBlk) OM_WAVES_ATTR void k_frame_paths(OmSceneDev S, OmParamsDev P, Seg G, FrameSrc F, Queue out,
                                                      uint32_t* __restrict__ count_out, float4* __restrict__ res,
                                                      uint32_t* __restrict__ res_id, unsigned long long* __restrict__ counters,
                                                      uint32_t* __restrict__ tail_next) {
    if (tail_next && blockIdx.x == 0 && threadIdx.x == 0) *tail_next = 0u;
    const uint64_t seg0 = (uint64_t)blockIdx.x * G.segcap;
    const uint32_t n = F.range * F.samples;                          // (at most 2^OM_WF_MAX_PATHS_LOG2)
    const Deal dl = batch_deal(n, G.nseg);
    const uint32_t chunks = dl.blocks_of(blockIdx.x);
    if (chunks == 0) {
        if (threadIdx.x == 0) count_out[blockIdx.x] = 0u;
        return;
    }
    __shared__ uint32_t q_next, q_out;
    if (threadIdx.x == 0) { q_next = kBlk / 64u; q_out = 0u; }
    __syncthreads();
    const Tracer T = stage_scene<TR>(S);
    const uint32_t cap = depth_cap(P);
    WorkT<COUNT, false, tr_bary(TR)> w;
    uint32_t segs = 0;
    const uint32_t lane = __lane_id();
    for (uint32_t chunk = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); chunk < chunks;) {   // wave-uniform
        const uint32_t i = (uint32_t)(dl.block(blockIdx.x, chunk) * 64u) + lane;
        bool keep = false;
        Path p;
        bool live = i < n;
        uint64_t at = 0;
        uint32_t pixel = 0, s = 0;
        if (live) {
            const uint32_t s_local = i / F.range, kk = i - s_local * F.range;
            pixel = F.pixels ? F.pixels[kk] : F.pixel0 + kk;
            const om_pixel_stats& ps = F.stats[pixel];
            s = ps.n + s_local;
            at = (uint64_t)s_local * F.ray_stride + kk;
            if (!(s < P.spp_total && !(P.adaptive && (ps.flags & 1u)))) {
                res_id[i] = kNoSample;
                live = false;
            }
        }
        if (live) {
            load_query_ray(F.rays, at, p.o, p.d);
            if (!(p.o.x * 0.0f + p.o.y * 0.0f + p.o.z * 0.0f + p.d.x * 0.0f + p.d.y * 0.0f + p.d.z * 0.0f == 0.0f)) {   // not traced (k_paths)
                const float qnan = __uint_as_float(0x7FC00000u);
                res[i] = make_float4(qnan, qnan, qnan, INFINITY);
                res_id[i] = 0u;
                live = false;
            }
        }
        if (live) {
            if (F.rng) {
                const uint32_t* st = (const uint32_t*)(F.rng + at);
                p.g.s = __builtin_nontemporal_load(st); p.g.k = __builtin_nontemporal_load(st + 1);
            } else {
                p.g = path_rng(P.skey, pixel, s);
            }
            p.cur = f3(1.0f, 1.0f, 1.0f); p.depthf = 0.0f; p.first_id = 0u; p.seg = 0u; p.slot = i;
            float closest = P.tmax;
            int best;
            if (far_origin(S, p.o))
                best = traced_brute<false>(S, p.o, p.d, P.tmin, closest, w);
            else
                best = trace_traced<TR>(S, T, p.o, p.d, P.tmin, closest, w);
            if (MARCH) {
                float tm;
                const int mg = march(S, p.o, p.d, P.tmin, P.tmax, closest, P.march_steps, tm, w);
                if (mg >= 0) { best = mg; closest = tm; }
            }
            keep = shade_path<MARCH, USER>(S, P, cap, p, closest, best, res, res_id);
            if (COUNT) segs++;
        }
        const uint64_t m = __ballot(keep);
        uint32_t obase = 0u, nc = 0u;
        if (lane == 0) {
            obase = m ? atomicAdd(&q_out, (uint32_t)__popcll(m)) : 0u;
            nc = atomicAdd(&q_next, 1u);
        }
        obase = __builtin_amdgcn_readfirstlane(obase);
        chunk = __builtin_amdgcn_readfirstlane(nc);
        const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (keep) store_path(out, seg0 + obase + rank, p);
    }
    __syncthreads();
    if (threadIdx.x == 0) count_out[blockIdx.x] = q_out;
    if (COUNT) {
        flush_counter(counters, OMC_SEGMENTS, segs);
        flush_counter(counters, OMC_PRIM_TESTS, w.prim);
        flush_counter(counters, OMC_PRE_TESTS, w.pre);
        flush_counter(counters, OMC_MARCH, w.march);
    }
}

// ---------------------------------------------------------------- accumulate
// Adaptive batches (ad.list): lane kk owns live-list entry kk, and a pixel that is still live after
// the batch, with samples of the call left, is appended to the stream's next list (one ballot and
// one atomic per workgroup: ThreadPixels::add_run / swap_buffers, render_thread.rs:68-102).  The list's
// order then depends on which wave appends first; a result's slot and a path's RNG never do.
template <bool COUNT>
__global__ __launch_bounds__(kBlk) void k_accumulate(OmParamsDev P, om_pixel_stats* __restrict__ stats,
                                                     const uint32_t* __restrict__ pixels, uint32_t n_pixels, uint32_t by_pixel,
                                                     uint32_t batch, const float4* __restrict__ res,
                                                     const uint32_t* __restrict__ res_id, const uint64_t* __restrict__ bloom,
                                                     AdList ad, unsigned long long* __restrict__ counters) {
    const uint32_t kk = blockIdx.x * kBlk + threadIdx.x;
    uint32_t n_samples = 0, credited = 0;
    uint32_t done0 = 0;
    if (ad.list) {
        const AdPlan pl = uniform_load(ad.plan);
        n_pixels = pl.c;
        batch = ad_batch(pl.c, pl.done, ad.j, ad.A);
        done0 = pl.done;
        if (kk == 0) ad.plan_next->done = pl.done + batch;
    }
    bool relist = false;
    uint32_t k = kk;
    if (kk < n_pixels) {
        if (ad.list) k = ad.list[kk];
        const uint32_t slot = by_pixel ? pixels[k] : k;
        const om_pixel_stats in = stats[slot];
        PixelState st;
        st.bloom = in.bloom; st.sx = in.sum[0]; st.sy = in.sum[1]; st.sz = in.sum[2]; st.n = in.n;
        st.avg_depth = in.avg_depth; st.bad = in.bad_avgs;
        st.rgbf = (uint32_t)in.color[0] | ((uint32_t)in.color[1] << 8) | ((uint32_t)in.color[2] << 16) | ((uint32_t)in.flags << 24);
        // the loads of OM_ACC_GROUP samples are issued together (ids, then results and bloom
        // words), then added in sample order: one lane's samples no longer cost a chain of
        // dependent global round trips each (r03: 0.2-0.85 ms per 1080p x 16-spp launch before)
        bool retired = P.adaptive && (st.rgbf & 0x01000000u);          // retired before the batch: no loads
        for (uint32_t s0 = 0; s0 < batch && !retired; s0 += OM_ACC_GROUP) {
            const uint32_t m = batch - s0 < OM_ACC_GROUP ? batch - s0 : OM_ACC_GROUP;
            uint32_t id[OM_ACC_GROUP];
            float4 rr[OM_ACC_GROUP];
            uint64_t bl[OM_ACC_GROUP];
#pragma unroll
            for (uint32_t j = 0; j < OM_ACC_GROUP; ++j) id[j] = j < m ? res_id[(uint64_t)(s0 + j) * n_pixels + kk] : kNoSample;
#pragma unroll
            for (uint32_t j = 0; j < OM_ACC_GROUP; ++j) {
                if (j < m) rr[j] = res[(uint64_t)(s0 + j) * n_pixels + kk];
                bl[j] = bloom[id[j] == kNoSample ? 0u : id[j]];
            }
#pragma unroll
            for (uint32_t j = 0; j < OM_ACC_GROUP; ++j) {                  // sample order == reference order
                if (j >= m) break;
                // adaptive batches of several samples: a pixel that retires at sample j takes no more
                // (ThreadPixels::add_run, render_thread.rs:68-102); the batch's later samples of it
                // were rendered speculatively and are dropped here
                if (P.adaptive && (st.rgbf & 0x01000000u)) { retired = true; break; }
                if (id[j] == kNoSample) continue;
                const bool done = stats_add(st, f3(rr[j].x, rr[j].y, rr[j].z), rr[j].w, bl[j]);
                if (COUNT) n_samples++;
                credited += ((done && P.adaptive) ? (P.spp_total - st.n) : 0u) + 1u;   // render_thread.rs:196-198
            }
        }
        om_pixel_stats out;
        out.bloom = st.bloom; out.sum[0] = st.sx; out.sum[1] = st.sy; out.sum[2] = st.sz; out.n = st.n;
        out.avg_depth = st.avg_depth; out.bad_avgs = st.bad;
        out.color[0] = (uint8_t)(st.rgbf & 0xFFu); out.color[1] = (uint8_t)((st.rgbf >> 8) & 0xFFu);
        out.color[2] = (uint8_t)((st.rgbf >> 16) & 0xFFu); out.flags = (uint8_t)(st.rgbf >> 24); out.reserved = 0u;
        stats[slot] = out;
        relist = ad.list && !(st.rgbf & 0x01000000u) && st.n < P.spp_total && done0 + batch < ad.A.sample_count;
    }
    if (ad.list) {                                                  // the stream's next live list
        const uint64_t m = __ballot(relist);
        uint32_t base = 0u;
        // one global atomic per workgroup (the waves' counts summed in LDS first): the ~16k
        // contended atomics on one word of a 1M-pixel accumulate become ~2k (r06: C1_adaptive
        // +3.8%, profiles/r06_adaptive)
        __shared__ uint32_t wg_n, wg_base;
        if (threadIdx.x == 0) wg_n = 0u;
        __syncthreads();
        if (__lane_id() == 0 && m) base = atomicAdd(&wg_n, (uint32_t)__popcll(m));
        __syncthreads();
        if (threadIdx.x == 0) wg_base = wg_n ? atomicAdd(&ad.plan_next->c, wg_n) : 0u;
        __syncthreads();
        base = __builtin_amdgcn_readfirstlane(base) + wg_base;
        if (relist) ad.list_next[base + (uint32_t)__popcll(m & ((1ull << __lane_id()) - 1ull))] = k;
    }
    if (COUNT) {
        flush_counter(counters, OMC_SAMPLES, n_samples);
        flush_counter(counters, OMC_CREDITED, credited);
    }
    if (P.progress) {                                               // live samples_atom (om_progress)
        // summed per workgroup first: one contended atomic per workgroup, not per wave
        __shared__ unsigned long long wg_credit;
        if (threadIdx.x == 0) wg_credit = 0ull;
        __syncthreads();
        const uint32_t v = wave_sum32(credited);
        if (__lane_id() == 0 && v) atomicAdd(&wg_credit, (unsigned long long)v);
        __syncthreads();
        if (threadIdx.x == 0 && wg_credit) atomicAdd(&counters[OMC_PROGRESS], wg_credit);
    }
}

// k_snapshot: n0[k] = Stats.n of listed pixel k at the start of a concurrent fixed-spp call.
__global__ __launch_bounds__(256) void k_snapshot(const om_pixel_stats* __restrict__ stats, const uint32_t* __restrict__ pixels,
                                                  uint32_t n_pixels, uint32_t by_pixel, uint32_t* __restrict__ n0) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n_pixels) return;
    n0[k] = stats[by_pixel ? pixels[k] : k].n;
}

// k_ad_init: the first live list of every stream of an adaptive call.  Chunk q of 64 list entries
// (a tile of a frame list) belongs to stream q % ns; its pixels that are not retired and have
// samples left are appended to that stream's list (one ballot per wave, one atomic per workgroup and stream: a wave is one
// chunk).  plans (zeroed by the caller) get the counts.
constexpr uint32_t kAdInitBlk = 1024u;
__global__ __launch_bounds__(kAdInitBlk) void k_ad_init(const om_pixel_stats* __restrict__ stats, const uint32_t* __restrict__ pixels,
                                                 uint32_t n_pixels, uint32_t by_pixel, uint32_t spp_total, uint32_t ns,
                                                 uint32_t* __restrict__ lists, uint64_t list_stride, AdPlan* __restrict__ plans,
                                                 uint32_t plan_stride) {
    const uint32_t k = blockIdx.x * kAdInitBlk + threadIdx.x;
    bool live = false;
    if (k < n_pixels) {
        const om_pixel_stats& ps = stats[by_pixel ? pixels[k] : k];
        live = !(ps.flags & 1u) && ps.n < spp_total;
    }
    const uint32_t s = (k >> 6) % ns;                                // wave-uniform
    const uint64_t m = __ballot(live);
    uint32_t base = 0u;
    // per stream, one global atomic per workgroup (the waves' counts summed in LDS first)
    __shared__ uint32_t wg_n[4], wg_base[4];
    if (threadIdx.x < 4u) wg_n[threadIdx.x] = 0u;
    __syncthreads();
    if (__lane_id() == 0 && m) base = atomicAdd(&wg_n[s], (uint32_t)__popcll(m));
    __syncthreads();
    if (threadIdx.x < ns && wg_n[threadIdx.x])
        wg_base[threadIdx.x] = atomicAdd(&plans[(uint64_t)threadIdx.x * plan_stride].c, wg_n[threadIdx.x]);
    __syncthreads();
    base = __builtin_amdgcn_readfirstlane(base) + (m ? wg_base[s] : 0u);
    if (live) lists[s * list_stride + base + (uint32_t)__popcll(m & ((1ull << __lane_id()) - 1ull))] = k;
}

hipError_t grow(Buffers& B, uint64_t cap, uint32_t counts_n, int nsets) {
    hipError_t e;
    if (cap > B.cap || nsets > B.nsets) {
        for (auto& s : B.set) s.release();
        B.cap = 0; B.nsets = 0; B.counts_n = 0;
        for (int k = 0; k < nsets; ++k) {
            QueueSet& S = B.set[k];
            for (int a = 0; a < 2; ++a) {
                for (int b = 0; b < 3; ++b) if ((e = hipMalloc(&S.q[a][b], cap * sizeof(float4))) != hipSuccess) return e;
                if ((e = hipMalloc(&S.qr[a], cap * sizeof(uint4))) != hipSuccess) return e;
            }
            if ((e = hipMalloc(&S.res, cap * sizeof(float4))) != hipSuccess) return e;
            if ((e = hipMalloc(&S.res_id, cap * sizeof(uint32_t))) != hipSuccess) return e;
            if ((e = hipMalloc(&S.hit, cap * sizeof(float2))) != hipSuccess) return e;
        }
        B.cap = cap; B.nsets = nsets;
    }
    if (counts_n > B.counts_n) {
        for (int k = 0; k < B.nsets; ++k) {
            QueueSet& S = B.set[k];
            if (S.counts) (void)hipFree(S.counts);
            S.counts = nullptr;
            if ((e = hipMalloc(&S.counts, (size_t)counts_n * sizeof(uint32_t))) != hipSuccess) return e;
        }
        B.counts_n = counts_n;
    }
    return hipSuccess;
}

Queue queue(QueueSet& B, int k) { return Queue{B.q[k][0], B.q[k][1], B.q[k][2], B.qr[k]}; }

// k_tail's dynamic LDS: the segment-count prefix (nseg + 1 words) behind stage_scene's bytes
inline uint32_t tail_pre_off(uint32_t lds) { return (lds + 15u) & ~15u; }
inline uint32_t tail_lds(uint32_t lds, uint32_t nseg) { return tail_pre_off(lds) + (nseg + 1u) * 4u; }

// Rows of nseg segment counts a queue set holds: one per bounce and the counts behind the last one;
// the fused first launch writes row 2 whatever the depth.
inline uint32_t count_rows(uint32_t depth_cap) { return std::max<uint32_t>(depth_cap, kFuseB1 ? 2u : 1u) + 1u; }

// One batch: bounce 0 .. tail_at-1 as per-bounce launches, then the tail launch, all on `st`;
// returns the number of bounce-family launches.
// EXACT (marched worlds, where exact_view_built<TR>()): the marched set has C2's shape and no user
// object (OmMSdf), so the march kernels take MarchedC2Lds and the shade leaves the SDF programs out.
// X (ray_color batches): segment 0 is k_paths over the caller's rays instead of the camera's launch
// (k_raygen and bounce 0's k_march pair, or k_bounce<FIRST> with its fused bounce 1); its out queue
// is bounce 1's, and everything from there on is the render's.  R is then unused by the kernels.
// F (render_rays batches): the same with k_frame_paths over the batch's rectangle of the frame's rays.
template <int TR, bool COUNT, bool MARCH, bool EXACT>
uint32_t run_batch(QueueSet& B, const Launch& L, hipStream_t st, Seg G, const Gen& R, uint32_t tail_at, uint32_t lds,
                   uint32_t tail_grid, const RaySrc* X = nullptr, const FrameSrc* F = nullptr) {
    const bool ext = X || F;                                     // segment 0 from the caller's rays
    constexpr int VIEW = EXACT && exact_view_built<TR>() ? MV_EXACT_C2_LDS : MV_ARRAYS;
    Timer& tm = *L.timer;
    const bool each = tm.mode == 1;
    uint32_t launches = 0;
    const uint32_t cap = depth_cap(L.P);
    // the traced tail's claim counter: the word behind the set's per-bounce counts
    uint32_t* const tail_next = B.counts + (size_t)count_rows(cap) * G.nseg;
    auto tail = [&](const Queue& in, const uint32_t* cin) {
        const int ti = each ? tm.begin(st) : -1;
        if constexpr (MARCH) {
            const uint32_t grid = (G.nseg + kTailSpb - 1u) / kTailSpb;
            hipLaunchKernelGGL((k_tail_march<TR, COUNT, VIEW>), dim3(grid), dim3(kBlk), lds, st, L.S, L.P, G, in, cin,
                               B.res, B.res_id, L.counters);
        } else {
            hipLaunchKernelGGL((k_tail<TR, COUNT>), dim3(tail_grid), dim3(kBlk), tail_lds(lds, G.nseg), st, L.S, L.P, G, in, cin,
                               tail_pre_off(lds), tail_next, B.res, B.res_id, L.counters);
        }
        tm.end(ti, OM_KT_TAIL, st);
        return launches + 1u;
    };
    if constexpr (MARCH) {
        // split march pipeline: k_raygen compacts the camera paths into queue 0;
        // per bounce, the lane-refilling k_march writes every path's (closest, winner) to the hit
        // buffer and k_bounce<HIT> shades and compacts
        {
            const int ti = each ? tm.begin(st) : -1;
            if (F)
                hipLaunchKernelGGL((k_frame_paths<TR, COUNT, true, !EXACT>), dim3(G.nseg), dim3(kBlk), lds, st, L.S, L.P, G, *F, queue(B, 1),
                                   B.counts + G.nseg, B.res, B.res_id, L.counters, (uint32_t*)nullptr);
            else if (X)
                hipLaunchKernelGGL((k_paths<TR, COUNT, true, !EXACT>), dim3(G.nseg), dim3(kBlk), lds, st, L.S, L.P, G, *X, queue(B, 1),
                                   B.counts + G.nseg, B.res, B.res_id, L.counters, (uint32_t*)nullptr);
            else
                hipLaunchKernelGGL((k_raygen<COUNT>), dim3(G.nseg), dim3(kBlk), 0, st, L.P, G, R, queue(B, 0), B.counts, B.res_id);
            tm.end(ti, OM_KT_BOUNCE0, st);
            ++launches;
        }
        for (uint32_t bounce = ext ? 1u : 0u; bounce < cap; ++bounce) {
            const Queue in = queue(B, bounce & 1u), out = queue(B, (bounce + 1u) & 1u);
            const uint32_t* cin = B.counts + (size_t)bounce * G.nseg;
            if (bounce >= tail_at) return tail(in, cin);   // (tail_at 0: k_raygen's camera paths too)
            uint32_t* cout = B.counts + (size_t)(bounce + 1u) * G.nseg;
            const int kc = bounce == 0 ? OM_KT_BOUNCE0 : OM_KT_BOUNCE;
            int ti = each ? tm.begin(st) : -1;
            hipLaunchKernelGGL((k_march<TR, COUNT, VIEW>), dim3(G.nseg), dim3(kBlk), lds, st, L.S, L.P, G, in, cin, B.hit,
                               L.counters);
            tm.end(ti, kc, st);
            ti = each ? tm.begin(st) : -1;
            hipLaunchKernelGGL((k_bounce<TR, COUNT, MARCH, false, true, !EXACT>), dim3(G.nseg), dim3(kBlk), 0, st, L.S, L.P, G, R,
                               in, cin, out, cout, B.res, B.res_id, L.counters, (const float2*)B.hit, (uint32_t*)nullptr);
            tm.end(ti, kc, st);
            launches += 2u;
        }
        return launches;
    } else {
    // (fused first launch: bounces 0 and 1, its out queue is bounce 2's; the first queue the tail or a
    // per-bounce launch can read is the one that launch wrote, whatever tail_at asks for)
    for (uint32_t bounce = 0, next; bounce < cap; bounce = next) {
        next = bounce + (bounce == 0 && kFuseB1 && !ext ? 2u : 1u);
        const Queue in = queue(B, bounce & 1u), out = queue(B, next & 1u);
        const uint32_t* cin = B.counts + (size_t)bounce * G.nseg;
        if (bounce > 0 && bounce >= tail_at) return tail(in, cin);
        uint32_t* cout = B.counts + (size_t)next * G.nseg;
        const int ti = each ? tm.begin(st) : -1;
        if (bounce == 0 && F)
            hipLaunchKernelGGL((k_frame_paths<TR, COUNT, false, false>), dim3(G.nseg), dim3(kBlk), lds, st, L.S, L.P, G, *F, out, cout,
                               B.res, B.res_id, L.counters, tail_next);
        else if (bounce == 0 && X)
            hipLaunchKernelGGL((k_paths<TR, COUNT, false, false>), dim3(G.nseg), dim3(kBlk), lds, st, L.S, L.P, G, *X, out, cout,
                               B.res, B.res_id, L.counters, tail_next);
        else if (bounce == 0)
            hipLaunchKernelGGL((k_bounce<TR, COUNT, MARCH, true>), dim3(G.nseg), dim3(kBlk), lds, st, L.S, L.P, G, R, in,
                               cin, out, cout, B.res, B.res_id, L.counters, (const float2*)nullptr, tail_next);
        else
            hipLaunchKernelGGL((k_bounce<TR, COUNT, MARCH, false>), dim3(G.nseg), dim3(kBlk), lds, st, L.S, L.P, G, R, in,
                               cin, out, cout, B.res, B.res_id, L.counters, (const float2*)nullptr, (uint32_t*)nullptr);
        tm.end(ti, bounce == 0 ? OM_KT_BOUNCE0 : OM_KT_BOUNCE, st);
        ++launches;
    }
    return launches;
    }
}

hipError_t ensure_events(Buffers& B, size_t n) {
    while (B.ev.size() < n) {
        hipEvent_t e = nullptr;
        const hipError_t r = hipEventCreateWithFlags(&e, hipEventDisableTiming);
        if (r != hipSuccess) return r;
        B.ev.push_back(e);
    }
    return hipSuccess;
}

// The closest-hit variant (TR_*) of a ctx's kernel choice (Launch::trace_mode) for the uploaded
// world: renders and ray queries share it.
int pick_trace(int trace_mode, const OmSceneDev& S) {
    int tr = trace_mode == TR_SBVH_LDS ? TR_SBVH_GLOBAL : trace_mode;
    // OM_KERNEL_BVH2W: the wide variant for any world that has the wide nodes; an empty tree takes
    // OM_KERNEL_BVH2's fallbacks below
    if (tr == TR_BVH2_WIDE) {
        if (S.n_b2wnodes) return TR_BVH2_WIDE | TR_BARY;
        tr = TR_BVH2_LDS;
    }
    if (tr == TR_BVH4_LDS) tr = S.n_b4nodes == 0 ? TR_BVH2_LDS : (S.b4_lds_bytes ? TR_BVH4_LDS : TR_BVH4_GLOBAL);
    // an empty BVH2 (no bounded sphere/cube: marched-only worlds, C2) takes the reference loop
    // when the old BVH holds at most one leaf: TR_BVH's 64-entry stack lives in scratch memory,
    // which every k_march / k_tail wave would then carry for nothing (C2: 1785 vs 1649, r02_v8)
    // a tree past the 15-bit codes (n_b2nodes == 0) with the wide nodes usable: the same traversal
    // over 32-bit codes instead of TR_BVH; BVH4 requests arrive here too
    if (tr == TR_BVH2_LDS && S.n_b2nodes == 0 && S.n_b2wnodes) return TR_BVH2_WIDE | TR_BARY;
    if (tr == TR_BVH2_LDS)
        tr = S.n_b2nodes == 0 ? (S.n_bvh_nodes <= 1u ? TR_BRUTE : TR_BVH) : (S.b2_lds_bytes ? TR_BVH2_LDS : TR_BVH2_GLOBAL);
    // triangles / parallelograms in the leaves: the tree variants' TR_BARY instantiations
    const int bary = S.n_srec_bary ? TR_BARY : 0;
    switch (tr) {
        case TR_BRUTE: case TR_CULLED: case TR_BVH: return tr;
        case TR_SBVH_GLOBAL: case TR_BVH2_LDS: case TR_BVH4_LDS: case TR_BVH4_GLOBAL: return tr | bary;
        default: return TR_BVH2_GLOBAL | bary;
    }
}
// dynamic LDS bytes of a workgroup that stages variant `tr` (stage_scene's [stack][nodes][leaf table])
uint32_t trace_lds(int trf, const OmSceneDev& S) {
    const int tr = tr_base(trf);
    return tr == TR_BVH2_LDS ? stack_bytes<TR_BVH2_LDS>(S) + b2_stage_bytes(S)
         : tr == TR_BVH2_GLOBAL ? stack_bytes<TR_BVH2_GLOBAL>(S) + hyb_nodes(S) * (uint32_t)sizeof(OmBvh2NodeH)
         : tr == TR_BVH4_LDS ? stack_bytes<TR_BVH4_LDS>(S) + S.b4_lds_bytes
         : tr == TR_BVH4_GLOBAL ? stack_bytes<TR_BVH4_GLOBAL>(S) + hyb4_nodes(S) * (uint32_t)sizeof(OmBvh4NodeH)
         : tr == TR_BVH2_WIDE ? stack_bytes<TR_BVH2_WIDE>(S) + hybw_nodes(S) * (uint32_t)sizeof(OmBvh2NodeW)
         : 0u;
}
// f(std::integral_constant<int, TR>) for a variant pick_trace returned
template <class F>
void with_tr(int tr, F f) {
    switch (tr) {
        case TR_BRUTE: f(std::integral_constant<int, TR_BRUTE>{}); break;
        case TR_CULLED: f(std::integral_constant<int, TR_CULLED>{}); break;
        case TR_BVH: f(std::integral_constant<int, TR_BVH>{}); break;
        case TR_SBVH_GLOBAL: f(std::integral_constant<int, TR_SBVH_GLOBAL>{}); break;
        case TR_BVH2_LDS: f(std::integral_constant<int, TR_BVH2_LDS>{}); break;
        case TR_BVH4_LDS: f(std::integral_constant<int, TR_BVH4_LDS>{}); break;
        case TR_BVH4_GLOBAL: f(std::integral_constant<int, TR_BVH4_GLOBAL>{}); break;
        case TR_SBVH_GLOBAL | TR_BARY: f(std::integral_constant<int, TR_SBVH_GLOBAL | TR_BARY>{}); break;
        case TR_BVH2_LDS | TR_BARY: f(std::integral_constant<int, TR_BVH2_LDS | TR_BARY>{}); break;
        case TR_BVH2_GLOBAL | TR_BARY: f(std::integral_constant<int, TR_BVH2_GLOBAL | TR_BARY>{}); break;
        case TR_BVH4_LDS | TR_BARY: f(std::integral_constant<int, TR_BVH4_LDS | TR_BARY>{}); break;
        case TR_BVH4_GLOBAL | TR_BARY: f(std::integral_constant<int, TR_BVH4_GLOBAL | TR_BARY>{}); break;
        case TR_BVH2_WIDE | TR_BARY: f(std::integral_constant<int, TR_BVH2_WIDE | TR_BARY>{}); break;
        default: f(std::integral_constant<int, TR_BVH2_GLOBAL>{}); break;
    }
}

// the current device's CU count and its LDS limit per workgroup
struct DeviceLimits { int cus = 256, lds_max = 0; };
DeviceLimits device_limits() {
    DeviceLimits d;
    int dev = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&d.cus, hipDeviceAttributeMultiprocessorCount, dev);
    (void)hipDeviceGetAttribute(&d.lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
    return d;
}

}  // namespace

// Schedules:
//   fixed spp, serial      (L.streams == 1) one batch after another on `st`.
//   fixed spp, concurrent  (default) the call's samples split into batches of at most half the
//               call, dealt round-robin to L.streams streams (`st` + side streams), each with its
//               own queue set: two batches are in flight at once, so one batch's latency-bound
//               phases (the drain of every launch, the late bounces, the tail) run beside the
//               other's full ones.  Sample indices come from the call-start Stats.n snapshot (n0).
//   adaptive    the listed pixels are dealt to the streams by 64-entry chunks; each stream runs
//               up to ad_batches batches over ITS live pixels, from a live list its own
//               k_accumulate compacts, with the batch's sample count planned on the device from
//               the live count (ad_batch): nothing is rendered for a retired pixel, and samples
//               past a retirement inside a batch are dropped in sample order by k_accumulate.
// In both concurrent forms the accumulates run in batch order through events (acc i after
// acc i-1) and the call ends joined on `st`.
// Timing: mode 2 brackets the call once on `st` (OM_KT_BOUNCE_SPAN, with the call's
// bounce-family launch count); mode 1 brackets every launch on its stream and the call.
hipError_t render(Buffers& B, const Launch& L, hipStream_t st, std::string& err) {
    const uint32_t n_px = L.n_pixels;
    if (n_px == 0 || L.P.sample_count == 0) return hipSuccess;
    const bool adaptive = L.P.adaptive != 0u;
    const uint32_t want = std::max<uint32_t>(1u, std::min<uint32_t>(L.streams, (uint32_t)kMaxSets));
    // fixed spp: paths per batch 2^25 (33.5M, ~4.9 GB of queues per set; 16 spp of 1080p, the
    // measured sweet spot, §5.5), raised up to 16 spp of the frame for frames above 2M pixels,
    // within 2^27 (~21 GB per set, two sets; MI355X has 288 GB): a 4K frame (C4, 8.3M pixels) then
    // runs 16-spp batches like 1080p instead of 4-spp ones, whose 4x launches and 4x Stats
    // read-modify-write per sample cost C4 ~11% in k_accumulate alone (r03)
    const uint64_t kMaxPaths = std::min<uint64_t>(1ull << OM_WF_MAX_PATHS_LOG2,
                                                  std::max<uint64_t>(1ull << OM_WF_MIN_PATHS_LOG2, (uint64_t)OM_WF_BATCH_SPP * n_px));
    uint32_t ns, nb, batch = 0, ad_k = 0, cmax = 0;
    uint64_t max_paths;
    std::vector<uint32_t> done_at(1, 0u);                          // fixed spp: samples of the call before batch i
    AdCfg A{};
    if (adaptive) {
        const uint32_t chunks = (n_px + 63u) / 64u;
        ns = std::min<uint32_t>(want, chunks);
        cmax = std::min<uint32_t>(n_px, (chunks + ns - 1u) / ns * 64u);   // entries of the fullest stream
        // batches per stream: OM_WF_ADAPTIVE_BATCHES, more when the forced even share of a large
        // call would exceed 2^OM_WF_ADAPTIVE_CAP_LOG2 paths
        const uint64_t capmax = 1ull << OM_WF_ADAPTIVE_CAP_LOG2;
        uint64_t k = L.ad_batches ? L.ad_batches : OM_WF_ADAPTIVE_BATCHES;
        while (k < L.P.sample_count && (uint64_t)cmax * ((L.P.sample_count + k - 1u) / k) > capmax) ++k;
        ad_k = (uint32_t)std::min<uint64_t>(k, L.P.sample_count);
        A.sample_count = L.P.sample_count; A.batches = ad_k;
        A.paths = 1u << (L.ad_paths_log2 ? L.ad_paths_log2 : OM_WF_ADAPTIVE_PATHS_LOG2);
        max_paths = std::max<uint64_t>(std::min<uint64_t>(A.paths, (uint64_t)cmax * L.P.sample_count),
                                       (uint64_t)cmax * ((L.P.sample_count + ad_k - 1u) / ad_k));
        nb = ad_k * ns;
    } else {
        const bool concurrent = want >= 2u && L.P.sample_count >= 2u;
        batch = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(L.P.sample_count, kMaxPaths / n_px));
        // at most 1/want of the call per batch, so every call has batches in flight together
        if (concurrent) batch = std::min<uint32_t>(batch, (L.P.sample_count + want - 1u) / want);
        while (done_at.back() < L.P.sample_count)
            done_at.push_back(done_at.back() + std::min(batch, L.P.sample_count - done_at.back()));
        nb = (uint32_t)done_at.size() - 1u;
        ns = concurrent ? std::min<uint32_t>(want, nb) : 1u;
        max_paths = (uint64_t)n_px * batch;
    }
    const uint32_t cap = depth_cap(L.P);
    const DeviceLimits dev = device_limits();
    const int tr = pick_trace(L.trace_mode, L.S);
    // segments, a multiple of the tail grouping: 4096 lanes per CU (8 workgroups of 512) for
    // traced worlds whose BVH2 sits in LDS, 8192 for marched worlds and L2-resident trees
    const bool march = has_marched(L.S);
    // the marched set of C2's shape, no user objects (run_batch's EXACT)
    const bool exact = march && L.S.n_msdf == 0u && MarchedC2Lds::matches(L.S.n_msph, L.S.n_mbox, L.S.n_mtor);
    // trees read through L2 (the wide BVH2 among them)
    const bool l2_tree = tr_base(tr) == TR_BVH2_GLOBAL || tr_base(tr) == TR_BVH4_GLOBAL || tr_base(tr) == TR_BVH2_WIDE;
    // the first bounce of the tail: the caller's (om_set_tail_bounce), or the default count of
    // per-bounce launches, which the fused first launch carries one bounce further
    const uint32_t tail_at = L.tail_bounce ? L.tail_bounce
                           : march ? kTailMarched
                           : (l2_tree ? kTailL2 : adaptive ? OM_WF_ADAPTIVE_TAIL
                              : max_paths > (1ull << 25) ? kTailBigBatch : kTailDefault) + (kFuseB1 ? 1u : 0u);
    const uint32_t lanes_per_cu = (march || l2_tree) ? OM_WF_LANES_PER_CU_WIDE : OM_WF_LANES_PER_CU;
    const uint32_t nseg = deal_segments(max_paths, (uint32_t)dev.cus, lanes_per_cu, kBlk, kTailSpb);
    // the fullest workgroup's share of the largest batch's deal (adaptive: max_paths bounds every
    // batch the device plans, and capacity() grows with the paths)
    const uint32_t segcap = batch_deal(max_paths, nseg).capacity();
    // (+ 1: the traced tail's claim counter, run_batch)
    hipError_t e = grow(B, (uint64_t)nseg * segcap, count_rows(cap) * nseg + 1u, (int)ns);
    if (e != hipSuccess) { err = "wavefront buffer allocation failed"; return e; }
    const uint32_t lds = trace_lds(tr, L.S);
    // the traced tail: a resident grid, and the segment-count prefix in LDS behind the tree
    const uint32_t tail_grid = (uint32_t)dev.cus * kTailWgsPerCu;
    if (!march && tail_at < cap && tail_lds(lds, nseg) > (uint32_t)dev.lds_max) {
        err = "the tail's LDS request exceeds the device's limit";
        return hipErrorInvalidValue;
    }
    // every other launch of the variant requests `lds` (a wide tree at the 32-entry bound: 64 KiB of stack)
    if (lds > (uint32_t)dev.lds_max) {
        err = "the traversal's LDS request exceeds the device's limit";
        return hipErrorInvalidValue;
    }
    Gen R;
    R.C = L.C; R.jitter = L.jitter; R.stats = L.stats; R.pixels = L.pixels; R.n_pixels = n_px;
    R.by_pixel = L.stats_by_pixel ? 1u : 0u;
    R.tile_off = L.tile_off; R.tile_idx = L.tile_idx; R.tile_tnear = L.tile_tnear;
    R.n0 = nullptr; R.done = 0; R.ad = AdList{};
    hipStream_t streams[kMaxSets] = {st, st, st, st};
    Timer& tm = *L.timer;
    const int call_ti = tm.begin(st);
    // device words: fixed spp, the call-start Stats.n snapshot (n0, concurrent calls); adaptive, per
    // stream two live lists (ping-pong) of cmax entries and ad_k + 1 plans
    const uint32_t plan_stride = ad_k + 1u;
    const uint64_t words = adaptive ? (uint64_t)ns * 2u * cmax + (uint64_t)ns * plan_stride * 2u : (ns > 1 ? n_px : 0u);
    if (words > B.n0_cap) {
        if (B.n0) (void)hipFree(B.n0);
        B.n0 = nullptr; B.n0_cap = 0;
        if ((e = hipMalloc(&B.n0, (size_t)words * sizeof(uint32_t))) != hipSuccess) { err = "n0 allocation failed"; return e; }
        B.n0_cap = words;
    }
    uint32_t* lists = B.n0;
    AdPlan* plans = adaptive ? (AdPlan*)(B.n0 + (uint64_t)ns * 2u * cmax) : nullptr;
    if (adaptive) {
        (void)hipMemsetAsync(plans, 0, (size_t)ns * plan_stride * sizeof(AdPlan), st);
        hipLaunchKernelGGL(k_ad_init, dim3((n_px + kAdInitBlk - 1u) / kAdInitBlk), dim3(kAdInitBlk), 0, st, L.stats, L.pixels, n_px, R.by_pixel,
                           L.P.spp_total, ns, lists, (uint64_t)2u * cmax, plans, plan_stride);
    } else if (ns > 1) {
        hipLaunchKernelGGL(k_snapshot, dim3((n_px + 255u) / 256u), dim3(256), 0, st, L.stats, L.pixels, n_px, R.by_pixel, B.n0);
        R.n0 = B.n0;
    }
    // events: [0] call start on `st`, [k] side stream k joined, [kMaxSets + i] batch i accumulated
    if (ns > 1) {
        if ((e = ensure_events(B, kMaxSets + nb)) != hipSuccess) { err = "event creation failed"; return e; }
        (void)hipEventRecord(B.ev[0], st);                       // side streams start after everything before the call
        for (uint32_t k = 1; k < ns; ++k) {
            if (!B.side[k] && (e = hipStreamCreateWithFlags(&B.side[k], hipStreamNonBlocking)) != hipSuccess) {
                err = "side stream creation failed"; return e;
            }
            streams[k] = B.side[k];
            (void)hipStreamWaitEvent(streams[k], B.ev[0], 0);
        }
    }
    uint32_t launches = 0;
    for (uint32_t i = 0; i < nb; ++i) {
        const uint32_t sidx = i % ns;                             // stream (and queue set) of batch i
        hipStream_t si = streams[sidx];
        QueueSet& QS = B.set[sidx];
        Seg G;
        G.nseg = nseg;
        uint32_t b = 0, grid_a;
        AdList ad{};
        if (adaptive) {
            // batch j of stream sidx: its live list and plan, the next ones written by its accumulate
            const uint32_t j = i / ns;
            uint32_t* lbase = lists + (uint64_t)sidx * 2u * cmax;
            ad.list = lbase + (uint64_t)(j & 1u) * cmax;
            ad.list_next = lbase + (uint64_t)((j + 1u) & 1u) * cmax;
            ad.plan = plans + (uint64_t)sidx * plan_stride + j;
            ad.plan_next = plans + (uint64_t)sidx * plan_stride + j + 1u;
            ad.A = A; ad.j = j;
            G.segcap = segcap;                                    // queue capacity of the largest batch
            grid_a = (cmax + kBlk - 1) / kBlk;
        } else {
            const uint32_t done = done_at[i];
            b = done_at[i + 1] - done;
            G.segcap = batch_deal((uint64_t)n_px * b, nseg).capacity();
            R.done = done;
            grid_a = (n_px + kBlk - 1) / kBlk;
        }
        R.batch = b;
        R.ad = ad;
        with_tr(tr, [&](auto t) {
            constexpr int TR = decltype(t)::value;
            with_flags({L.count, march, exact && exact_view_built<TR>()}, [&](auto count, auto mar, auto ex) {
                if constexpr (mar || !ex) launches += run_batch<TR, count, mar, ex>(QS, L, si, G, R, tail_at, lds, tail_grid);
            });
        });
        // accumulates in batch order: fixed spp needs it (Stats::add in sample order); an adaptive
        // stream's pixels are its own, so there it only keeps the streams in step and the progress
        // copies in order (unchained streams measured the same: 49.3 vs 49.2 ms per frame, r05_p6)
        if (ns > 1 && i > 0) (void)hipStreamWaitEvent(si, B.ev[kMaxSets + i - 1u], 0);
        const int ati = tm.mode == 1 ? tm.begin(si) : -1;
        with_flags({L.count}, [&](auto count) {
            hipLaunchKernelGGL(k_accumulate<count>, dim3(grid_a), dim3(kBlk), 0, si, L.P, L.stats, L.pixels, n_px,
                               L.stats_by_pixel ? 1u : 0u, b, QS.res, QS.res_id, L.S.bloom, ad, L.counters);
        });
        tm.end(ati, OM_KT_ACCUMULATE, si);
        // live progress: the cumulative credit after this batch, to the host word om_progress
        // hands out; ahead of the event the next batch's accumulate waits on, so the copies
        // land in order and the word only grows
        if (L.progress_host)
            (void)hipMemcpyAsync(L.progress_host, L.counters + OMC_PROGRESS, sizeof(unsigned long long),
                                 hipMemcpyDeviceToHost, si);
        if (ns > 1) (void)hipEventRecord(B.ev[kMaxSets + i], si);
        if ((e = hipGetLastError()) != hipSuccess) { err = "wavefront launch failed"; return e; }
    }
    for (uint32_t k = 1; k < ns; ++k) {
        (void)hipEventRecord(B.ev[k], streams[k]);
        (void)hipStreamWaitEvent(st, B.ev[k], 0);
    }
    tm.end(call_ti, OM_KT_BOUNCE_SPAN, st, launches);
    return hipSuccess;
}

// ray_color for Q.n caller-given rays (om_ray_color*): batches of at most
// 2^paths_log2 paths, one after another on `st` through queue set 0 of the ctx (the set renders on
// `st` use, so a query and a render of one ctx order themselves on the stream).  Per batch: k_paths
// (segment 0), the render's per-bounce launches and tail (run_batch), k_radiance into the caller's
// records.  The tail threshold is the render's without the fused first launch's extra bounce.
hipError_t ray_color(Buffers& B, const PathQuery& Q, hipStream_t st, std::string& err) {
    if (Q.n == 0) return hipSuccess;
    const uint32_t log2 = Q.paths_log2 ? Q.paths_log2 : (uint32_t)OM_WF_QUERY_PATHS_LOG2;
    const uint64_t max_paths = std::min<uint64_t>(Q.n, 1ull << log2);
    Launch L{};
    L.S = Q.S; L.P = Q.P; L.counters = Q.counters; L.count = Q.count; L.timer = Q.timer;
    const uint32_t cap = depth_cap(L.P);
    const DeviceLimits dev = device_limits();
    const int tr = pick_trace(Q.trace_mode, L.S);
    const bool march = has_marched(L.S);
    const bool exact = march && L.S.n_msdf == 0u && MarchedC2Lds::matches(L.S.n_msph, L.S.n_mbox, L.S.n_mtor);
    const bool l2_tree = tr_base(tr) == TR_BVH2_GLOBAL || tr_base(tr) == TR_BVH4_GLOBAL || tr_base(tr) == TR_BVH2_WIDE;
    const uint32_t tail_at = Q.tail_bounce ? Q.tail_bounce : march ? std::max<uint32_t>(kTailMarched, 1u)
                           : l2_tree ? kTailL2 : kTailDefault;
    const uint32_t lanes_per_cu = (march || l2_tree) ? OM_WF_LANES_PER_CU_WIDE : OM_WF_LANES_PER_CU;
    const uint32_t nseg = deal_segments(max_paths, (uint32_t)dev.cus, lanes_per_cu, kBlk, kTailSpb);
    const uint32_t segcap = batch_deal(max_paths, nseg).capacity();
    const uint32_t lds = trace_lds(tr, L.S);
    const uint32_t tail_grid = (uint32_t)dev.cus * kTailWgsPerCu;
    if (!march && tail_at < cap && tail_lds(lds, nseg) > (uint32_t)dev.lds_max) {
        err = "the tail's LDS request exceeds the device's limit";
        return hipErrorInvalidValue;
    }
    if (lds > (uint32_t)dev.lds_max) {
        err = "the traversal's LDS request exceeds the device's limit";
        return hipErrorInvalidValue;
    }
    // (an existing larger set, or more sets, stay as they are: grow never shrinks)
    hipError_t e = grow(B, (uint64_t)nseg * segcap, count_rows(cap) * nseg + 1u, std::max(B.nsets, 1));
    if (e != hipSuccess) { err = "wavefront buffer allocation failed"; return e; }
    QueueSet& QS = B.set[0];
    Timer& tm = *L.timer;
    const int call_ti = tm.begin(st);
    const Gen R{};
    uint32_t launches = 0;
    for (uint64_t at = 0; at < Q.n; at += max_paths) {
        RaySrc X;
        X.n = (uint32_t)std::min<uint64_t>(max_paths, Q.n - at);
        X.rays = Q.rays + at;
        X.rng = Q.rng ? Q.rng + at : nullptr;
        X.stream0 = Q.stream_base + (uint32_t)at;                  // (mod 2^32)
        X.sample = Q.sample;
        Seg G;
        G.nseg = nseg;
        G.segcap = batch_deal(X.n, nseg).capacity();
        with_tr(tr, [&](auto t) {
            constexpr int TR = decltype(t)::value;
            with_flags({L.count, march, exact && exact_view_built<TR>()}, [&](auto count, auto mar, auto ex) {
                if constexpr (mar || !ex) launches += run_batch<TR, count, mar, ex>(QS, L, st, G, R, tail_at, lds, tail_grid, &X);
            });
        });
        hipLaunchKernelGGL(k_radiance, dim3((X.n + 255u) / 256u), dim3(256), 0, st, (const float4*)QS.res,
                           (const uint32_t*)QS.res_id, X.n, Q.out + at);
        if ((e = hipGetLastError()) != hipSuccess) { err = "path query launch failed"; return e; }
    }
    tm.end(call_ti, OM_KT_BOUNCE_SPAN, st, launches);
    return hipSuccess;
}

// A frame from the caller's rays (om_render_rays*): Q.P.sample_count samples of the
// Q.n_pixels listed pixels, ray_color of Q.rays[s * n_pixels + k] added to the pixel's Stats in
// sample order.  A batch is a rectangle of the call with at most 2^paths_log2 paths: all listed
// pixels times as many whole samples as fit, or, for a list longer than a batch, a range of the list
// times one sample.  Per pixel range the sample batches run in order, one after another on `st`
// through queue set 0: k_frame_paths (liveness on the live Stats, segment 0), run_batch's launches and
// tail, k_accumulate in its fixed-list form over the range.  The previous batch's accumulate has run
// when k_frame_paths reads the Stats, so a full or retired pixel costs a kNoSample store per sample
// from the next batch on; inside a batch its later samples are traced and dropped in sample order.
hipError_t render_rays(Buffers& B, const FrameRays& Q, hipStream_t st, std::string& err) {
    const uint32_t n_px = Q.n_pixels, S_call = Q.P.sample_count;
    if (n_px == 0 || S_call == 0 || Q.P.spp_total == 0) return hipSuccess;
    const uint32_t log2 = Q.paths_log2 ? Q.paths_log2 : (uint32_t)OM_WF_QUERY_PATHS_LOG2;
    const uint64_t batch_paths = 1ull << log2;
    const uint32_t range_max = (uint32_t)std::min<uint64_t>(n_px, batch_paths);
    const uint32_t b_max = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(S_call, batch_paths / range_max));
    const uint64_t max_paths = (uint64_t)range_max * b_max;
    Launch L{};
    L.S = Q.S; L.P = Q.P; L.counters = Q.counters; L.count = Q.count; L.timer = Q.timer;
    const uint32_t cap = depth_cap(L.P);
    const DeviceLimits dev = device_limits();
    const int tr = pick_trace(Q.trace_mode, L.S);
    const bool march = has_marched(L.S);
    const bool exact = march && L.S.n_msdf == 0u && MarchedC2Lds::matches(L.S.n_msph, L.S.n_mbox, L.S.n_mtor);
    const bool l2_tree = tr_base(tr) == TR_BVH2_GLOBAL || tr_base(tr) == TR_BVH4_GLOBAL || tr_base(tr) == TR_BVH2_WIDE;
    // (ray_color's threshold: there is no fused first launch here either)
    const uint32_t tail_at = Q.tail_bounce ? Q.tail_bounce : march ? std::max<uint32_t>(kTailMarched, 1u)
                           : l2_tree ? kTailL2 : kTailDefault;
    const uint32_t lanes_per_cu = (march || l2_tree) ? OM_WF_LANES_PER_CU_WIDE : OM_WF_LANES_PER_CU;
    const uint32_t nseg = deal_segments(max_paths, (uint32_t)dev.cus, lanes_per_cu, kBlk, kTailSpb);
    const uint32_t segcap = batch_deal(max_paths, nseg).capacity();
    const uint32_t lds = trace_lds(tr, L.S);
    const uint32_t tail_grid = (uint32_t)dev.cus * kTailWgsPerCu;
    if (!march && tail_at < cap && tail_lds(lds, nseg) > (uint32_t)dev.lds_max) {
        err = "the tail's LDS request exceeds the device's limit";
        return hipErrorInvalidValue;
    }
    if (lds > (uint32_t)dev.lds_max) {
        err = "the traversal's LDS request exceeds the device's limit";
        return hipErrorInvalidValue;
    }
    hipError_t e = grow(B, (uint64_t)nseg * segcap, count_rows(cap) * nseg + 1u, std::max(B.nsets, 1));
    if (e != hipSuccess) { err = "wavefront buffer allocation failed"; return e; }
    QueueSet& QS = B.set[0];
    Timer& tm = *L.timer;
    const int call_ti = tm.begin(st);
    const Gen R{};
    uint32_t launches = 0;
    for (uint32_t k0 = 0; k0 < n_px; k0 += range_max) {
        const uint32_t range = std::min(range_max, n_px - k0);
        for (uint32_t s0 = 0; s0 < S_call; s0 += b_max) {
            const uint32_t b = std::min(b_max, S_call - s0);
            const uint64_t first = (uint64_t)s0 * n_px + k0;
            FrameSrc F;
            F.rays = Q.rays + first;
            F.rng = Q.rng ? Q.rng + first : nullptr;
            F.ray_stride = n_px;
            F.stats = Q.stats;
            F.pixels = Q.pixels ? Q.pixels + k0 : nullptr;
            F.pixel0 = k0;
            F.range = range; F.samples = b;
            Seg G;
            G.nseg = nseg;
            G.segcap = batch_deal((uint64_t)range * b, nseg).capacity();
            with_tr(tr, [&](auto t) {
                constexpr int TR = decltype(t)::value;
                with_flags({L.count, march, exact && exact_view_built<TR>()}, [&](auto count, auto mar, auto ex) {
                    if constexpr (mar || !ex)
                        launches += run_batch<TR, count, mar, ex>(QS, L, st, G, R, tail_at, lds, tail_grid, nullptr, &F);
                });
            });
            // list entry kk of the range: pixels[k0 + kk], or pixel k0 + kk of a whole frame
            const int ati = tm.mode == 1 ? tm.begin(st) : -1;
            with_flags({L.count}, [&](auto count) {
                hipLaunchKernelGGL(k_accumulate<count>, dim3((range + kBlk - 1u) / kBlk), dim3(kBlk), 0, st, L.P,
                                   Q.pixels ? Q.stats : Q.stats + k0, F.pixels, range, Q.pixels ? 1u : 0u, b,
                                   (const float4*)QS.res, (const uint32_t*)QS.res_id, L.S.bloom, AdList{}, L.counters);
            });
            tm.end(ati, OM_KT_ACCUMULATE, st);
            if (Q.progress_host)
                (void)hipMemcpyAsync(Q.progress_host, L.counters + OMC_PROGRESS, sizeof(unsigned long long),
                                     hipMemcpyDeviceToHost, st);
            if ((e = hipGetLastError()) != hipSuccess) { err = "render_rays launch failed"; return e; }
        }
    }
    tm.end(call_ti, OM_KT_BOUNCE_SPAN, st, launches);
    return hipSuccess;
}

// Workgroups the device holds at once at the bounce kernels' occupancy request (OM_WF_WAVES waves
// per SIMD, 4 SIMDs per CU): the grid cap of the persistent k_query.
uint32_t max_grid(const DeviceLimits& d) { return (uint32_t)d.cus * (uint32_t)(OM_WF_WAVES * 4 * 64 / kBlk); }
uint32_t query_max_grid() { return max_grid(device_limits()); }

void tree_regime(int trace_mode, const OmSceneDev& S, int32_t* regime, uint32_t* lds_bytes) {
    const int tr = pick_trace(trace_mode, S);
    const int b = tr_base(tr);
    // TR_BVH counts as the fallback only where a BVH2-family choice fell back to it
    const bool asked_b2 = trace_mode == TR_BVH2_LDS || trace_mode == TR_BVH4_LDS || trace_mode == TR_BVH2_WIDE;
    *regime = b == TR_BVH2_LDS ? OM_TREE_LDS : b == TR_BVH2_GLOBAL ? OM_TREE_L2 : b == TR_BVH2_WIDE ? OM_TREE_WIDE
            : (b == TR_BVH && asked_b2) ? OM_TREE_FALLBACK_BVH : OM_TREE_NONE;
    *lds_bytes = trace_lds(tr, S);
}

// One k_query (Q.hits) or k_occluded (Q.occluded) launch on `st`: the variant renders would trace
// with (pick_trace), MARCH / USER from the world's marched and SDF-program counts.
hipError_t query(const Query& Q, hipStream_t st) {
    if (Q.n == 0) return hipSuccess;
    const int tr = pick_trace(Q.trace_mode, Q.S);
    const uint32_t lds = trace_lds(tr, Q.S);
    // refused here, not as a launch error (a wide tree at the 32-entry bound requests 64 KiB of stack)
    const DeviceLimits dev = device_limits();
    if (lds > (uint32_t)dev.lds_max) return hipErrorInvalidValue;
    const bool march = has_marched(Q.S);
    const bool user = Q.S.n_msdf != 0u;                      // (a user object is a marched one)
    OmParamsDev P{};
    P.tmin = Q.tmin; P.tmax = Q.tmax; P.march_steps = Q.march_steps;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)Q.n + kBlk - 1u) / kBlk, max_grid(dev));
    with_tr(tr, [&](auto t) {
        constexpr int TR = decltype(t)::value;
        if (Q.occluded)
            with_flags({march, Q.count}, [&](auto mar, auto count) {
                hipLaunchKernelGGL((k_occluded<TR, mar, count>), dim3(grid), dim3(kBlk), lds, st, Q.S, P, Q.rays, Q.windows, Q.n,
                                   Q.occluded, Q.counters);
            });
        else
            with_flags({march, user, Q.windows != nullptr, Q.count}, [&](auto mar, auto usr, auto win, auto count) {
                if constexpr (!mar && usr) return;
                else if constexpr (win)
                    hipLaunchKernelGGL((k_query_windows<TR, mar, usr, count>), dim3(grid), dim3(kBlk), lds, st, Q.S, P, Q.rays,
                                       Q.windows, Q.n, Q.hits, Q.counters);
                else
                    hipLaunchKernelGGL((k_query<TR, mar, usr, count>), dim3(grid), dim3(kBlk), lds, st, Q.S, P, Q.rays, Q.n, Q.hits,
                                       Q.counters);
            });
    });
    return hipGetLastError();
}

}  // namespace omw
