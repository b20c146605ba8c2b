// om_render.hip — the C API of libottomarcher.so (include/ottomarcher.h), host side: the context,
// world upload, render and ray-query entry points, counters, timing, progress and display.  The
// kernels are elsewhere: a render call goes to the wavefront (om_wavefront.hip) or the megakernel
// (om_megakernel.hip), a ray query to om_wavefront.hip, a view to om_display.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/ottomarcher.h"
#include "om_device.h"
#include "om_layout.h"
#include "om_display.h"
#include "om_tiles.h"
#include "om_wavefront.h"
#include "om_world.h"
#include "om_internal.h"
#include "om_refit_dev.h"

using namespace omd;

static_assert(sizeof(om_pixel_stats) == 40, "om_pixel_stats layout");
static_assert(sizeof(om_ray) == 24 && sizeof(om_hit) == 32 && sizeof(om_query_params) == 16, "query record layouts");
static_assert(sizeof(om_ray_window) == 8, "query window layout");
static_assert(sizeof(om_path_params) == 32 && sizeof(om_radiance) == 20, "radiance query layouts");
static_assert(OM_QUERY_BLOCK == 512, "OM_QUERY_BLOCK is the wavefront workgroup size");
static_assert(sizeof(OmAffineTest) == 64 && sizeof(OmBvhNode) == 32, "layout");
static_assert(sizeof(OmBvh2NodeW) == sizeof(OmBvh2NodeH) && sizeof(om_tree_info) == 32, "wide node / om_tree_info layout");

namespace {

thread_local std::string g_err;

struct DevBuf {
    void* p = nullptr;
    size_t n = 0;
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

}  // namespace

struct om_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    std::vector<DevBuf> scene_bufs;
    OmSceneDev scene{};
    bool have_world = false;
    om_tree_info tree_info{};           // the uploaded world's trees (om_get_tree_info)
    int kernel = OM_KERNEL_AUTO;
    DevBuf counters, stats, pixels, view_scratch, view_rgb;
    // jitter tables, one immutable device buffer per (seed, spp_total): a table that queued
    // kernels may still read is never rewritten in place (most recent first, kMaxJitterTables)
    struct JitterTable { uint64_t seed; uint32_t spp; DevBuf buf; };
    std::vector<JitterTable> jitters;
    hipStream_t last_stream = nullptr;
    bool count_work = true;
    int pipeline = OM_PIPELINE_AUTO;
    uint32_t tail_bounce = 0;
    uint32_t wf_streams = 2;            // wavefront calls: batches in flight (om_set_streams)
    uint32_t ad_batches = 0, ad_paths_log2 = 0;   // adaptive wavefront schedule (om_set_adaptive_batches; 0 = default)
    // primary-ray tile lists (om_tiles.h): host record boxes of the uploaded world, the
    // device lists of the last (camera, frame, world) and the policy (om_set_primary_lists)
    std::vector<float> srec_box;
    uint64_t world_gen = 0;
    int primary_lists = OM_PRIMARY_LISTS_AUTO;
    DevBuf tile_off, tile_idx, tile_tnear;
    bool tiles_valid = false, tiles_use = false;
    float root_box[6] = {0, 0, 0, 0, 0, 0};   // box of the bounded primitives (the global BVH's root); have_root: there is one
    bool have_root = false;
    om_camera tiles_cam{};
    uint32_t tiles_w = 0, tiles_h = 0;
    uint64_t tiles_gen = 0;
    double tiles_avg = 0.0;
    omw::Timer timer;
    omw::Buffers wf;
    unsigned long long* progress_host = nullptr;   // om_progress: pinned host word (null: progress off)
    DevBuf frame_list;                  // tile-ordered pixel list of the full frame (wavefront path)
    DevBuf query_rays, query_hits;      // om_hit_rays staging (grown on demand, reused)
    DevBuf query_windows, query_occ;    // om_*_windows / om_occluded_rays staging
    DevBuf path_rng, path_out;          // om_ray_color staging (the rays go through query_rays)
    uint32_t path_batch_log2 = 0;       // om_set_path_batch (0 = default)
    uint32_t frame_w = 0, frame_h = 0;
    // om_update_triangles (om_refit.hip): the uploaded world's refit tables (their
    // buffers are scene_bufs), staging of the host form, and what the host keeps of the boxes: the
    // root box comes back through a pinned node after each update (root_ev: that copy; two of each,
    // used in turn, so that an update does not wait on the host for the one before it), the record
    // boxes of the tile lists are fetched when the next lists are built (boxes_stale)
    omr::Tables refit;
    DevBuf upd_vertices, upd_indices;
    OmBvhNode* root_host = nullptr;       // two nodes
    hipEvent_t root_ev[2] = {nullptr, nullptr};
    uint32_t root_slot = 0;               // the slot of the last update
    bool root_used[2] = {false, false};   // a copy into the slot has been queued
    bool root_pending = false, boxes_stale = false;
    om_update_info update_info{};
    ~om_ctx() {
        for (auto& b : scene_bufs) b.release();
        for (auto& j : jitters) j.buf.release();
        counters.release(); stats.release(); pixels.release(); frame_list.release();
        query_rays.release(); query_hits.release();
        query_windows.release(); query_occ.release();
        path_rng.release(); path_out.release();
        view_scratch.release(); view_rgb.release(); tile_off.release(); tile_idx.release(); tile_tnear.release();
        wf.release();
        timer.release();
        upd_vertices.release(); upd_indices.release();
        if (root_host) (void)hipHostFree(root_host);
        for (hipEvent_t e : root_ev) if (e) (void)hipEventDestroy(e);
        if (progress_host) (void)hipHostFree(progress_host);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

om_status set_err(om_ctx* c, om_status code, const std::string& msg) {
    g_err = msg;
    if (c) c->err = msg;
    return code;
}
#define OM_HIP(ctx, call)                                                                       \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) return set_err(ctx, OM_ERR_DEVICE, std::string(#call ": ") + hipGetErrorString(e_)); \
    } while (0)

template <class T>
om_status upload(om_ctx* c, const std::vector<T>& v, const T** out) {
    *out = nullptr;
    if (v.empty()) return OM_OK;
    DevBuf b;
    b.n = v.size() * sizeof(T);
    OM_HIP(c, hipMalloc(&b.p, b.n));
    c->scene_bufs.push_back(b);
    OM_HIP(c, hipMemcpyAsync(b.p, v.data(), b.n, hipMemcpyHostToDevice, c->stream));
    *out = (const T*)b.p;
    return OM_OK;
}

om_status ensure(om_ctx* c, DevBuf& b, size_t n) {
    if (b.n >= n) return OM_OK;
    b.release();
    OM_HIP(c, hipMalloc(&b.p, n));
    b.n = n;
    return OM_OK;
}

// jitter table render_thread.rs:164-174: ((s/2)&1, s&1) shuffled once (om-rng SplitMix64 Fisher-Yates).
// Each (seed, spp) gets its own device buffer, written once before any kernel can read it,
// so an asynchronous call with another seed never races a queued one.
constexpr size_t kMaxJitterTables = 8;
om_status prepare_jitter(om_ctx* c, uint64_t seed, uint32_t spp, const float2** out) {
    *out = nullptr;
    for (size_t i = 0; i < c->jitters.size(); ++i)
        if (c->jitters[i].seed == seed && c->jitters[i].spp == spp) {
            if (i) std::rotate(c->jitters.begin(), c->jitters.begin() + i, c->jitters.begin() + i + 1);
            *out = (const float2*)c->jitters[0].buf.p;
            return OM_OK;
        }
    std::vector<float> jt(2 * (size_t)spp);
    for (uint32_t s = 0; s < spp; ++s) { jt[2 * s] = (float)((s / 2) & 1u); jt[2 * s + 1] = (float)(s & 1u); }
    auto mix = [](uint64_t z) {
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        return z ^ (z >> 31);
    };
    uint64_t st = mix(seed ^ 0x4A177E5B0C1D2E3FULL);
    for (uint32_t i = spp; i-- > 1;) {
        st += 0x9E3779B97F4A7C15ULL;
        const uint32_t j = (uint32_t)((mix(st) >> 32) % (uint64_t)(i + 1));
        std::swap(jt[2 * i], jt[2 * j]);
        std::swap(jt[2 * i + 1], jt[2 * j + 1]);
    }
    if (c->jitters.size() >= kMaxJitterTables) {      // evict the least recent once the device is idle
        OM_HIP(c, hipDeviceSynchronize());
        c->jitters.back().buf.release();
        c->jitters.pop_back();
    }
    om_ctx::JitterTable t{seed, spp, DevBuf{}};
    om_status s = ensure(c, t.buf, jt.size() * sizeof(float) + 16);
    if (s) return s;
    const hipError_t e = hipMemcpyAsync(t.buf.p, jt.data(), jt.size() * sizeof(float), hipMemcpyHostToDevice, c->stream);
    const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(c->stream) : e;   // jt is a host temporary
    if (e2 != hipSuccess) {
        t.buf.release();
        return set_err(c, OM_ERR_DEVICE, std::string("jitter upload: ") + hipGetErrorString(e2));
    }
    c->jitters.insert(c->jitters.begin(), t);
    *out = (const float2*)t.buf.p;
    return OM_OK;
}

om_status validate(om_ctx* c, const om_camera* cam, const om_render_params* p) {
    if (!c) return set_err(nullptr, OM_ERR_INVALID, "null ctx");
    if (!cam || !p) return set_err(c, OM_ERR_INVALID, "null camera/params");
    if (!c->have_world) return set_err(c, OM_ERR_STATE, "om_upload_world must precede rendering");
    if (p->width == 0 || p->height == 0) return set_err(c, OM_ERR_INVALID, "width/height must be > 0");
    if ((uint64_t)p->width * p->height > (1ull << 31)) return set_err(c, OM_ERR_INVALID, "image too large");
    return OM_OK;
}

// Primary-ray candidate lists for (camera, frame, world), rebuilt only when one changes.
// AUTO uses them when a pixel sees <= 12 candidates on average (a primary BVH2 traversal
// costs ~11 node visits + 3.5 exact tests); S-traced at 1080p sees 3.2 (max 14 per tile).
constexpr double kTileListMaxAvg = 12.0;
om_status ensure_tile_lists(om_ctx* c, const om_camera* cam, uint32_t W, uint32_t H, hipStream_t stream) {
    if (c->primary_lists == OM_PRIMARY_LISTS_OFF) { c->tiles_use = false; return OM_OK; }
    const bool same = c->tiles_valid && c->tiles_gen == c->world_gen && c->tiles_w == W && c->tiles_h == H &&
                      std::memcmp(&c->tiles_cam, cam, sizeof(om_camera)) == 0;
    if (!same) {
        if (c->boxes_stale) {       // an update moved boxes: the records' own, from the device
            std::vector<float> pb((size_t)c->refit.n_prim * 6u);
            std::vector<uint32_t> items(c->refit.n_titems);
            OM_HIP(c, hipStreamSynchronize(stream));
            if (c->last_stream && c->last_stream != stream) OM_HIP(c, hipStreamSynchronize(c->last_stream));
            OM_HIP(c, hipMemcpy(pb.data(), c->refit.prim_box, pb.size() * 4u, hipMemcpyDeviceToHost));
            if (!items.empty()) OM_HIP(c, hipMemcpy(items.data(), c->refit.titems, items.size() * 4u, hipMemcpyDeviceToHost));
            for (size_t r = 0; r < items.size(); ++r) std::copy_n(pb.begin() + 6u * (size_t)items[r], 6, c->srec_box.begin() + 6u * r);
            c->boxes_stale = false;
        }
        omt::TileLists tl;
        const bool ok = omt::build(c->srec_box, *cam, W, H, tl);
        // the cache keys are set only once the device lists are complete: a failed upload
        // leaves tiles_valid false, so the next call rebuilds instead of reading stale lists
        c->tiles_valid = false;
        c->tiles_use = false;
        if (ok) {
            om_status s = ensure(c, c->tile_off, tl.off.size() * 4u);
            // +1 entry: the uniform (scalar) reader loads whole dwords (traced_tiles<true>, om_trace.h)
            if (s == OM_OK) s = ensure(c, c->tile_idx, (tl.idx.size() + 2u) * 2u);
            if (s == OM_OK) s = ensure(c, c->tile_tnear, std::max<size_t>(tl.tnear.size(), 1u) * 4u);
            if (s != OM_OK) return s;
            OM_HIP(c, hipStreamSynchronize(stream));        // the previous lists may still be read
            OM_HIP(c, hipMemcpy(c->tile_off.p, tl.off.data(), tl.off.size() * 4u, hipMemcpyHostToDevice));
            if (!tl.idx.empty()) OM_HIP(c, hipMemcpy(c->tile_idx.p, tl.idx.data(), tl.idx.size() * 2u, hipMemcpyHostToDevice));
            if (!tl.tnear.empty())
                OM_HIP(c, hipMemcpy(c->tile_tnear.p, tl.tnear.data(), tl.tnear.size() * 4u, hipMemcpyHostToDevice));
        }
        c->tiles_valid = true; c->tiles_gen = c->world_gen; c->tiles_w = W; c->tiles_h = H; c->tiles_cam = *cam;
        c->tiles_avg = ok ? tl.avg_per_pixel : -1.0;
    }
    c->tiles_use = c->tiles_avg >= 0.0 &&
                   (c->primary_lists == OM_PRIMARY_LISTS_ON || c->tiles_avg <= kTileListMaxAvg);
    return OM_OK;
}

// omw::Launch::trace_mode of a resolved (non-AUTO) OM_KERNEL_* choice
int wf_trace_mode(int mode) {
    return mode == OM_KERNEL_BRUTE ? TR_BRUTE : mode == OM_KERNEL_CULLED ? TR_CULLED
         : mode == OM_KERNEL_BVH ? TR_BVH : mode == OM_KERNEL_BVH2 ? TR_BVH2_LDS
         : mode == OM_KERNEL_BVH4 ? TR_BVH4_LDS : mode == OM_KERNEL_BVH2W ? TR_BVH2_WIDE : TR_SBVH_LDS;
}

// The wavefront's pixel list of a full frame: 8x8 tiles in row-major tile order, lanes row-major
// inside a tile; rebuilt when the frame size changes.
om_status ensure_frame_list(om_ctx* c, uint32_t W, uint32_t H, hipStream_t stream) {
    if (c->frame_w == W && c->frame_h == H && c->frame_list.p) return OM_OK;
    std::vector<uint32_t> lst;
    lst.reserve((size_t)W * H);
    const uint32_t tx = (W + 7u) / 8u, ty = (H + 7u) / 8u;
    for (uint32_t t = 0; t < tx * ty; ++t)
        for (uint32_t l = 0; l < 64u; ++l) {
            const uint32_t px = (t % tx) * 8u + (l & 7u), py = (t / tx) * 8u + (l >> 3);
            if (px < W && py < H) lst.push_back(py * W + px);
        }
    om_status s = ensure(c, c->frame_list, lst.size() * 4);
    if (s != OM_OK) return s;
    OM_HIP(c, hipMemcpyAsync(c->frame_list.p, lst.data(), lst.size() * 4, hipMemcpyHostToDevice, stream));
    OM_HIP(c, hipStreamSynchronize(stream));
    c->frame_w = W; c->frame_h = H;
    return OM_OK;
}

om_status launch(om_ctx* c, const om_camera* cam, const om_render_params* p, om_pixel_stats* dev_stats,
                 const uint32_t* dev_pixels, uint32_t n_pixels, hipStream_t stream) {
    // samples_per_pixel = 0: render()'s pass loop never runs (render_thread.rs:176), Stats untouched
    if (p->spp_total == 0 || p->sample_count == 0) return OM_OK;
    omw::Launch L;
    om_status s = prepare_jitter(c, p->seed, p->spp_total, &L.jitter);
    if (s) return s;
    if (!c->counters.p) {
        s = ensure(c, c->counters, OMC_SLOTS * sizeof(unsigned long long));
        if (s) return s;
        OM_HIP(c, hipMemsetAsync(c->counters.p, 0, OMC_SLOTS * sizeof(unsigned long long), stream));
    }
    c->last_stream = stream;
    OmCamDev& C = L.C;
    for (int i = 0; i < 3; ++i) {
        C.origin[i] = cam->origin[i]; C.horizontal[i] = cam->horizontal[i]; C.vertical[i] = cam->vertical[i];
        C.llc_minus_origin[i] = cam->lower_left_corner[i] - cam->origin[i];          // camera.rs:72
        C.u[i] = cam->u_of_plane[i]; C.v[i] = cam->v_of_plane[i];
    }
    C.lens_radius = cam->lens_radius;
    OmParamsDev& P = L.P;
    P.width = p->width; P.height = p->height; P.spp_total = p->spp_total; P.sample_count = p->sample_count;
    P.max_depth = p->max_depth; P.march_steps = p->march_steps; P.adaptive = p->adaptive ? 1u : 0u;
    P.tmin = p->tmin; P.tmax = p->tmax;
    P.wf_m1 = (float)p->width - 1.0f; P.hf_m1 = (float)p->height - 1.0f;             // render_thread.rs:190-191
    const uint64_t sk = p->seed + 0x632BE59BD9B4E019ULL;
    uint64_t z = sk;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    P.skey = z ^ (z >> 31);
    P.tiles_x = (p->width + 7u) / 8u;
    P.progress = c->progress_host ? 1u : 0u;
    P.n_pixels = dev_pixels ? n_pixels : p->width * p->height;
    if (P.n_pixels == 0) return OM_OK;
    int mode = c->kernel;
    if (mode == OM_KERNEL_AUTO) mode = OM_KERNEL_BVH2;
    // A camera beyond the reach of the slab test (beyond_slab_reach, the rule of far_origin in
    // om_wavefront.hip, against the box of the bounded primitives) renders with the reference loop:
    // out there the slab test is no finer than the box inflation.  Decided per call
    // on the host; no other frame runs anything else.
    if (c->root_pending) {          // the last update's root box (its copy is queued behind the refit)
        const OmBvhNode& root = c->root_host[c->root_slot];
        OM_HIP(c, hipEventSynchronize(c->root_ev[c->root_slot]));
        for (int i = 0; i < 3; ++i) { c->root_box[i] = root.lo[i]; c->root_box[3 + i] = root.hi[i]; }
        c->root_pending = false;
    }
    if (c->have_root && beyond_slab_reach(c->root_box, c->root_box + 3, cam->origin[0], cam->origin[1], cam->origin[2]))
        mode = OM_KERNEL_BRUTE;
    L.S = c->scene;
    L.stats = dev_stats;
    L.pixels = dev_pixels; L.n_pixels = P.n_pixels; L.stats_by_pixel = !dev_pixels;
    L.counters = (unsigned long long*)c->counters.p;
    L.count = c->count_work;
    L.trace_mode = wf_trace_mode(mode);
    L.tail_bounce = c->tail_bounce;
    L.streams = c->wf_streams;
    L.ad_batches = c->ad_batches; L.ad_paths_log2 = c->ad_paths_log2;
    L.timer = &c->timer;
    L.tile_off = nullptr; L.tile_idx = nullptr; L.tile_tnear = nullptr;
    L.progress_host = c->progress_host;
    std::string err;
    hipError_t e;
    // AUTO: the wavefront, the faster pipeline on every measured config since r04:
    // C1 6100 vs 3142 Msamples/s, C2 with one stream 2377 vs 1180-1202 (r04_ad), C2 adaptive 2939 vs
    // 1041 credited (16-sample calls), C1 adaptive 3466 vs 2832 (16-sample calls), 4199 vs 3388 (64),
    // all counting build; production build, C1 adaptive 64 spp in one call: 7171 vs 3392-3507 (r04_q7).
    if (c->pipeline == OM_PIPELINE_MEGAKERNEL) {
        e = omw::render_megakernel(L, stream, err);
    } else {
        // (a tree past the 15-bit codes has n_b2nodes 0: its primary rays traverse, and om_tiles.cpp
        // lists at most 65 535 records anyway; OM_KERNEL_BVH2W takes the lists like OM_KERNEL_BVH2)
        if ((mode == OM_KERNEL_BVH2 && c->scene.n_b2nodes) || (mode == OM_KERNEL_BVH2W && c->scene.n_b2wnodes)) {
            if ((s = ensure_tile_lists(c, cam, p->width, p->height, stream)) != OM_OK) return s;
            if (c->tiles_use) {
                L.tile_off = (const uint32_t*)c->tile_off.p; L.tile_idx = (const uint16_t*)c->tile_idx.p;
                L.tile_tnear = (const float*)c->tile_tnear.p;
            }
        }
        if (!dev_pixels) {
            if ((s = ensure_frame_list(c, p->width, p->height, stream)) != OM_OK) return s;
            L.pixels = (const uint32_t*)c->frame_list.p;
        }
        e = omw::render(c->wf, L, stream, err);
    }
    if (e != hipSuccess) return set_err(c, OM_ERR_DEVICE, err + ": " + hipGetErrorString(e));
    return OM_OK;
}

}  // namespace

extern "C" {

const char* om_world_last_error_internal(void);

om_status om_create(int32_t device, om_ctx** out) {
    if (!out) return set_err(nullptr, OM_ERR_INVALID, "om_create: null out");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) return set_err(nullptr, OM_ERR_DEVICE, "om_create: no HIP device available");
    if (device < 0 || device >= n) return set_err(nullptr, OM_ERR_INVALID, "om_create: device index out of range");
    om_ctx* c = new (std::nothrow) om_ctx();
    if (!c) return set_err(nullptr, OM_ERR_NOMEM, "om_create: out of memory");
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return set_err(nullptr, OM_ERR_DEVICE, "om_create: stream creation failed");
    }
    *out = c;
    return OM_OK;
}

void om_destroy(om_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c;
}

const char* om_last_error(const om_ctx* c) {
    if (c) return c->err.c_str();
    if (!g_err.empty()) return g_err.c_str();
    return om_world_last_error_internal();
}

om_status om_upload_world(om_ctx* c, const om_world* w) {
    if (!c || !w) return set_err(c, OM_ERR_INVALID, "om_upload_world: null pointer");
    OM_HIP(c, hipSetDevice(c->device));
    OM_HIP(c, hipStreamSynchronize(c->stream));
    for (auto& b : c->scene_bufs) b.release();
    c->scene_bufs.clear();
    c->have_world = false;
    om::FrozenWorld fw;
    om::RefitTables rt;
    w->freeze(fw, &rt);
    c->refit = omr::Tables();
    c->root_pending = false; c->boxes_stale = false;
    c->root_used[0] = c->root_used[1] = false;       // (the stream was synchronised above: no copy is in flight)
    c->update_info = om_update_info{};
    OmSceneDev& S = c->scene;
    S = OmSceneDev{};
    om_status s = OM_OK;
#define UP(vec, field) if ((s = upload(c, fw.vec, &S.field)) != OM_OK) return s
    UP(sph_test, sph_test); UP(sph_hit, sph_hit); UP(sph_bound, sph_bound);
    UP(cube_test, cube_test); UP(cube_hit, cube_hit); UP(cube_bound, cube_bound);
    UP(tri, tri); UP(plane, plane); UP(para, para);
    UP(msph, msph); UP(mbox, mbox); UP(mtor, mtor); UP(msdf, msdf); UP(msdf_ops, msdf_ops);
    UP(mats, mats); UP(bloom, bloom); UP(bvh, bvh); UP(bvh_prims, bvh_prims); UP(always, always);
    UP(snodes, snodes); UP(srecs, srecs); UP(always2, always2); UP(always2_rec, always2_rec); UP(b2nodes, b2nodes); UP(b2leaves, b2leaves);
#undef UP
    // which trees are usable and which are staged in LDS: om::plan_trees (om_world.h)
    const om::TreePlan plan = om::plan_trees(fw);
    // one buffer behind S.b2h: the half nodes of a tree within the 15-bit codes, then the wide nodes
    // (OmBvh2NodeW, same size) of a tree the wide regime can run, which the kernels find at
    // b2h + n_b2nodes -- OmSceneDev keeps its size (om_layout.h)
    {
        static_assert(sizeof(OmBvh2NodeW) == sizeof(OmBvh2NodeH), "wide and half nodes share a buffer");
        std::vector<OmBvh2NodeH> both;
        if (plan.b2_ok) both = fw.b2h;
        if (plan.b2w_ok) {
            const size_t at = both.size();
            both.resize(at + fw.b2w.size());
            std::memcpy(both.data() + at, fw.b2w.data(), fw.b2w.size() * sizeof(OmBvh2NodeW));
        }
        if ((s = upload(c, both, &S.b2h)) != OM_OK) return s;
    }
    c->srec_box = fw.srec_box;
    c->world_gen++;
    c->tiles_valid = false;
    S.n_sph = fw.counts[0]; S.n_cube = fw.counts[1]; S.n_tri = fw.counts[2]; S.n_plane = fw.counts[3]; S.n_para = fw.counts[4];
    S.n_msph = fw.counts[5]; S.n_mbox = fw.counts[6]; S.n_mtor = fw.counts[7]; S.n_msdf = fw.counts[om::K_MSDF];
    S.off_cube = fw.offsets[1]; S.off_tri = fw.offsets[2]; S.off_plane = fw.offsets[3]; S.off_para = fw.offsets[4];
    S.off_msph = fw.offsets[5]; S.off_mbox = fw.offsets[6]; S.off_mtor = fw.offsets[7];
    S.off_msdf = fw.offsets[om::K_MSDF]; S.n_total = fw.offsets[om::K_N];
    S.n_bvh_nodes = (uint32_t)fw.bvh.size();
    c->have_root = !fw.bvh.empty();
    if (c->have_root) for (int i = 0; i < 3; ++i) { c->root_box[i] = fw.bvh[0].lo[i]; c->root_box[3 + i] = fw.bvh[0].hi[i]; }
    S.n_always = (uint32_t)fw.always.size();
    S.n_snodes = (uint32_t)fw.snodes.size(); S.n_srecs = (uint32_t)fw.srecs.size(); S.n_always2 = (uint32_t)fw.always2.size();
    S.lds_bytes = plan.lds_bytes;
    S.n_b2nodes = plan.n_b2nodes; S.n_b2leaves = plan.n_b2leaves;
    S.b2_direct = plan.b2_direct; S.b2_stack = plan.b2_stack; S.b2_lds_bytes = plan.b2_lds_bytes;
    if (plan.b4_ok && (s = upload(c, fw.b4nodes, &S.b4nodes)) != OM_OK) return s;
    if (plan.b4_ok && (s = upload(c, fw.b4h, &S.b4h)) != OM_OK) return s;
    S.n_b4nodes = plan.b4_ok ? (uint32_t)fw.b4nodes.size() : 0u;
    S.b4_stack = plan.b4_stack; S.b4_lds_bytes = plan.b4_lds_bytes;
    S.n_b2wnodes = plan.n_b2wnodes; S.b2w_stack = plan.b2w_stack;
    om::fill_tree_info(fw, plan, &c->tree_info);
    if (!rt.empty()) {              // worlds with triangles: what om_update_triangles needs
        omr::Tables& T = c->refit;
        const float* prim_box = nullptr; const uint32_t *tri_rec = nullptr, *g_level = nullptr, *titems = nullptr, *t_level = nullptr,
                                                        *snode_src = nullptr, *b2_src = nullptr, *b4_src = nullptr, *b4h_src = nullptr;
        const OmBvhNode* tnodes = nullptr;
#define UPT(vec) if ((s = upload(c, rt.vec, &vec)) != OM_OK) return s
        UPT(prim_box); UPT(tri_rec); UPT(g_level); UPT(tnodes); UPT(titems); UPT(t_level); UPT(snode_src); UPT(b2_src);
        if (plan.b4_ok) { UPT(b4_src); UPT(b4h_src); }
#undef UPT
        DevBuf info;
        info.n = omr::kInfoWords * sizeof(uint32_t);
        OM_HIP(c, hipMalloc(&info.p, info.n));
        c->scene_bufs.push_back(info);
        OM_HIP(c, hipMemsetAsync(info.p, 0, info.n, c->stream));
        T.prim_box = (float*)prim_box; T.n_prim = (uint32_t)(rt.prim_box.size() / 6u); T.covering = rt.covering;
        T.tri_first = rt.tri_first; T.n_tri = fw.counts[om::K_TRI]; T.tri_rec = (uint32_t*)tri_rec;
        T.g_level = (uint32_t*)g_level; T.g_level_off = rt.g_level_off;
        T.tnodes = (OmBvhNode*)tnodes; T.n_tnodes = (uint32_t)rt.tnodes.size();
        T.titems = (uint32_t*)titems; T.n_titems = (uint32_t)rt.titems.size();
        T.t_level = (uint32_t*)t_level; T.t_level_off = rt.t_level_off;
        T.snode_src = (uint32_t*)snode_src; T.n_snode = (uint32_t)rt.snode_src.size();
        T.b2_src = (uint32_t*)b2_src; T.n_b2 = (uint32_t)fw.b2nodes.size();
        T.n_b2h = plan.b2_ok ? T.n_b2 : 0u; T.n_b2w = plan.b2w_ok ? T.n_b2 : 0u;
        T.b4_src = (uint32_t*)b4_src; T.b4h_src = (uint32_t*)b4h_src; T.n_b4 = plan.b4_ok ? (uint32_t)fw.b4nodes.size() : 0u;
        T.info = (uint32_t*)info.p;
        if (!c->root_host) OM_HIP(c, hipHostMalloc((void**)&c->root_host, 2u * sizeof(OmBvhNode), hipHostMallocDefault));
        for (hipEvent_t& e : c->root_ev) if (!e) OM_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    // barycentric leaf records carry gi in 30 bits beside the two kind bits (om_layout.h OM_REC_GI)
    S.n_srec_bary = fw.n_srec_bary;
    if (fw.n_srec_bary && fw.offsets[om::K_N] > OM_REC_GI)
        return set_err(c, OM_ERR_UNSUPPORTED, "om_upload_world: a world with triangles in its trees holds at most 2^30 objects");
    OM_HIP(c, hipStreamSynchronize(c->stream));
    c->have_world = true;
    return OM_OK;
}

// ---- moving triangles of the uploaded world ----
static om_status validate_update(om_ctx* c, uint32_t first, const float* vertices, uint32_t n_tri, bool* work) {
    *work = false;
    if (!c) return set_err(nullptr, OM_ERR_INVALID, "om_update_triangles: null ctx");
    if (!c->have_world) return set_err(c, OM_ERR_STATE, "om_upload_world must precede om_update_triangles");
    if ((uint64_t)first + n_tri > c->scene.n_tri) return set_err(c, OM_ERR_INVALID, "om_update_triangles: range past the world's triangles");
    if (n_tri == 0) return OM_OK;
    if (!vertices) return set_err(c, OM_ERR_INVALID, "om_update_triangles: null vertices");
    *work = true;
    return OM_OK;
}

om_status om_update_triangles_device(om_ctx* c, uint32_t first_triangle, const float* dev_vertices, uint32_t n_vertices,
                                     const uint32_t* dev_indices, uint32_t n_tri, void* stream) {
    bool work;
    om_status s = validate_update(c, first_triangle, dev_vertices, n_tri, &work);
    if (s || !work) return s;
    OM_HIP(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    // The new root box for launch()'s far-camera rule comes back through the pinned node the last
    // update did not use; its own earlier copy (two updates ago) must have landed, which is the one
    // wait an update can meet on the host, and it stands before anything is launched.  (Once the
    // kernels are queued the records are being rewritten: an OM_ERR_DEVICE from the launches or from
    // the copy behind them is a device failure, after which the world wants a new upload.)
    const uint32_t slot = c->root_slot ^ 1u;
    if (c->have_root && c->root_used[slot]) OM_HIP(c, hipEventSynchronize(c->root_ev[slot]));
    const hipError_t e = omr::update(c->refit, c->scene, first_triangle, dev_vertices, n_vertices, dev_indices, n_tri, st);
    if (e != hipSuccess) return set_err(c, OM_ERR_DEVICE, std::string("om_update_triangles launch: ") + hipGetErrorString(e));
    if (c->have_root) {
        OM_HIP(c, hipMemcpyAsync(c->root_host + slot, c->scene.bvh, sizeof(OmBvhNode), hipMemcpyDeviceToHost, st));
        OM_HIP(c, hipEventRecord(c->root_ev[slot], st));
        c->root_slot = slot; c->root_used[slot] = true;
        c->root_pending = true;
    }
    c->last_stream = st;
    c->world_gen++;                 // the primary-ray tile lists are of the old boxes
    c->boxes_stale = true;
    c->update_info.updates++;
    c->update_info.triangles = n_tri;
    return OM_OK;
}

om_status om_update_triangles(om_ctx* c, uint32_t first_triangle, const float* vertices, uint32_t n_vertices, const uint32_t* indices,
                              uint32_t n_tri) {
    bool work;
    om_status s = validate_update(c, first_triangle, vertices, n_tri, &work);
    if (s || !work) return s;
    if (!indices && (uint64_t)n_tri * 3u > n_vertices) return set_err(c, OM_ERR_INVALID, "om_update_triangles: vertex index out of range");
    for (size_t k = 0; indices && k < (size_t)n_tri * 3u; ++k)
        if (indices[k] >= n_vertices) return set_err(c, OM_ERR_INVALID, "om_update_triangles: vertex index out of range");
    OM_HIP(c, hipSetDevice(c->device));
    const size_t vb = (size_t)n_vertices * 3u * sizeof(float), ib = (size_t)n_tri * 3u * sizeof(uint32_t);
    if ((s = ensure(c, c->upd_vertices, vb)) != OM_OK) return s;
    if (indices && (s = ensure(c, c->upd_indices, ib)) != OM_OK) return s;
    OM_HIP(c, hipMemcpyAsync(c->upd_vertices.p, vertices, vb, hipMemcpyHostToDevice, c->stream));
    if (indices) OM_HIP(c, hipMemcpyAsync(c->upd_indices.p, indices, ib, hipMemcpyHostToDevice, c->stream));
    s = om_update_triangles_device(c, first_triangle, (const float*)c->upd_vertices.p, n_vertices,
                                   indices ? (const uint32_t*)c->upd_indices.p : nullptr, n_tri, c->stream);
    if (s != OM_OK) return s;
    OM_HIP(c, hipStreamSynchronize(c->stream));
    return OM_OK;
}

om_status om_get_update_info(om_ctx* c, om_update_info* out) {
    if (!c) return set_err(nullptr, OM_ERR_INVALID, "om_get_update_info: null ctx");
    if (!out) return set_err(c, OM_ERR_INVALID, "om_get_update_info: null out");
    if (!c->have_world) return set_err(c, OM_ERR_STATE, "om_upload_world must precede om_get_update_info");
    *out = c->update_info;
    if (!c->refit.ready() || c->update_info.updates == 0u) return OM_OK;
    OM_HIP(c, hipSetDevice(c->device));
    OM_HIP(c, hipStreamSynchronize(c->stream));
    if (c->last_stream && c->last_stream != c->stream) OM_HIP(c, hipStreamSynchronize(c->last_stream));
    uint32_t h[omr::kInfoWords];
    OM_HIP(c, hipMemcpy(h, c->refit.info, sizeof(h), hipMemcpyDeviceToHost));
    out->unbounded = h[omr::kInfoUnbounded]; out->skipped = h[omr::kInfoSkipped];
    out->triangles = c->update_info.triangles - out->skipped;
    return OM_OK;
}

om_status om_set_kernel(om_ctx* c, int32_t k) {
    if (!c) return set_err(nullptr, OM_ERR_INVALID, "null ctx");
    if (k < OM_KERNEL_AUTO || k > OM_KERNEL_BVH2W) return set_err(c, OM_ERR_INVALID, "om_set_kernel: unknown kernel");
    c->kernel = k;
    return OM_OK;
}

om_status om_get_tree_info(om_ctx* c, om_tree_info* out) {
    if (!c) return set_err(nullptr, OM_ERR_INVALID, "om_get_tree_info: null ctx");
    if (!out) return set_err(c, OM_ERR_INVALID, "om_get_tree_info: null out");
    if (!c->have_world) return set_err(c, OM_ERR_STATE, "om_upload_world must precede om_get_tree_info");
    *out = c->tree_info;
    int mode = c->kernel;
    if (mode == OM_KERNEL_AUTO) mode = OM_KERNEL_BVH2;
    omw::tree_regime(wf_trace_mode(mode), c->scene, &out->regime, &out->lds_bytes);
    return OM_OK;
}

om_status om_render_device(om_ctx* c, const om_camera* cam, const om_render_params* p, om_pixel_stats* dev_stats, void* stream) {
    om_status s = validate(c, cam, p);
    if (s) return s;
    if (!dev_stats) return set_err(c, OM_ERR_INVALID, "null dev_stats");
    OM_HIP(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return launch(c, cam, p, dev_stats, nullptr, 0, st);
}

om_status om_render_device_pixels(om_ctx* c, const om_camera* cam, const om_render_params* p, om_pixel_stats* dev_stats,
                                  const uint32_t* dev_pixels, uint32_t n_pixels, void* stream) {
    om_status s = validate(c, cam, p);
    if (s) return s;
    if (!dev_stats || (!dev_pixels && n_pixels)) return set_err(c, OM_ERR_INVALID, "null dev_stats/dev_pixels");
    OM_HIP(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (n_pixels == 0) return OM_OK;
    return launch(c, cam, p, dev_stats, dev_pixels, n_pixels, st);
}

om_status om_render(om_ctx* c, const om_camera* cam, const om_render_params* p, om_pixel_stats* stats, om_counters* counters) {
    om_status s = validate(c, cam, p);
    if (s) return s;
    if (!stats) return set_err(c, OM_ERR_INVALID, "null stats");
    OM_HIP(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)p->width * p->height * sizeof(om_pixel_stats);
    if ((s = ensure(c, c->stats, bytes)) != OM_OK) return s;
    OM_HIP(c, hipMemcpyAsync(c->stats.p, stats, bytes, hipMemcpyHostToDevice, c->stream));
    if ((s = om_reset_counters(c, c->stream)) != OM_OK) return s;
    if ((s = launch(c, cam, p, (om_pixel_stats*)c->stats.p, nullptr, 0, c->stream)) != OM_OK) return s;
    OM_HIP(c, hipMemcpyAsync(stats, c->stats.p, bytes, hipMemcpyDeviceToHost, c->stream));
    OM_HIP(c, hipStreamSynchronize(c->stream));
    if (counters) return om_get_counters(c, counters);
    return OM_OK;
}

// ---- closest-hit ray queries (FrozenHittableList::hit, hits.rs:270-334) ----
static om_status validate_query(om_ctx* c, const om_query_params* q, const void* rays, uint32_t n, const void* hits) {
    if (!c) return set_err(nullptr, OM_ERR_INVALID, "om_hit_rays: null ctx");
    if (!q) return set_err(c, OM_ERR_INVALID, "om_hit_rays: null params");
    if (q->reserved != 0u) return set_err(c, OM_ERR_INVALID, "om_hit_rays: reserved must be 0");
    if (std::isnan(q->tmin) || std::isnan(q->tmax)) return set_err(c, OM_ERR_INVALID, "om_hit_rays: tmin/tmax is NaN");
    if (!c->have_world) return set_err(c, OM_ERR_STATE, "om_upload_world must precede ray queries");
    if (n && (!rays || !hits)) return set_err(c, OM_ERR_INVALID, "om_hit_rays: null rays/hits");
    return OM_OK;
}

// One query launch: closest-hit into dev_hits, or any-hit into dev_occ (exactly one is non-null).
static om_status launch_query(om_ctx* c, const om_query_params* q, const om_ray* dev_rays, const om_ray_window* dev_windows,
                              uint32_t n, om_hit* dev_hits, uint8_t* dev_occ, void* stream) {
    om_status s = validate_query(c, q, dev_rays, n, dev_hits ? (const void*)dev_hits : (const void*)dev_occ);
    if (s) return s;
    if (n == 0) return OM_OK;
    OM_HIP(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (!c->counters.p) {
        if ((s = ensure(c, c->counters, OMC_SLOTS * sizeof(unsigned long long))) != OM_OK) return s;
        OM_HIP(c, hipMemsetAsync(c->counters.p, 0, OMC_SLOTS * sizeof(unsigned long long), st));
    }
    c->last_stream = st;
    int mode = c->kernel;
    if (mode == OM_KERNEL_AUTO) mode = OM_KERNEL_BVH2;
    omw::Query Q;
    Q.S = c->scene;
    Q.tmin = q->tmin; Q.tmax = q->tmax; Q.march_steps = q->march_steps;
    Q.rays = dev_rays; Q.windows = dev_windows; Q.hits = dev_hits; Q.occluded = dev_occ; Q.n = n;
    Q.counters = (unsigned long long*)c->counters.p;
    Q.count = c->count_work;
    Q.trace_mode = wf_trace_mode(mode);
    const hipError_t e = omw::query(Q, st);
    if (e != hipSuccess) return set_err(c, OM_ERR_DEVICE, std::string("ray query launch: ") + hipGetErrorString(e));
    return OM_OK;
}

// Host form of either query kind: rays (and windows) in through the ctx's staging buffers, the
// records or bytes back out, synchronous.
static om_status host_query(om_ctx* c, const om_query_params* q, const om_ray* rays, const om_ray_window* windows, uint32_t n,
                            om_hit* hits, uint8_t* occ) {
    om_status s = validate_query(c, q, rays, n, hits ? (const void*)hits : (const void*)occ);
    if (s) return s;
    if (n == 0) return OM_OK;
    OM_HIP(c, hipSetDevice(c->device));
    DevBuf& out = hits ? c->query_hits : c->query_occ;
    const size_t out_bytes = (size_t)n * (hits ? sizeof(om_hit) : sizeof(uint8_t));
    if ((s = ensure(c, c->query_rays, (size_t)n * sizeof(om_ray))) != OM_OK) return s;
    if (windows && (s = ensure(c, c->query_windows, (size_t)n * sizeof(om_ray_window))) != OM_OK) return s;
    if ((s = ensure(c, out, out_bytes)) != OM_OK) return s;
    OM_HIP(c, hipMemcpyAsync(c->query_rays.p, rays, (size_t)n * sizeof(om_ray), hipMemcpyHostToDevice, c->stream));
    if (windows)
        OM_HIP(c, hipMemcpyAsync(c->query_windows.p, windows, (size_t)n * sizeof(om_ray_window), hipMemcpyHostToDevice, c->stream));
    s = launch_query(c, q, (const om_ray*)c->query_rays.p, windows ? (const om_ray_window*)c->query_windows.p : nullptr, n,
                     hits ? (om_hit*)out.p : nullptr, hits ? nullptr : (uint8_t*)out.p, c->stream);
    if (s != OM_OK) return s;
    OM_HIP(c, hipMemcpyAsync(hits ? (void*)hits : (void*)occ, out.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
    OM_HIP(c, hipStreamSynchronize(c->stream));
    return OM_OK;
}

om_status om_hit_rays_device(om_ctx* c, const om_query_params* q, const om_ray* dev_rays, uint32_t n, om_hit* dev_hits,
                             void* stream) {
    return launch_query(c, q, dev_rays, nullptr, n, dev_hits, nullptr, stream);
}
om_status om_hit_rays(om_ctx* c, const om_query_params* q, const om_ray* rays, uint32_t n, om_hit* hits) {
    return host_query(c, q, rays, nullptr, n, hits, nullptr);
}
om_status om_hit_rays_windows_device(om_ctx* c, const om_query_params* q, const om_ray* dev_rays, const om_ray_window* dev_windows,
                                     uint32_t n, om_hit* dev_hits, void* stream) {
    return launch_query(c, q, dev_rays, dev_windows, n, dev_hits, nullptr, stream);
}
om_status om_hit_rays_windows(om_ctx* c, const om_query_params* q, const om_ray* rays, const om_ray_window* windows, uint32_t n,
                              om_hit* hits) {
    return host_query(c, q, rays, windows, n, hits, nullptr);
}
om_status om_occluded_rays_device(om_ctx* c, const om_query_params* q, const om_ray* dev_rays, const om_ray_window* dev_windows,
                                  uint32_t n, uint8_t* dev_occluded, void* stream) {
    return launch_query(c, q, dev_rays, dev_windows, n, nullptr, dev_occluded, stream);
}
om_status om_occluded_rays(om_ctx* c, const om_query_params* q, const om_ray* rays, const om_ray_window* windows, uint32_t n,
                           uint8_t* occluded) {
    return host_query(c, q, rays, windows, n, nullptr, occluded);
}

// ---- radiance queries (ray_color, render_thread.rs:128-143) ----
// om-rng v2 on the host: mix64 and the path key as om_device.h / launch() have them
static uint64_t host_mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
uint64_t om_path_rng_state(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t draws) {
    const uint64_t skey = host_mix64(seed + 0x632BE59BD9B4E019ULL);
    const uint64_t z = host_mix64((((uint64_t)pixel << 32) | (uint64_t)sample) ^ skey);
    // a draw adds the Weyl constant to the low word (mod 2^32) and leaves the key
    const uint32_t s = (uint32_t)z + draws * 0x9E3779B9u;
    return (z & 0xFFFFFFFF00000000ULL) | (uint64_t)s;
}

static om_status validate_paths(om_ctx* c, const om_path_params* p, const void* rays, uint32_t n, const void* out) {
    if (!c) return set_err(nullptr, OM_ERR_INVALID, "om_ray_color: null ctx");
    if (!p) return set_err(c, OM_ERR_INVALID, "om_ray_color: null params");
    if (std::isnan(p->tmin) || std::isnan(p->tmax)) return set_err(c, OM_ERR_INVALID, "om_ray_color: tmin/tmax is NaN");
    if (!c->have_world) return set_err(c, OM_ERR_STATE, "om_upload_world must precede radiance queries");
    if (n && (!rays || !out)) return set_err(c, OM_ERR_INVALID, "om_ray_color: null rays/out");
    return OM_OK;
}

om_status om_ray_color_device(om_ctx* c, const om_path_params* p, const om_ray* dev_rays, const uint64_t* dev_rng, uint32_t n,
                              om_radiance* dev_out, void* stream) {
    om_status s = validate_paths(c, p, dev_rays, n, dev_out);
    if (s) return s;
    if (n == 0) return OM_OK;
    if (dev_rng && ((uintptr_t)dev_rng & 7u)) return set_err(c, OM_ERR_INVALID, "om_ray_color: rng must be 8-byte aligned");
    OM_HIP(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (!c->counters.p) {
        if ((s = ensure(c, c->counters, OMC_SLOTS * sizeof(unsigned long long))) != OM_OK) return s;
        OM_HIP(c, hipMemsetAsync(c->counters.p, 0, OMC_SLOTS * sizeof(unsigned long long), st));
    }
    c->last_stream = st;
    int mode = c->kernel;
    if (mode == OM_KERNEL_AUTO) mode = OM_KERNEL_BVH2;
    omw::PathQuery Q{};
    Q.S = c->scene;
    Q.P.tmin = p->tmin; Q.P.tmax = p->tmax; Q.P.march_steps = p->march_steps; Q.P.max_depth = p->max_depth;
    Q.P.skey = host_mix64(p->seed + 0x632BE59BD9B4E019ULL);
    Q.rays = dev_rays; Q.rng = dev_rng; Q.n = n; Q.stream_base = p->stream_base; Q.sample = p->sample; Q.out = dev_out;
    Q.counters = (unsigned long long*)c->counters.p;
    Q.count = c->count_work;
    Q.trace_mode = wf_trace_mode(mode);
    Q.tail_bounce = c->tail_bounce;
    Q.paths_log2 = c->path_batch_log2;
    Q.timer = &c->timer;
    std::string err;
    const hipError_t e = omw::ray_color(c->wf, Q, st, err);
    if (e != hipSuccess) return set_err(c, OM_ERR_DEVICE, err + ": " + hipGetErrorString(e));
    return OM_OK;
}

om_status om_ray_color(om_ctx* c, const om_path_params* p, const om_ray* rays, const uint64_t* rng, uint32_t n, om_radiance* out) {
    om_status s = validate_paths(c, p, rays, n, out);
    if (s) return s;
    if (n == 0) return OM_OK;
    OM_HIP(c, hipSetDevice(c->device));
    if ((s = ensure(c, c->query_rays, (size_t)n * sizeof(om_ray))) != OM_OK) return s;
    if (rng && (s = ensure(c, c->path_rng, (size_t)n * sizeof(uint64_t))) != OM_OK) return s;
    if ((s = ensure(c, c->path_out, (size_t)n * sizeof(om_radiance))) != OM_OK) return s;
    OM_HIP(c, hipMemcpyAsync(c->query_rays.p, rays, (size_t)n * sizeof(om_ray), hipMemcpyHostToDevice, c->stream));
    if (rng) OM_HIP(c, hipMemcpyAsync(c->path_rng.p, rng, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    s = om_ray_color_device(c, p, (const om_ray*)c->query_rays.p, rng ? (const uint64_t*)c->path_rng.p : nullptr, n,
                            (om_radiance*)c->path_out.p, c->stream);
    if (s != OM_OK) return s;
    OM_HIP(c, hipMemcpyAsync(out, c->path_out.p, (size_t)n * sizeof(om_radiance), hipMemcpyDeviceToHost, c->stream));
    OM_HIP(c, hipStreamSynchronize(c->stream));
    return OM_OK;
}

om_status om_set_path_batch(om_ctx* c, uint32_t paths_log2) {
    if (!c) return set_err(nullptr, OM_ERR_INVALID, "null ctx");
    if (paths_log2 != 0u && (paths_log2 < 6u || paths_log2 > (uint32_t)OM_WF_MAX_PATHS_LOG2))
        return set_err(c, OM_ERR_INVALID, "om_set_path_batch: paths_log2 must be 0 or 6..27");
    c->path_batch_log2 = paths_log2;
    return OM_OK;
}

// ---- frames from caller-given rays ----
// The checks both forms share; *work is false for a call that is OM_OK and launches nothing.
static om_status validate_frame_rays(om_ctx* c, const om_render_params* p, const void* rays, const void* pixels, uint32_t n_pixels,
                                     const void* stats, bool* work) {
    *work = false;
    if (!c) return set_err(nullptr, OM_ERR_INVALID, "om_render_rays: null ctx");
    if (!p) return set_err(c, OM_ERR_INVALID, "om_render_rays: null params");
    if (p->width == 0 || p->height == 0) return set_err(c, OM_ERR_INVALID, "width/height must be > 0");
    const uint64_t frame = (uint64_t)p->width * p->height;
    if (frame > (1ull << 31)) return set_err(c, OM_ERR_INVALID, "image too large");
    if (!pixels && n_pixels != frame) return set_err(c, OM_ERR_INVALID, "om_render_rays: without a pixel list n_pixels is width * height");
    if (n_pixels > frame) return set_err(c, OM_ERR_INVALID, "om_render_rays: more listed pixels than the frame has");
    if (std::isnan(p->tmin) || std::isnan(p->tmax)) return set_err(c, OM_ERR_INVALID, "om_render_rays: tmin/tmax is NaN");
    if (!c->have_world) return set_err(c, OM_ERR_STATE, "om_upload_world must precede rendering");
    if (p->sample_count == 0 || p->spp_total == 0 || n_pixels == 0) return OM_OK;
    if (!rays || !stats) return set_err(c, OM_ERR_INVALID, "om_render_rays: null rays/stats");
    *work = true;
    return OM_OK;
}

om_status om_render_rays_device(om_ctx* c, const om_render_params* p, const om_ray* dev_rays, const uint64_t* dev_rng,
                                const uint32_t* dev_pixels, uint32_t n_pixels, om_pixel_stats* dev_stats, void* stream) {
    bool work;
    om_status s = validate_frame_rays(c, p, dev_rays, dev_pixels, n_pixels, dev_stats, &work);
    if (s || !work) return s;
    if (dev_rng && ((uintptr_t)dev_rng & 7u)) return set_err(c, OM_ERR_INVALID, "om_render_rays: rng must be 8-byte aligned");
    OM_HIP(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (!c->counters.p) {
        if ((s = ensure(c, c->counters, OMC_SLOTS * sizeof(unsigned long long))) != OM_OK) return s;
        OM_HIP(c, hipMemsetAsync(c->counters.p, 0, OMC_SLOTS * sizeof(unsigned long long), st));
    }
    c->last_stream = st;
    int mode = c->kernel;
    if (mode == OM_KERNEL_AUTO) mode = OM_KERNEL_BVH2;
    omw::FrameRays Q{};
    Q.S = c->scene;
    OmParamsDev& P = Q.P;
    P.width = p->width; P.height = p->height; P.spp_total = p->spp_total; P.sample_count = p->sample_count;
    P.max_depth = p->max_depth; P.march_steps = p->march_steps; P.adaptive = p->adaptive ? 1u : 0u;
    P.tmin = p->tmin; P.tmax = p->tmax;
    P.skey = host_mix64(p->seed + 0x632BE59BD9B4E019ULL);
    P.progress = c->progress_host ? 1u : 0u;
    P.n_pixels = n_pixels;
    Q.rays = dev_rays; Q.rng = dev_rng; Q.pixels = dev_pixels; Q.n_pixels = n_pixels; Q.stats = dev_stats;
    Q.counters = (unsigned long long*)c->counters.p;
    Q.count = c->count_work;
    Q.trace_mode = wf_trace_mode(mode);
    Q.tail_bounce = c->tail_bounce;
    Q.paths_log2 = c->path_batch_log2;
    Q.timer = &c->timer;
    Q.progress_host = c->progress_host;
    std::string err;
    const hipError_t e = omw::render_rays(c->wf, Q, st, err);
    if (e != hipSuccess) return set_err(c, OM_ERR_DEVICE, err + ": " + hipGetErrorString(e));
    return OM_OK;
}

om_status om_render_rays(om_ctx* c, const om_render_params* p, const om_ray* rays, const uint64_t* rng, const uint32_t* pixels,
                         uint32_t n_pixels, om_pixel_stats* stats, om_counters* counters) {
    bool work;
    om_status s = validate_frame_rays(c, p, rays, pixels, n_pixels, stats, &work);
    if (s) return s;
    const uint32_t frame = p->width * p->height;
    if (work && pixels)
        for (uint32_t k = 0; k < n_pixels; ++k)
            if (pixels[k] >= frame) return set_err(c, OM_ERR_INVALID, "om_render_rays: a listed pixel is outside the frame");
    OM_HIP(c, hipSetDevice(c->device));
    if ((s = om_reset_counters(c, c->stream)) != OM_OK) return s;
    if (work) {
        const size_t n = (size_t)p->sample_count * n_pixels, bytes = (size_t)frame * sizeof(om_pixel_stats);
        if ((s = ensure(c, c->query_rays, n * sizeof(om_ray))) != OM_OK) return s;
        if (rng && (s = ensure(c, c->path_rng, n * sizeof(uint64_t))) != OM_OK) return s;
        if (pixels && (s = ensure(c, c->pixels, (size_t)n_pixels * sizeof(uint32_t))) != OM_OK) return s;
        if ((s = ensure(c, c->stats, bytes)) != OM_OK) return s;
        OM_HIP(c, hipMemcpyAsync(c->query_rays.p, rays, n * sizeof(om_ray), hipMemcpyHostToDevice, c->stream));
        if (rng) OM_HIP(c, hipMemcpyAsync(c->path_rng.p, rng, n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        if (pixels) OM_HIP(c, hipMemcpyAsync(c->pixels.p, pixels, (size_t)n_pixels * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        OM_HIP(c, hipMemcpyAsync(c->stats.p, stats, bytes, hipMemcpyHostToDevice, c->stream));
        s = om_render_rays_device(c, p, (const om_ray*)c->query_rays.p, rng ? (const uint64_t*)c->path_rng.p : nullptr,
                                  pixels ? (const uint32_t*)c->pixels.p : nullptr, n_pixels, (om_pixel_stats*)c->stats.p, c->stream);
        if (s != OM_OK) return s;
        OM_HIP(c, hipMemcpyAsync(stats, c->stats.p, bytes, hipMemcpyDeviceToHost, c->stream));
        OM_HIP(c, hipStreamSynchronize(c->stream));
    }
    if (counters) return om_get_counters(c, counters);
    return OM_OK;
}

uint32_t om_query_max_grid(om_ctx* c) {
    if (!c) { set_err(nullptr, OM_ERR_INVALID, "om_query_max_grid: null ctx"); return 0u; }
    if (hipSetDevice(c->device) != hipSuccess) { set_err(c, OM_ERR_DEVICE, "om_query_max_grid: hipSetDevice"); return 0u; }
    return omw::query_max_grid();
}

om_status om_host_register(void* p, size_t bytes) {
    if (!p || !bytes) return set_err(nullptr, OM_ERR_INVALID, "om_host_register: null/empty buffer");
    const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterDefault);
    if (e != hipSuccess) return set_err(nullptr, OM_ERR_DEVICE, std::string("om_host_register: ") + hipGetErrorString(e));
    return OM_OK;
}

om_status om_host_unregister(void* p) {
    if (!p) return set_err(nullptr, OM_ERR_INVALID, "om_host_unregister: null buffer");
    const hipError_t e = hipHostUnregister(p);
    if (e != hipSuccess) return set_err(nullptr, OM_ERR_DEVICE, std::string("om_host_unregister: ") + hipGetErrorString(e));
    return OM_OK;
}

om_status om_get_counters(om_ctx* c, om_counters* out) {
    if (!c || !out) return set_err(c, OM_ERR_INVALID, "null pointer");
    std::memset(out, 0, sizeof(*out));
    if (!c->counters.p) return OM_OK;
    OM_HIP(c, hipSetDevice(c->device));
    unsigned long long h[OMC_N];
    OM_HIP(c, hipStreamSynchronize(c->stream));
    if (c->last_stream && c->last_stream != c->stream) OM_HIP(c, hipStreamSynchronize(c->last_stream));
    OM_HIP(c, hipMemcpy(h, c->counters.p, sizeof(h), hipMemcpyDeviceToHost));
    out->samples = h[OMC_SAMPLES]; out->segments = h[OMC_SEGMENTS]; out->prim_tests = h[OMC_PRIM_TESTS];
    out->pre_tests = h[OMC_PRE_TESTS]; out->march_steps = h[OMC_MARCH]; out->credited = h[OMC_CREDITED];
    return OM_OK;
}

om_status om_set_pipeline(om_ctx* c, int32_t pipeline) {
    if (!c) return set_err(nullptr, OM_ERR_INVALID, "null ctx");
    if (pipeline != OM_PIPELINE_MEGAKERNEL && pipeline != OM_PIPELINE_WAVEFRONT && pipeline != OM_PIPELINE_AUTO)
        return set_err(c, OM_ERR_INVALID, "om_set_pipeline: unknown pipeline");
    c->pipeline = pipeline;
    return OM_OK;
}

om_status om_set_primary_lists(om_ctx* c, int32_t mode) {
    if (!c) return set_err(nullptr, OM_ERR_INVALID, "null ctx");
    if (mode < OM_PRIMARY_LISTS_OFF || mode > OM_PRIMARY_LISTS_ON)
        return set_err(c, OM_ERR_INVALID, "om_set_primary_lists: unknown mode");
    c->primary_lists = mode;
    return OM_OK;
}

om_status om_set_tail_bounce(om_ctx* c, uint32_t bounce) {
    if (!c) return set_err(nullptr, OM_ERR_INVALID, "null ctx");
    c->tail_bounce = bounce;
    return OM_OK;
}

om_status om_set_streams(om_ctx* c, uint32_t streams) {
    if (!c) return set_err(nullptr, OM_ERR_INVALID, "null ctx");
    if (streams < 1 || streams > (uint32_t)omw::kMaxSets) return set_err(c, OM_ERR_INVALID, "om_set_streams: streams must be 1..4");
    c->wf_streams = streams;
    return OM_OK;
}

om_status om_set_adaptive_batches(om_ctx* c, uint32_t batches, uint32_t paths_log2) {
    if (!c) return set_err(nullptr, OM_ERR_INVALID, "null ctx");
    // every planned batch is launched whether or not the device plan leaves it any pixel (the host
    // never reads the live count back): ~10 launches of ~5 us each per empty batch and stream, so
    // the knob is capped at a few dozen batches
    if (batches > 64u || paths_log2 > 27u)
        return set_err(c, OM_ERR_INVALID, "om_set_adaptive_batches: batches <= 64, paths_log2 <= 27");
    c->ad_batches = batches; c->ad_paths_log2 = paths_log2;
    return OM_OK;
}

om_status om_set_timing(om_ctx* c, int32_t mode) {
    if (!c) return set_err(nullptr, OM_ERR_INVALID, "null ctx");
    if (mode < 0 || mode > 2) return set_err(c, OM_ERR_INVALID, "om_set_timing: mode must be 0, 1 or 2");
    OM_HIP(c, hipSetDevice(c->device));
    for (size_t i = 0; c->timer.on() && i < c->timer.cls.size(); ++i)
        if (c->timer.cls[i] >= 0) OM_HIP(c, hipEventSynchronize(c->timer.ev[2 * i + 1]));
    c->timer.mode = mode;
    c->timer.clear();
    return OM_OK;
}

om_status om_get_kernel_times(om_ctx* c, om_kernel_times* out) {
    if (!c || !out) return set_err(c, OM_ERR_INVALID, "om_get_kernel_times: null argument");
    OM_HIP(c, hipSetDevice(c->device));
    *out = om_kernel_times{};
    omw::Timer& t = c->timer;
    for (size_t i = 0; i < t.cls.size(); ++i) {
        if (t.cls[i] < 0) continue;
        OM_HIP(c, hipEventSynchronize(t.ev[2 * i + 1]));
        float ms = 0.0f;
        OM_HIP(c, hipEventElapsedTime(&ms, t.ev[2 * i], t.ev[2 * i + 1]));
        out->launches[t.cls[i]] += t.nl[i];
        out->ms[t.cls[i]] += (double)ms;
    }
    t.clear();
    return OM_OK;
}

om_status om_display_device(om_ctx* c, const om_pixel_stats* dev_stats, uint32_t width, uint32_t height, int32_t view,
                            uint8_t* dev_rgb, void* stream) {
    if (!c || !dev_stats || !dev_rgb) return set_err(c, OM_ERR_INVALID, "om_display_device: null argument");
    if (view < OM_VIEW_NORMAL || view > OM_VIEW_ID_BLUR) return set_err(c, OM_ERR_INVALID, "om_display_device: unknown view");
    if (width == 0 || height == 0 || (uint64_t)width * height > 0xFFFFFFFFull / 3u)
        return set_err(c, OM_ERR_INVALID, "om_display_device: bad frame size");
    const bool blur = view == OM_VIEW_SAMPLE_BLUR || view == OM_VIEW_DEPTH_BLUR || view == OM_VIEW_ID_BLUR;
    if (blur && (width < 2 || height < 2))   // apply_box_filter indexes a 2x2 corner neighbourhood
        return set_err(c, OM_ERR_INVALID, "om_display_device: blur views need width, height >= 2");
    OM_HIP(c, hipSetDevice(c->device));
    om_status s = ensure(c, c->view_scratch, omv::scratch_bytes(width, height));
    if (s != OM_OK) return s;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    const hipError_t e = omv::render(dev_stats, width, height, view, dev_rgb, c->view_scratch.p, st);
    if (e != hipSuccess) return set_err(c, OM_ERR_DEVICE, std::string("om_display_device: ") + hipGetErrorString(e));
    c->last_stream = st;
    return OM_OK;
}

om_status om_display(om_ctx* c, const om_pixel_stats* stats, uint32_t width, uint32_t height, int32_t view, uint8_t* rgb) {
    if (!c || !stats || !rgb) return set_err(c, OM_ERR_INVALID, "om_display: null argument");
    if (width == 0 || height == 0 || (uint64_t)width * height > 0xFFFFFFFFull / 3u)
        return set_err(c, OM_ERR_INVALID, "om_display: bad frame size");
    OM_HIP(c, hipSetDevice(c->device));
    const size_t npx = (size_t)width * height;
    om_status s = ensure(c, c->stats, npx * sizeof(om_pixel_stats));
    if (s != OM_OK) return s;
    if ((s = ensure(c, c->view_rgb, npx * 3)) != OM_OK) return s;
    OM_HIP(c, hipMemcpyAsync(c->stats.p, stats, npx * sizeof(om_pixel_stats), hipMemcpyHostToDevice, c->stream));
    OM_HIP(c, hipMemcpyAsync(c->view_rgb.p, rgb, npx * 3, hipMemcpyHostToDevice, c->stream));
    if ((s = om_display_device(c, (const om_pixel_stats*)c->stats.p, width, height, view, (uint8_t*)c->view_rgb.p, c->stream)) != OM_OK)
        return s;
    OM_HIP(c, hipMemcpyAsync(rgb, c->view_rgb.p, npx * 3, hipMemcpyDeviceToHost, c->stream));
    OM_HIP(c, hipStreamSynchronize(c->stream));
    return OM_OK;
}

const volatile uint64_t* om_progress(om_ctx* c) {
    if (!c) { set_err(nullptr, OM_ERR_INVALID, "om_progress: null ctx"); return nullptr; }
    if (c->progress_host) return (const volatile uint64_t*)c->progress_host;
    if (hipSetDevice(c->device) != hipSuccess) { set_err(c, OM_ERR_DEVICE, "om_progress: hipSetDevice"); return nullptr; }
    if (!c->counters.p) {
        if (ensure(c, c->counters, OMC_SLOTS * sizeof(unsigned long long)) != OM_OK) return nullptr;
        if (hipMemset(c->counters.p, 0, OMC_SLOTS * sizeof(unsigned long long)) != hipSuccess) {
            set_err(c, OM_ERR_DEVICE, "om_progress: hipMemset");
            return nullptr;
        }
    }
    unsigned long long* h = nullptr;
    if (hipHostMalloc((void**)&h, sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess) {
        set_err(c, OM_ERR_NOMEM, "om_progress: hipHostMalloc");
        return nullptr;
    }
    *h = 0;
    if (hipStreamSynchronize(c->stream) != hipSuccess ||
        hipMemcpy(h, (unsigned long long*)c->counters.p + OMC_PROGRESS, sizeof(*h), hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipHostFree(h);
        set_err(c, OM_ERR_DEVICE, "om_progress: reading the device word");
        return nullptr;
    }
    c->progress_host = h;
    return (const volatile uint64_t*)h;
}

om_status om_reset_progress(om_ctx* c) {
    if (!c) return set_err(nullptr, OM_ERR_INVALID, "null ctx");
    if (!c->progress_host) return OM_OK;
    OM_HIP(c, hipSetDevice(c->device));
    OM_HIP(c, hipDeviceSynchronize());
    OM_HIP(c, hipMemset((unsigned long long*)c->counters.p + OMC_PROGRESS, 0, sizeof(unsigned long long)));
    *(volatile unsigned long long*)c->progress_host = 0;
    return OM_OK;
}

om_status om_set_counting(om_ctx* c, int32_t enable) {
    if (!c) return set_err(nullptr, OM_ERR_INVALID, "null ctx");
    c->count_work = enable != 0;
    return OM_OK;
}

om_status om_reset_counters(om_ctx* c, void* stream) {
    if (!c) return set_err(nullptr, OM_ERR_INVALID, "null ctx");
    OM_HIP(c, hipSetDevice(c->device));
    const bool fresh = !c->counters.p;
    om_status s = ensure(c, c->counters, OMC_SLOTS * sizeof(unsigned long long));
    if (s) return s;
    // the counters only; the progress word after them keeps counting (om_reset_progress)
    OM_HIP(c, hipMemsetAsync(c->counters.p, 0, (fresh ? OMC_SLOTS : OMC_N) * sizeof(unsigned long long),
                             stream ? (hipStream_t)stream : c->stream));
    return OM_OK;
}

}  // extern "C"

namespace omi {
int ctx_device(const om_ctx* c) { return c->device; }
hipStream_t ctx_stream(const om_ctx* c) { return c->stream; }
om_status ctx_error(om_ctx* c, om_status code, const std::string& msg) { return set_err(c, code, msg); }
om_status global_error(om_status code, const std::string& msg) { return set_err(nullptr, code, msg); }
}  // namespace omi
