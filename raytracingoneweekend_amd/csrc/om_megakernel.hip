// om_megakernel.hip — the megakernel pipeline (OM_PIPELINE_MEGAKERNEL): ray_color
// (render_thread.rs:105-202) as one persistent-path kernel.  One lane owns one pixel for the whole call
// and walks its samples in order (Stats::add in the reference's order, bit for bit); the bounce
// recursion is a segment loop with path REGENERATION: a lane whose path ends starts the pixel's next
// sample in the same iteration.  A wave owns an 8x8 tile.  Traversals, HitRecord and counter flush are
// om_trace.h's, shared with the wavefront.  MODE is a TR_* value (om_layout.h): TR_BVH2_LDS
// also reads a tree past the LDS budget through L2; a tree past the 15-bit codes and OM_KERNEL_BVH2W
// run TR_BVH (the wide BVH2, DESIGN.md §5.18, is the wavefront's).
#include <hip/hip_runtime.h>

#include "om_device.h"
#include "om_trace.h"
#include "om_wavefront.h"

using namespace omd;

namespace {

constexpr int kBlock = 256;
constexpr int kBlockLds = 512;                 // the SBVH variants' workgroup
constexpr int kStack2 = (int)kB2Stack;         // BVH2 lane-stack bound (om::plan_trees checks the depth)
template <int MODE> constexpr int block_of() { return MODE == TR_SBVH_LDS || MODE == TR_SBVH_GLOBAL ? kBlockLds : kBlock; }
// the variants whose leaves may hold triangles / parallelograms: the only ones with BARY instantiations
template <int MODE> constexpr bool bary_built() { return MODE == TR_SBVH_LDS || MODE == TR_SBVH_GLOBAL || MODE == TR_BVH2_LDS; }

extern __shared__ __attribute__((aligned(16))) uint4 om_lds[];

// MARCH is a compile-time split (as in the wavefront): traced-only scenes do not carry
// the sphere-tracing code's registers.  BARY likewise (SBVH / BVH2 modes): worlds whose leaves
// hold triangles / parallelograms run the leaf test with the barycentric case.
template <int MODE, int BLOCK, bool COUNT, bool MARCH, bool BARY = false>
__global__ __launch_bounds__(BLOCK, (BLOCK >= 512 ? 4 : 1)) void render_kernel(OmSceneDev S, OmCamDev C, OmParamsDev P,
                                                       const float2* __restrict__ jitter,
                                                       om_pixel_stats* __restrict__ stats,
                                                       const uint32_t* __restrict__ pixel_list,
                                                       unsigned long long* __restrict__ counters) {
    if (MODE == TR_SBVH_LDS) {
        // stage the stackless BVH + its records once per workgroup (uint4 chunks)
        const uint32_t nn = S.n_snodes * 2u, nr = S.n_srecs * 4u;
        const uint4* sn = (const uint4*)S.snodes;
        const uint4* sr = (const uint4*)S.srecs;
        for (uint32_t i = threadIdx.x; i < nn; i += BLOCK) om_lds[i] = sn[i];
        for (uint32_t i = threadIdx.x; i < nr; i += BLOCK) om_lds[nn + i] = sr[i];
        __syncthreads();
    }
    const OmSkipNode* lds_nodes = (const OmSkipNode*)om_lds;
    const OmAffineTest* lds_recs = (const OmAffineTest*)(om_lds + S.n_snodes * 2u);
    // BVH2: [lane stack][nodes][leaf table] in LDS (nodes through L2 when they exceed the budget)
    uint16_t* b2_stk = (uint16_t*)om_lds + threadIdx.x;
    const OmBvh2Node* b2_nodes = S.b2nodes;
    const uint32_t* b2_leaves = S.b2leaves;
    if (MODE == TR_BVH2_LDS && S.b2_lds_bytes) {
        uint4* dst = om_lds + (BLOCK * S.b2_stack * 2u) / 16u;
        const uint32_t nn = S.n_b2nodes * (uint32_t)(sizeof(OmBvh2Node) / 16u);
        const uint4* sn = (const uint4*)S.b2nodes;
        for (uint32_t i = threadIdx.x; i < nn; i += BLOCK) dst[i] = sn[i];
        uint32_t* ldst = (uint32_t*)(dst + nn);
        for (uint32_t i = threadIdx.x; i < S.n_b2leaves; i += BLOCK) ldst[i] = S.b2leaves[i];
        __syncthreads();
        b2_nodes = (const OmBvh2Node*)dst;
        b2_leaves = ldst;
    }
    const uint32_t tid = blockIdx.x * BLOCK + threadIdx.x;
    uint32_t pixel, slot;
    bool valid;
    if (pixel_list) {
        valid = tid < P.n_pixels;
        pixel = valid ? pixel_list[tid] : 0u;
        slot = tid;
    } else {
        const uint32_t wave = tid >> 6, lane = tid & 63u;
        const uint32_t tx = wave % P.tiles_x, ty = wave / P.tiles_x;
        const uint32_t px = tx * 8u + (lane & 7u), py = ty * 8u + (lane >> 3);
        valid = px < P.width && py < P.height;
        pixel = py * P.width + px;
        slot = pixel;
    }
    PixelState st;
    if (valid) {
        const om_pixel_stats in = stats[slot];
        st.bloom = in.bloom; st.sx = in.sum[0]; st.sy = in.sum[1]; st.sz = in.sum[2]; st.n = in.n;
        st.avg_depth = in.avg_depth; st.bad = in.bad_avgs;
        st.rgbf = (uint32_t)in.color[0] | ((uint32_t)in.color[1] << 8) | ((uint32_t)in.color[2] << 16) | ((uint32_t)in.flags << 24);
    } else {
        st.bloom = 0; st.sx = st.sy = st.sz = 0.0f; st.n = 0; st.avg_depth = 0.0f; st.bad = 0; st.rgbf = 0;
    }
    const uint32_t line = valid ? pixel / P.width : 0u;
    const float j_f = (float)line, i_f = (float)(pixel - P.width * line);
    const uint32_t cap = depth_cap(P);

    uint32_t todo = valid ? P.sample_count : 0u;
    bool live = false;
    F3 o = f3(0, 0, 0), d = f3(0, 0, 0), cur = f3(1, 1, 1);
    Rng g; g.s = 0; g.k = 0;
    uint32_t seg = 0, first_id = 0;
    float depthf = 0.0f;
    WorkT<COUNT, false, BARY> w;
    uint32_t n_samples = 0, n_segments = 0, credited = 0;

    for (;;) {
        if (!live && todo > 0u) {
            if ((P.adaptive && (st.rgbf & 0x01000000u)) || st.n >= P.spp_total) {
                todo = 0u;
            } else {
                // render_thread.rs:183-192 + Camera::get_ray camera.rs:60-65 (gen_camera_ray written out, like
                // the shading below: the shared function cost this kernel 0.7 % on C1, bench.txt)
                const uint32_t s = st.n;
                g = path_rng(P.skey, pixel, s);
                const float2 jt = jitter[s];
                const float i_rand = (g.next() + jt.x) / 2.0f;
                const float j_rand = (g.next() + jt.y) / 2.0f;
                const float u = (i_f + i_rand) / P.wf_m1;
                const float v = 1.0f - (j_f + j_rand) / P.hf_m1;
                float dx, dy;
                for (;;) {                                                     // rand_in_unit_disc vec3.rs:108-113
                    dx = g.range(-1.0f, 1.0f);
                    dy = g.range(-1.0f, 1.0f);
                    if (dx * dx + dy * dy < 1.0f) break;
                }
                const float rlx = dx * C.lens_radius, rly = dy * C.lens_radius;
                const F3 off = f3(C.u[0] * rlx + C.v[0] * rly, C.u[1] * rlx + C.v[1] * rly, C.u[2] * rlx + C.v[2] * rly);
                // uv_to_dir . (u, v, 0, 1): ((H*u + V*v) + 0*0) + D*1
                const F3 dir = f3((C.horizontal[0] * u + C.vertical[0] * v) + 0.0f * 0.0f + C.llc_minus_origin[0],
                                  (C.horizontal[1] * u + C.vertical[1] * v) + 0.0f * 0.0f + C.llc_minus_origin[1],
                                  (C.horizontal[2] * u + C.vertical[2] * v) + 0.0f * 0.0f + C.llc_minus_origin[2]);
                o = add(ld3(C.origin), off);
                d = unit(unit(sub(dir, off)));                                 // camera.rs:64 + ray.rs:12
                cur = f3(1.0f, 1.0f, 1.0f);
                seg = 0; live = true; todo--;
            }
        }
        if (__ballot(live) == 0ull) break;
        if (!live) continue;

        // ---- one segment: handle_hit(world.hit(ray)) render_thread.rs:105-126
        if (COUNT) n_segments++;
        float closest = P.tmax;
        int best;
        if (MODE == TR_SBVH_LDS) best = traced_sbvh(S, lds_nodes, lds_recs, o, d, P.tmin, closest, w);
        else if (MODE == TR_SBVH_GLOBAL) best = traced_sbvh(S, S.snodes, S.srecs, o, d, P.tmin, closest, w);
        else if (MODE == TR_BVH) best = traced_bvh(S, o, d, P.tmin, closest, w);
        else if (MODE == TR_BVH2_LDS) best = traced_bvh2<kStack2, BLOCK>(S, b2_nodes, b2_leaves, S.srecs, b2_stk, o, d, P.tmin, closest, w);
        else best = traced_brute<MODE == TR_CULLED>(S, o, d, P.tmin, closest, w);
        if (MARCH) {
            float tm;
            const int mg = march(S, o, d, P.tmin, P.tmax, closest, P.march_steps, tm, w);
            if (mg >= 0) { best = mg; closest = tm; }
        }
        // (the wavefront's shade_path, written out: as a shared function it cost this kernel 1.5-3 % on
        // C1 at equal registers, profiles/one_integrator/bench.txt)
        float seg_depth; uint32_t seg_id;
        if (best >= 0) {
            F3 point, normal;
            finalize<MARCH>(S, best, o, d, P.tmin, closest, point, normal);
            F3 nd, att;
            scatter(S.mats[best], d, normal, g, nd, att);
            cur = mul(cur, att);
            o = point; d = unit(nd);
            seg_depth = closest; seg_id = (uint32_t)best + 1u;
        } else {
            const float t = 0.5f * (d.y + 1.0f);                               // render_thread.rs:118-120
            cur = mul(cur, f3((1.0f - t) + 0.5f * t, (1.0f - t) + 0.7f * t, (1.0f - t) + 1.0f * t));
            seg_depth = INFINITY; seg_id = 0u;
        }
        bool finished = false;
        F3 result = cur;
        float rdepth = 0.0f; uint32_t rid = 0;
        if (seg == 0u) {
            depthf = seg_depth; first_id = seg_id;
            if (isinf(seg_depth)) { finished = true; rdepth = INFINITY; rid = 0u; }     // :133-135
        } else if (isinf(seg_depth)) {
            finished = true; rdepth = depthf; rid = first_id;                       // :138-140
        }
        if (!finished && seg + 1u >= cap) {                              // :142  -Color::ZERO
            finished = true; result = f3(-0.0f, -0.0f, -0.0f); rdepth = depthf; rid = first_id;
        }
        seg++;
        if (finished) {
            const bool done = stats_add(st, result, rdepth, S.bloom[rid]);
            if (COUNT) n_samples++;
            credited += ((done && P.adaptive) ? (P.spp_total - st.n) : 0u) + 1u;     // :196-198
            live = false;
        }
    }

    if (valid) {
        om_pixel_stats out;
        out.bloom = st.bloom; out.sum[0] = st.sx; out.sum[1] = st.sy; out.sum[2] = st.sz; out.n = st.n;
        out.avg_depth = st.avg_depth; out.bad_avgs = st.bad;
        out.color[0] = (uint8_t)(st.rgbf & 0xFFu); out.color[1] = (uint8_t)((st.rgbf >> 8) & 0xFFu);
        out.color[2] = (uint8_t)((st.rgbf >> 16) & 0xFFu); out.flags = (uint8_t)(st.rgbf >> 24); out.reserved = 0u;
        stats[slot] = out;
    }
    // (the wave's first lane from threadIdx.x, live anyway: __lane_id() in the progress add, which every
    // instantiation carries, moved the VGPR count of 31 of the 36 and cost <TR_BVH2_LDS, 256, false, true> a wave)
    const bool first = (threadIdx.x & 63u) == 0u;
    if (COUNT) {
        flush_counter(counters, OMC_SAMPLES, n_samples, first);
        flush_counter(counters, OMC_SEGMENTS, n_segments, first);
        flush_counter(counters, OMC_PRIM_TESTS, w.prim, first);
        flush_counter(counters, OMC_PRE_TESTS, w.pre, first);
        flush_counter(counters, OMC_MARCH, w.march, first);
        flush_counter(counters, OMC_CREDITED, credited, first);
    }
    if (P.progress) flush_counter(counters, OMC_PROGRESS, credited, first);      // live samples_atom (om_progress)
}

// The variant of a ctx's kernel choice (Launch::trace_mode) for the uploaded world.
int pick_mode(int trace_mode, const OmSceneDev& S) {
    if (trace_mode == TR_SBVH_LDS) return S.lds_bytes ? TR_SBVH_LDS : TR_SBVH_GLOBAL;
    if (trace_mode == TR_BRUTE || trace_mode == TR_CULLED) return trace_mode;
    if (trace_mode == TR_BVH2_LDS || trace_mode == TR_BVH4_LDS) {
        if (S.n_b2nodes) return TR_BVH2_LDS;
        // empty BVH2 and at most one leaf in the old BVH (marched-only worlds): the reference
        // loop, without TR_BVH's scratch-memory stack
        if (S.n_bvh_nodes <= 1u) return TR_BRUTE;
    }
    return TR_BVH;
}

template <int MODE>
void go(const omw::Launch& L, hipStream_t stream) {
    constexpr int BLOCK = block_of<MODE>();
    const uint64_t threads = L.pixels ? L.n_pixels : (uint64_t)L.P.tiles_x * ((L.P.height + 7u) / 8u) * 64u;
    const uint32_t blocks = (uint32_t)((threads + BLOCK - 1) / BLOCK);
    const uint32_t lds = MODE == TR_SBVH_LDS ? L.S.lds_bytes : MODE == TR_BVH2_LDS ? BLOCK * L.S.b2_stack * 2u + L.S.b2_lds_bytes : 0u;
    omw::with_flags({L.count, has_marched(L.S), bary_built<MODE>() && L.S.n_srec_bary != 0u}, [&](auto count, auto march, auto bary) {
        if constexpr (!bary || bary_built<MODE>())
            hipLaunchKernelGGL((render_kernel<MODE, BLOCK, count, march, bary>), dim3(blocks), dim3(BLOCK), lds, stream, L.S, L.C,
                               L.P, L.jitter, L.stats, L.pixels, L.counters);
    });
}

}  // namespace

namespace omw {

hipError_t render_megakernel(const Launch& L, hipStream_t stream, std::string& err) {
    const int ti = L.timer->begin(stream);
    switch (pick_mode(L.trace_mode, L.S)) {
        case TR_SBVH_LDS: go<TR_SBVH_LDS>(L, stream); break;
        case TR_SBVH_GLOBAL: go<TR_SBVH_GLOBAL>(L, stream); break;
        case TR_BRUTE: go<TR_BRUTE>(L, stream); break;
        case TR_CULLED: go<TR_CULLED>(L, stream); break;
        case TR_BVH2_LDS: go<TR_BVH2_LDS>(L, stream); break;
        default: go<TR_BVH>(L, stream); break;
    }
    L.timer->end(ti, OM_KT_MEGAKERNEL, stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { err = "megakernel launch failed"; return e; }
    if (L.progress_host) {   // one launch per call: the word advances when it ends
        e = hipMemcpyAsync(L.progress_host, L.counters + OMC_PROGRESS, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream);
        if (e != hipSuccess) err = "megakernel progress copy failed";
    }
    return e;
}

}  // namespace omw
