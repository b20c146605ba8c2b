// om_refit.hip — om_update_triangles on the device: the records and boxes of the
// moved triangles, every internal box bottom-up, the planes of every layout.  Each kernel is one
// thread per element over the OM_HD functions of om_refit.h, which the host builder calls too; all
// writes are ordinary stores, and a level only reads what an earlier launch wrote (stream order is
// the only ordering: no workgroup waits for another).
#include "om_refit_dev.h"

using namespace om;

namespace omr {
namespace {

constexpr uint32_t kBlock = 256u;
inline uint32_t grid_of(uint32_t n) { return (n + kBlock - 1u) / kBlock; }

// step 1: triangle first + k from its three vertices.  An index outside the vertex array leaves the
// triangle as it was (skipped); a non-finite record or box is counted as unbounded.
__global__ void __launch_bounds__(kBlock)
k_triangles(OmBary* tri, float* prim_box, uint32_t* titems, const uint32_t* tri_rec, uint32_t tri_first, uint32_t covering,
            uint32_t first, const float* vertices, uint32_t n_vertices, const uint32_t* indices, uint32_t n_tri, uint32_t* info) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_tri) return;
    uint32_t i0 = 3u * k, i1 = 3u * k + 1u, i2 = 3u * k + 2u;
    if (indices) { i0 = indices[3u * (size_t)k]; i1 = indices[3u * (size_t)k + 1u]; i2 = indices[3u * (size_t)k + 2u]; }
    if (i0 >= n_vertices || i1 >= n_vertices || i2 >= n_vertices) { atomicAdd(info + kInfoSkipped, 1u); return; }
    const uint32_t t = first + k, gi = tri_first + t;
    OmBary rec;
    float planes[6];
    const int ok = refit_triangle(vertices + 3u * (size_t)i0, vertices + 3u * (size_t)i1, vertices + 3u * (size_t)i2, rec, planes);
    tri[t] = rec;
    float* pb = prim_box + 6u * (size_t)gi;
    float old[6], now[6];
    for (int i = 0; i < 6; ++i) old[i] = pb[i];
    refit_triangle_box(ok, planes, old, now);
    for (int i = 0; i < 6; ++i) pb[i] = now[i];
    const uint32_t r = tri_rec[t];
    if (r != kRefitNoNode) titems[r] = refit_triangle_item(ok, gi, covering);
    if (ok != (kRefitRecOk | kRefitBoxOk)) atomicAdd(info + kInfoUnbounded, 1u);
}

// step 2: the leaves of a topology, then its internal nodes one level per launch, deepest first
__global__ void __launch_bounds__(kBlock)
k_leaves(OmBvhNode* nodes, uint32_t n, const uint32_t* items, const float* prim_box) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    OmBvhNode nd = nodes[i];
    if (nd.left >= 0) return;
    refit_leaf(nd, items, prim_box);
    nodes[i] = nd;
}
__global__ void __launch_bounds__(kBlock)
k_level(OmBvhNode* nodes, const uint32_t* level, uint32_t n) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) refit_internal(nodes, level[i]);
}

// step 3: the planes of each layout from the leaf-record tree's boxes
__global__ void __launch_bounds__(kBlock)
k_planes_skip(OmSkipNode* snodes, const uint32_t* src, uint32_t n, const OmBvhNode* tnodes) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float b[6];
    slot_box(tnodes, src[i], b);
    planes_skip(snodes[i], b);
}
// one thread per child box of the BVH2: the f32 node, the half node and the wide node, whichever the device holds
__global__ void __launch_bounds__(kBlock)
k_planes_b2(OmBvh2Node* b2, OmBvh2NodeH* b2h, OmBvh2NodeW* b2w, uint32_t n_b2, uint32_t n_b2h, uint32_t n_b2w,
            const uint32_t* src, uint32_t n_src, const OmBvhNode* tnodes) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_src) return;
    const uint32_t n = i >> 1;
    const int k = (int)(i & 1u);
    float b[6];
    slot_box(tnodes, src[i], b);
    if (n < n_b2) planes_b2(b2[n], k, b);
    if (n < n_b2h) planes_b2_half(b2h[n].b, k, b);
    if (n < n_b2w) planes_b2_half(b2w[n].b, k, b);
}
__global__ void __launch_bounds__(kBlock)
k_planes_b4(OmBvh4Node* b4, OmBvh4NodeH* b4h, const uint32_t* src, const uint32_t* srch, uint32_t n_slots, const OmBvhNode* tnodes) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_slots) return;
    planes_b4(b4[i >> 2], (int)(i & 3u), tnodes, src[i]);
    planes_b4_half(b4h[i >> 2], (int)(i & 3u), tnodes, srch[i]);
}
__global__ void __launch_bounds__(kBlock)
k_planes_always(OmAlwaysRec* recs, uint32_t n, const float* prim_box) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    OmAlwaysRec r = recs[i];
    planes_always(r, prim_box);
    recs[i] = r;
}

}  // namespace

hipError_t update(const Tables& t, const OmSceneDev& S, uint32_t first, const float* dev_vertices, uint32_t n_vertices,
                  const uint32_t* dev_indices, uint32_t n_tri, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(t.info, 0, kInfoWords * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    k_triangles<<<grid_of(n_tri), kBlock, 0, stream>>>((OmBary*)S.tri, t.prim_box, t.titems, t.tri_rec, t.tri_first, t.covering, first,
                                                       dev_vertices, n_vertices, dev_indices, n_tri, t.info);
    // the global BVH, in place: its nodes are its layout
    if (S.n_bvh_nodes) {
        OmBvhNode* bvh = (OmBvhNode*)S.bvh;
        k_leaves<<<grid_of(S.n_bvh_nodes), kBlock, 0, stream>>>(bvh, S.n_bvh_nodes, S.bvh_prims, t.prim_box);
        for (size_t l = t.g_level_off.size() - 1; l-- > 0;) {
            const uint32_t n = t.g_level_off[l + 1] - t.g_level_off[l];
            if (n) k_level<<<grid_of(n), kBlock, 0, stream>>>(bvh, t.g_level + t.g_level_off[l], n);
        }
    }
    if (t.n_tnodes) {
        k_leaves<<<grid_of(t.n_tnodes), kBlock, 0, stream>>>(t.tnodes, t.n_tnodes, t.titems, t.prim_box);
        for (size_t l = t.t_level_off.size() - 1; l-- > 0;) {
            const uint32_t n = t.t_level_off[l + 1] - t.t_level_off[l];
            if (n) k_level<<<grid_of(n), kBlock, 0, stream>>>(t.tnodes, t.t_level + t.t_level_off[l], n);
        }
        if (t.n_snode) k_planes_skip<<<grid_of(t.n_snode), kBlock, 0, stream>>>((OmSkipNode*)S.snodes, t.snode_src, t.n_snode, t.tnodes);
        const uint32_t n_src = 2u * (t.n_b2 > t.n_b2w ? t.n_b2 : t.n_b2w);
        if (n_src)
            k_planes_b2<<<grid_of(n_src), kBlock, 0, stream>>>((OmBvh2Node*)S.b2nodes, (OmBvh2NodeH*)S.b2h,
                                                               (OmBvh2NodeW*)(S.b2h + S.n_b2nodes), t.n_b2, t.n_b2h, t.n_b2w, t.b2_src, n_src,
                                                               t.tnodes);
        if (t.n_b4)
            k_planes_b4<<<grid_of(4u * t.n_b4), kBlock, 0, stream>>>((OmBvh4Node*)S.b4nodes, (OmBvh4NodeH*)S.b4h, t.b4_src, t.b4h_src,
                                                                     4u * t.n_b4, t.tnodes);
    }
    if (S.n_always2) k_planes_always<<<grid_of(S.n_always2), kBlock, 0, stream>>>((OmAlwaysRec*)S.always2_rec, S.n_always2, t.prim_box);
    return hipGetLastError();
}

}  // namespace omr
