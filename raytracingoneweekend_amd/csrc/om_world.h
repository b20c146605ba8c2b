// om_world.h — host HittableList and its frozen, device-ready image.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ottomarcher.h"
#include "om_hostmath.h"
#include "om_layout.h"
#include "om_refit.h"
#include "om_tuning.h"

namespace om {

struct AffinePrim { Mat4 l2w, w2l; om_material mat; };              // Sphere / Cube (traced.rs:13-19, 229-235)
struct BaryPrim : BaryGeom { om_material mat; };                      // Barycentric<BT> (traced.rs:118-131; om_refit.h)
struct PlanePrim { Vec3 center, normal; om_material mat; };          // InfinitePlane (traced.rs:77-82)
struct MSpherePrim { Vec3 center; float radius; om_material mat; };  // marched.rs:50-54
struct MBoxPrim { Vec3 center, sizes; om_material mat; };            // marched.rs:79-83
struct MTorusPrim { Mat4 l2w_tr, w2l_tr; Vec4 l2w_s, w2l_s; Vec3 sizes; om_material mat; };  // marched.rs:105-113
// a user marched object (Arc<dyn Marched>, hits.rs:96-100): MarchedTorus's transform + an SDF program
struct MSdfPrim { MTorusPrim xf; std::vector<OmSdfOp> ops; om_material mat; };

enum PrimKind { K_SPHERE = 0, K_CUBE = 1, K_TRI = 2, K_PLANE = 3, K_PARA = 4, K_MSPHERE = 5, K_MBOX = 6, K_MTORUS = 7,
                K_MSDF = 8, K_N = 9 };

// Frozen image of a world: arrays laid out exactly as they are copied to HBM.
struct FrozenWorld {
    std::vector<OmAffineTest> sph_test, cube_test;
    std::vector<OmAffineHit> sph_hit, cube_hit;
    std::vector<OmBound> sph_bound, cube_bound;
    std::vector<OmBary> tri, para;
    std::vector<OmPlane> plane;
    std::vector<OmMSphere> msph;
    std::vector<OmMBox> mbox;
    std::vector<OmMTorus> mtor;
    std::vector<OmMSdf> msdf;          // user marched objects
    std::vector<OmSdfOp> msdf_ops;     // their programs, back to back
    std::vector<OmMaterial> mats;      // by global index
    std::vector<uint64_t> bloom;       // by obj id
    std::vector<OmBvhNode> bvh;
    std::vector<uint32_t> bvh_prims;   // global indices
    std::vector<uint32_t> always;      // global indices tested outside the BVH
    std::vector<OmSkipNode> snodes;    // stackless BVH (affine prims only)
    std::vector<OmAffineTest> srecs;   // its records in leaf order
    uint32_t n_srec_bary = 0;          // the OM_REC_BARY records among them (triangles / parallelograms in the leaves)
    std::vector<uint32_t> always2;     // prims outside the stackless BVH
    std::vector<OmAlwaysRec> always2_rec;  // the same, with their conservative boxes
    std::vector<float> srec_box;       // per srec: inflated box lo xyz, hi xyz (primary-ray tile lists)
    std::vector<OmBvh2Node> b2nodes;   // compressed BVH2 (same leaves/records as snodes)
    std::vector<OmBvh2NodeH> b2h;      // the same nodes with half-precision boxes rounded outward (device)
    std::vector<uint32_t> b2leaves;    // its leaf table: (first_record << 8) | count
    uint32_t b2_depth = 0;             // its depth (stack bound)
    uint32_t b2_direct = 0;            // 1: leaf child codes carry OM_LEAF | first_record << 4 | count (no table read)
    std::vector<OmBvh2NodeW> b2w;      // the BVH2 with 32-bit child codes (every world with a BVH2 whose records fit them)
    uint32_t b2w_depth = 0;            // its depth (stack bound)
    uint32_t b2_max_leaf = 0;          // records in the largest leaf of the BVH2
    std::vector<OmBvh4Node> b4nodes;   // 4-wide tree collapsed from b2nodes (leaf codes index b2leaves; none past the 16-bit codes)
    std::vector<OmBvh4NodeH> b4h;      // the same tree breadth-first, half-precision boxes rounded outward
    uint32_t b4_depth = 0;             // its depth
    uint32_t counts[K_N];
    uint32_t offsets[K_N + 1];         // global index offset per kind, offsets[K_N] = total
};

// Which traversal regime a frozen world gets (om_upload_world copies these into OmSceneDev; the
// host-only tests/cpp/tree_regimes.cpp reports them).  A zero *_lds_bytes means "not staged":
// the tree is read through L2 (BVH2 / BVH4) or from global memory (the megakernel's SBVH).
struct TreePlan {
    bool b2_ok = false;            // compressed BVH2 usable: node / leaf counts < kCode16Limit, depth <= kB2Stack
    uint32_t n_b2nodes = 0, n_b2leaves = 0, b2_direct = 0;
    uint32_t b2_stack = 0;         // lane-stack entries: one push per internal level, deepest included
    uint32_t b2_lds_bytes = 0;     // nodes (64 B each) + leaf table, rounded to 16, when within kB2LdsBudget
    bool b4_ok = false;
    uint32_t b4_stack = 0;         // 3 pushes per level + 3 spare entries for the unconditional pushes
    uint32_t b4_lds_bytes = 0;     // nodes (112 B each) + leaf table, rounded to 16, when within kB4LdsBudget
    uint32_t lds_bytes = 0;        // SBVH nodes + records when within kLdsBudget (at least 16)
    // wide BVH2 (32-bit codes): usable when the records fit the direct leaf code
    // (first < kDirectFirst32, count <= kLeafCountMax) and the depth the u32 lane stack's bound
    bool b2w_ok = false;
    uint32_t n_b2wnodes = 0, b2w_stack = 0;
};

// The wavefront's dynamic LDS per 512-lane workgroup in each BVH2 regime (om_wavefront.hip's
// trace_lds, restated for the host-only om_world_tree_info): [lane stack][nodes or prefix].
inline uint32_t wf_lds_b2_staged(uint32_t stack, uint32_t nodes, uint32_t leaves) {
    return OM_WF_BLOCK * stack * 2u + ((nodes * (uint32_t)OM_B2_NODE_STRIDE + leaves * 4u + 15u) & ~15u);
}
inline uint32_t wf_lds_b2_l2(uint32_t stack, uint32_t nodes) {
    const uint32_t cap = OM_WF_HYB_BYTES / (uint32_t)sizeof(OmBvh2NodeH);
    return OM_WF_BLOCK * stack * 2u + (nodes < cap ? nodes : cap) * (uint32_t)sizeof(OmBvh2NodeH);
}
inline uint32_t wf_lds_b2_wide(uint32_t stack, uint32_t nodes) {
    const uint32_t cap = OM_WF_HYBW_BYTES / (uint32_t)sizeof(OmBvh2NodeW);
    return OM_WF_BLOCK * stack * 4u + (nodes < cap ? nodes : cap) * (uint32_t)sizeof(OmBvh2NodeW);
}

inline TreePlan plan_trees(const FrozenWorld& fw) {
    TreePlan p;
    const size_t lds = fw.snodes.size() * sizeof(OmSkipNode) + fw.srecs.size() * sizeof(OmAffineTest);
    p.lds_bytes = lds <= kLdsBudget ? (uint32_t)(lds < 16 ? 16 : lds) : 0u;
    // compressed BVH2: usable when node and leaf ids fit the 15-bit codes and its depth fits
    // the lane-stack bound (otherwise the wavefront path uses the global-memory BVH)
    p.b2_ok = !fw.b2nodes.empty() && fw.b2nodes.size() < kCode16Limit && fw.b2leaves.size() < kCode16Limit &&
              fw.b2_depth <= kB2Stack;
    p.n_b2nodes = p.b2_ok ? (uint32_t)fw.b2nodes.size() : 0u;
    p.n_b2leaves = p.b2_ok ? (uint32_t)fw.b2leaves.size() : 0u;
    p.b2_direct = p.b2_ok ? fw.b2_direct : 0u;
    p.b2_stack = p.b2_ok ? fw.b2_depth : 0u;
    const size_t b2_bytes = fw.b2nodes.size() * sizeof(OmBvh2Node) + fw.b2leaves.size() * 4u;
    p.b2_lds_bytes = (p.b2_ok && b2_bytes <= kB2LdsBudget) ? (uint32_t)((b2_bytes + 15u) & ~(size_t)15u) : 0u;
    // BVH4 (same leaf table): within its lane-stack bound
    const uint32_t b4_stack = 3u * fw.b4_depth + 3u;
    p.b4_ok = p.b2_ok && !fw.b4nodes.empty() && fw.b4nodes.size() < kCode16Limit && b4_stack <= kB4Stack;
    p.b4_stack = p.b4_ok ? b4_stack : 0u;
    const size_t b4_bytes = fw.b4nodes.size() * sizeof(OmBvh4Node) + fw.b2leaves.size() * 4u;
    p.b4_lds_bytes = (p.b4_ok && b4_bytes <= kB4LdsBudget) ? (uint32_t)((b4_bytes + 15u) & ~(size_t)15u) : 0u;
    p.b2w_ok = !fw.b2w.empty() && fw.b2w.size() < OM_LEAFW && fw.srecs.size() < kDirectFirst32 && fw.b2_max_leaf <= kLeafCountMax &&
               fw.b2w_depth <= kB2WideStack &&
               fw.offsets[K_N] <= OM_REC_GI;   // its kernels are the OM_REC_BARY forms: gi beside two kind bits
    p.n_b2wnodes = p.b2w_ok ? (uint32_t)fw.b2w.size() : 0u;
    p.b2w_stack = p.b2w_ok ? fw.b2w_depth : 0u;
    return p;
}

// om_tree_info of a frozen world: its trees, and the regime and wavefront LDS of OM_KERNEL_AUTO
// (om_wavefront.hip's pick_trace; om_get_tree_info replaces the last two by the ctx's own choice).
inline void fill_tree_info(const FrozenWorld& fw, const TreePlan& p, om_tree_info* out) {
    out->records = (uint32_t)fw.srecs.size();
    out->always_tested = (uint32_t)fw.always2.size();
    out->b2_nodes = (uint32_t)fw.b2nodes.size();
    out->b2_leaves = (uint32_t)fw.b2leaves.size();
    out->b2_depth = fw.b2_depth;
    out->b2_max_leaf = fw.b2_max_leaf;
    if (p.b2_ok) {
        out->regime = p.b2_lds_bytes ? OM_TREE_LDS : OM_TREE_L2;
        out->lds_bytes = p.b2_lds_bytes ? wf_lds_b2_staged(p.b2_stack, p.n_b2nodes, p.n_b2leaves) : wf_lds_b2_l2(p.b2_stack, p.n_b2nodes);
    } else if (p.b2w_ok) {
        out->regime = OM_TREE_WIDE;
        out->lds_bytes = wf_lds_b2_wide(p.b2w_stack, p.n_b2wnodes);
    } else {
        out->regime = fw.bvh.size() <= 1u ? OM_TREE_NONE : OM_TREE_FALLBACK_BVH;
        out->lds_bytes = 0u;
    }
}

uint64_t bloom_hash(uint64_t id);      // utils.rs:94-107

}  // namespace om

struct om_world {
    std::vector<om::AffinePrim> spheres, cubes;
    std::vector<om::BaryPrim> triangles, parallelograms;
    std::vector<om::PlanePrim> planes;
    std::vector<om::MSpherePrim> msph;
    std::vector<om::MBoxPrim> mbox;
    std::vector<om::MTorusPrim> mtor;
    std::vector<om::MSdfPrim> msdf;
    // rt: also what a refit of the uploaded world needs (om_refit.h; filled for worlds with triangles)
    void freeze(om::FrozenWorld& fw, om::RefitTables* rt = nullptr) const;
};
