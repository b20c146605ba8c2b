// om_b2_planes.h — the ray-ordered LDS copy of an f32 BVH2 node (OM_B2_PLANES,
// om_tuning.h).  Host and device: stage_scene<TR_BVH2_LDS> (om_wavefront.hip) writes it,
// traced_bvh2 (om_trace.h) reads it, tests/cpp/ordered_planes.cpp checks both on the host.
//
// Which of an axis's two box planes a ray meets first is fixed by the sign of its inverse
// direction on that axis, so the copy keeps each (child, axis) as three dwords [lo, hi, lo]: a
// lane reads the two dwords at dword offset s = (inverse direction < 0) and has (near plane, far
// plane) without a min/max per visit.  2 children x 3 axes x 3 dwords + the two child codes =
// 20 dwords, the 80-B slot OM_B2_NODE_STRIDE reserves.  The 64-B OmBvh2Node in memory is unchanged.
#pragma once
#include "om_layout.h"

struct OM_ALIGN16 OmBvh2NodeS {
    float p[18];      // [9 k + 3 a + {0, 1, 2}] = lo, hi, lo of child k on axis a, lo <= hi
    uint32_t c0, c1;  // child codes; an internal child's in 16-B units of the slot stride
};
static_assert(sizeof(OmBvh2NodeS) == 80, "the ordered node fills the 80-B slot");

// dword of the (near, far) pair of child k on axis a for a ray whose inverse direction on that
// axis is negative (s = 1) or not (s = 0)
OM_HD constexpr uint32_t b2s_pair(uint32_t k, uint32_t a, uint32_t s) { return 9u * k + 3u * a + s; }

// min / max of a plane pair that keep a NaN (either operand's) in both results, as the slab
// test's IEEE minimum / maximum would: such a box is still visited by every ray
OM_HD inline float b2s_min(float a, float b) { return a != a ? a : b != b ? b : (b < a ? b : a); }
OM_HD inline float b2s_max(float a, float b) { return a != a ? a : b != b ? b : (a < b ? b : a); }

// The staged copy of node n, internal child codes multiplied by `scale` (slot stride / 16).  The
// planes are stored min(lo, hi), max(lo, hi): the builder's boxes have lo <= hi except the empty
// second child of a single-leaf tree (om_bvh.cpp emit_bvh2: lo = +inf, hi = -inf), which the
// unordered test's min/max of the two slab values turns into all of space (every ray visits the
// empty leaf and tests nothing there); stored (-inf, +inf) it stays exactly that.
OM_HD inline OmBvh2NodeS b2s_order(const OmBvh2Node& n, uint32_t scale) {
    OmBvh2NodeS s;
    for (uint32_t k = 0; k < 2u; ++k)
        for (uint32_t a = 0; a < 3u; ++a) {
            const float lo = b2s_min(OM_B2_LO(n, k, a), OM_B2_HI(n, k, a)), hi = b2s_max(OM_B2_LO(n, k, a), OM_B2_HI(n, k, a));
            s.p[b2s_pair(k, a, 0u)] = lo; s.p[b2s_pair(k, a, 1u)] = hi; s.p[b2s_pair(k, a, 1u) + 1u] = lo;
        }
    s.c0 = n.c0 < OM_LEAF ? n.c0 * scale : n.c0;
    s.c1 = n.c1 < OM_LEAF ? n.c1 * scale : n.c1;
    return s;
}
