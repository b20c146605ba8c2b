// om_refit.h — moving triangles in an uploaded world: the pieces the host builder
// and the refit kernels share, and the tables a freeze keeps for the refit.
//
// A refit keeps the SAH topology and recomputes every box bottom-up.  Everything a box or a record
// is made of is computed HERE, once, by functions both sides call: the host builder (om_world.cpp,
// om_bvh.cpp) and the kernels of om_refit.hip.  The operations are +, -, *, 1/x and sqrt in f32 and
// +, -, *, compare in f64; with no contraction and correctly rounded divide / sqrt (csrc/Makefile)
// the device produces the host's bits, so an update with unchanged vertices reproduces the freeze.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "om_hostmath.h"
#include "om_layout.h"

namespace om {

// ---- the triangle record ----
// Barycentric<BT> without its material (traced.rs:118-131)
struct BaryGeom {
    Vec3 origin, u; float u_length; Vec3 v; float v_length; Vec3 uxv, uxvxu; Mat3 base_inv; Vec3 v_in_base;
};

OM_HD inline BaryGeom bary_geom(const Vec3& origin, const Vec3& u, const Vec3& v, float ul, float vl) {  // traced.rs:135-147
    BaryGeom b;
    const Vec3 uu = u.unit();
    const Vec3 vu = v.unit();
    const Vec3 uxv = uu.cross(vu).unit();
    const Vec3 uxvxu = uxv.cross(uu).unit();
    b.base_inv = Mat3::cols(uu, uxv, uxvxu).transpose();
    b.v_in_base = b.base_inv.apply(vu);
    b.origin = origin; b.u = uu; b.u_length = ul; b.v = vu; b.v_length = vl; b.uxv = uxv; b.uxvxu = uxvxu;
    return b;
}

OM_HD inline BaryGeom bary_geom3(const Vec3& o, const Vec3& up, const Vec3& vp) {                      // traced.rs:148-154
    const Vec3 ur = up.sub(o);
    const float ul = ur.length();
    const Vec3 vr = vp.sub(o);
    const float vl = vr.length();
    return bary_geom(o, ur, vr, ul, vl);
}

// the frozen record: what hit_aux reads
OM_HD inline void pack_bary(const BaryGeom& b, OmBary& o) {
    b.origin.store(o.origin); o.u_length = b.u_length; b.uxv.store(o.uxv); o.v_length = b.v_length;
    for (int r = 0; r < 3; ++r) b.base_inv.r[r].store(o.base_inv + 3 * r);
    o.vx = b.v_in_base.x(); o.vy = b.v_in_base.z(); o.pad = 0.0f;
}

// ---- boxes ----
struct Box {
    double lo[3], hi[3];
    OM_HD void empty() { for (int i = 0; i < 3; ++i) { lo[i] = 1e300; hi[i] = -1e300; } }
    // (a NaN compares false and is left out, as std::min / std::max leave it out)
    OM_HD void grow(const Box& b) { for (int i = 0; i < 3; ++i) { lo[i] = b.lo[i] < lo[i] ? b.lo[i] : lo[i]; hi[i] = hi[i] < b.hi[i] ? b.hi[i] : hi[i]; } }
    OM_HD void grow_pt(const double* p) { for (int i = 0; i < 3; ++i) { lo[i] = p[i] < lo[i] ? p[i] : lo[i]; hi[i] = hi[i] < p[i] ? p[i] : hi[i]; } }
    double area() const {
        const double dx = hi[0] - lo[0] > 0.0 ? hi[0] - lo[0] : 0.0, dy = hi[1] - lo[1] > 0.0 ? hi[1] - lo[1] : 0.0,
                     dz = hi[2] - lo[2] > 0.0 ? hi[2] - lo[2] : 0.0;
        return 2.0 * (dx * dy + dy * dz + dz * dx);
    }
};

// Inflate a box beyond the f32 rounding of the exact tests at the scene scale.  The margin is
// absolute; Sphere::hit accepts rays that pass an ellipsoid at up to about 6e-8 * (D^2 + C*D) / (2r)
// outside it (ray origin D away, world coordinates up to C, smallest semi-axis r), which passes
// this margin for r = 0.2 from D of about 100 on and for r <= 9e-3 at D = 13 (thin_sphere keeps
// out of the trees what the worst case of that error can reach from OM_SPHERE_REACH away): DESIGN.md §5.3
// states the domain, tests/test_scale_conservative.py measures it from these very boxes.
OM_HD inline Box inflate(Box b) {
    double mag = 0.0;
    for (int i = 0; i < 3; ++i) {
        const double al = fabs(b.lo[i]), ah = fabs(b.hi[i]);
        const double m = al < ah ? ah : al;
        mag = mag < m ? m : mag;
    }
    for (int i = 0; i < 3; ++i) {
        const double ext = b.hi[i] - b.lo[i];
        const double m = 1e-3 * (1.0 + ext) + 1e-5 * mag;
        b.lo[i] -= m; b.hi[i] += m;
    }
    return b;
}

// the box of a triangle (para: parallelogram), from its frozen origin, axes and lengths
OM_HD inline Box bary_box(const BaryGeom& p, bool para) {
    Box b; b.empty();
    double o[3], pu[3], pv[3], puv[3];
    for (int i = 0; i < 3; ++i) {
        o[i] = p.origin.e[i];
        pu[i] = o[i] + (double)p.u.e[i] * p.u_length;
        pv[i] = o[i] + (double)p.v.e[i] * p.v_length;
        puv[i] = pu[i] + (double)p.v.e[i] * p.v_length;
    }
    b.grow_pt(o); b.grow_pt(pu); b.grow_pt(pv);
    if (para) b.grow_pt(puv);
    return inflate(b);
}

// std::nextafter(x, up ? +inf : -inf), on the bits
OM_HD inline float f32_next(float x, bool up) {
    if (x != x) return x;
    uint32_t b;
    memcpy(&b, &x, 4);
    if (x == 0.0f) b = up ? 0x00000001u : 0x80000001u;
    else if (b == (up ? 0x7F800000u : 0xFF800000u)) return x;
    else b = ((b >> 31) != 0u) == up ? b - 1u : b + 1u;
    float r;
    memcpy(&r, &b, 4);
    return r;
}
// the f32 planes every layout stores: the double box rounded to f32 and one step outward
OM_HD inline void box_planes(const Box& b, float* lo, float* hi) {
    for (int i = 0; i < 3; ++i) { lo[i] = f32_next((float)b.lo[i], false); hi[i] = f32_next((float)b.hi[i], true); }
}

// IEEE half bits -> the value, exactly (every half is a float).
OM_HD inline float half_value(uint16_t h) {
    const int e = (h >> 10) & 31, m = h & 1023;
    const float v = e == 0 ? ldexpf((float)m, -24) : e == 31 ? INFINITY : ldexpf((float)(1024 + m), e - 25);
    return (h & 0x8000u) ? -v : v;
}
// The half-precision plane that contains x on the outside: the largest half <= x (up = false, a
// box's lo) or the smallest half >= x (up = true, its hi); +-inf beyond the half range.  Binary
// search over the halves in value order (key k >= 0: bits k; k < 0: the negative half -k).
OM_HD inline uint16_t half_key(int k) { return (uint16_t)(k >= 0 ? k : (0x8000 | -k)); }
OM_HD inline uint16_t half_out(float x, bool up) {
    if (x != x) return half_key(up ? 0x7C00 : -0x7C00);
    int lo = -0x7C00, hi = 0x7C00;                       // -inf .. +inf
    if (!up) {                                           // largest k with value(k) <= x
        while (lo < hi) { const int mid = lo + (hi - lo + 1) / 2; if (half_value(half_key(mid)) <= x) lo = mid; else hi = mid - 1; }
        return half_key(lo);
    }
    while (lo < hi) { const int mid = lo + (hi - lo) / 2; if (half_value(half_key(mid)) >= x) hi = mid; else lo = mid + 1; }
    return half_key(lo);
}

// ---- what a refit keeps of a primitive's box (6 floats: lo xyz, hi xyz) ----
// covering: a primitive whose record or box is not finite; every ray then runs its exact test, and
// half_out rounds such a plane to an infinite half.  none: a box that adds nothing to a union.
OM_HD inline void box_covering(float* b) { for (int i = 0; i < 3; ++i) { b[i] = -FLT_MAX; b[3 + i] = FLT_MAX; } }
OM_HD inline void box_none(float* b) { for (int i = 0; i < 3; ++i) { b[i] = FLT_MAX; b[3 + i] = -FLT_MAX; } }
OM_HD inline bool box_is_none(const float* b) { return b[0] == FLT_MAX && b[3] == -FLT_MAX; }
OM_HD inline bool finite_f32(float x) { return fabsf(x) <= FLT_MAX; }     // false for NaN

// One moved triangle: its frozen record and its box planes from three vertices.  -> kRefitRecOk when
// every value of the record is finite, | kRefitBoxOk when every plane is (they are written only then).
constexpr int kRefitRecOk = 1, kRefitBoxOk = 2;
OM_HD inline int refit_triangle(const float* a, const float* b, const float* c, OmBary& rec, float* planes) {
    const BaryGeom g = bary_geom3(Vec3::load(a), Vec3::load(b), Vec3::load(c));
    pack_bary(g, rec);
    const Box bx = bary_box(g, false);
    bool rec_ok = true, box_ok = true;
    const float* f = (const float*)&rec;
    for (unsigned k = 0; k < sizeof(OmBary) / 4u; ++k) rec_ok = rec_ok && finite_f32(f[k]);
    for (int k = 0; k < 3; ++k) box_ok = box_ok && fabs(bx.lo[k]) <= DBL_MAX && fabs(bx.hi[k]) <= DBL_MAX;
    float p[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (box_ok) box_planes(bx, p, p + 3);
    for (int k = 0; k < 6; ++k) box_ok = box_ok && finite_f32(p[k]);
    if (box_ok) for (int k = 0; k < 6; ++k) planes[k] = p[k];
    return (rec_ok ? kRefitRecOk : 0) | (box_ok ? kRefitBoxOk : 0);
}
// The box a refit keeps for that triangle (`old` = the one it had), as the freeze's select has it:
// its planes when they are finite, whatever the record holds (the global BVH takes every such
// triangle as an item); covering otherwise, except that a box the freeze left out of every union
// (none: its min / max skip a NaN) stays left out while it stays non-finite.
OM_HD inline void refit_triangle_box(int ok, const float* planes, const float* old, float* out) {
    if (ok & kRefitBoxOk) { for (int k = 0; k < 6; ++k) out[k] = planes[k]; return; }
    if (box_is_none(old)) box_none(out); else box_covering(out);
}
// In the leaf-record tree the freeze keeps a triangle with a non-finite record or box outside, so
// that no cull stands before its exact test.  A refit keeps the topology: the record of such a
// triangle takes the covering box (slot `covering` of the primitive boxes) in place of its own.
OM_HD inline uint32_t refit_triangle_item(int ok, uint32_t gi, uint32_t covering) {
    return ok == (kRefitRecOk | kRefitBoxOk) ? gi : covering;
}

// ---- bottom-up: a node's box from its children ----
OM_HD inline void box_union(const float* a, const float* b, float* out) {
    for (int i = 0; i < 3; ++i) { out[i] = b[i] < a[i] ? b[i] : a[i]; out[3 + i] = a[3 + i] < b[3 + i] ? b[3 + i] : a[3 + i]; }
}
OM_HD inline void node_box(const OmBvhNode& n, float* b) { for (int i = 0; i < 3; ++i) { b[i] = n.lo[i]; b[3 + i] = n.hi[i]; } }
OM_HD inline void set_node_box(OmBvhNode& n, const float* b) { for (int i = 0; i < 3; ++i) { n.lo[i] = b[i]; n.hi[i] = b[3 + i]; } }

// A refit topology: the builder's nodes, parents before children (the root is node 0).  A leaf
// (left < 0) owns items [-(left + 1), -(left + 1) + right) of `items`, each the index of a
// primitive box; an internal node the union of nodes left and right.
// leaf: the union of its items' boxes (none for an empty leaf)
OM_HD inline void refit_leaf(OmBvhNode& n, const uint32_t* items, const float* prim_box) {
    float b[6];
    box_none(b);
    const uint32_t first = (uint32_t)(-(n.left + 1)), cnt = (uint32_t)n.right;
    for (uint32_t k = 0; k < cnt; ++k) box_union(b, prim_box + 6u * (size_t)items[first + k], b);
    set_node_box(n, b);
}
OM_HD inline void refit_internal(OmBvhNode* nodes, uint32_t i) {
    float a[6], b[6], u[6];
    node_box(nodes[(uint32_t)nodes[i].left], a);
    node_box(nodes[(uint32_t)nodes[i].right], b);
    box_union(a, b, u);
    set_node_box(nodes[i], u);
}

// ---- the planes of every layout from the nodes' boxes ----
constexpr uint32_t kRefitNoNode = 0xFFFFFFFFu;     // a child slot without a node (the second child of a single leaf; a BVH4 slot)
// the f32 box of a layout slot: its builder node's, or the empty box a missing BVH2 child has
OM_HD inline void slot_box(const OmBvhNode* nodes, uint32_t src, float* b) {
    if (src == kRefitNoNode) { for (int i = 0; i < 3; ++i) { b[i] = INFINITY; b[3 + i] = -INFINITY; } return; }
    node_box(nodes[src], b);
}
OM_HD inline void planes_skip(OmSkipNode& o, const float* b) { for (int i = 0; i < 3; ++i) { o.lo[i] = b[i]; o.hi[i] = b[3 + i]; } }
OM_HD inline void planes_b2(OmBvh2Node& o, int k, const float* b) {
    for (int i = 0; i < 3; ++i) { (k ? o.lo1 : o.lo0)[i] = b[i]; (k ? o.hi1 : o.hi0)[i] = b[3 + i]; }
}
// b2h and b2w: b[6k ..] = child k's lo xyz, hi xyz as outward halves
OM_HD inline void planes_b2_half(uint16_t* hb, int k, const float* b) {
    for (int i = 0; i < 3; ++i) { hb[6 * k + i] = half_out(b[i], false); hb[6 * k + 3 + i] = half_out(b[3 + i], true); }
}
OM_HD inline void planes_b4(OmBvh4Node& o, int k, const OmBvhNode* nodes, uint32_t src) {
    float b[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};             // an empty slot keeps zeros
    if (src != kRefitNoNode) node_box(nodes[src], b);
    o.lox[k] = b[0]; o.loy[k] = b[1]; o.loz[k] = b[2]; o.hix[k] = b[3]; o.hiy[k] = b[4]; o.hiz[k] = b[5];
}
OM_HD inline void planes_b4_half(OmBvh4NodeH& o, int k, const OmBvhNode* nodes, uint32_t src) {
    float b[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (src != kRefitNoNode) node_box(nodes[src], b);
    o.b[k] = half_out(b[0], false); o.b[4 + k] = half_out(b[1], false); o.b[8 + k] = half_out(b[2], false);
    o.b[12 + k] = half_out(b[3], true); o.b[16 + k] = half_out(b[4], true); o.b[20 + k] = half_out(b[5], true);
}
// a record outside the trees with a finite box follows its primitive; an unbounded one stays unbounded
OM_HD inline void planes_always(OmAlwaysRec& r, const float* prim_box) {
    bool boxed = true;
    for (int i = 0; i < 3; ++i) boxed = boxed && finite_f32(r.lo[i]) && finite_f32(r.hi[i]);
    if (!boxed) return;
    const float* b = prim_box + 6u * (size_t)r.gi;
    for (int i = 0; i < 3; ++i) { r.lo[i] = b[i]; r.hi[i] = b[3 + i]; }
}

// What a freeze keeps for the refit (worlds with triangles only; om::build_bvh fills it).  Two
// topologies: the global BVH (`bvh` over `bvh_prims`, refitted in place: its nodes are its layout)
// and the leaf-record tree `tnodes` behind snodes / b2nodes / b2h / b2w / b4nodes / b4h, whose
// leaves own records of srecs (`titems`: the primitive of each record).  Internal nodes by depth
// (`*_level`, level l = [off[l], off[l + 1])), so a refit runs one pass per level, deepest first.
struct RefitTables {
    std::vector<float> prim_box;                 // 6 per traced primitive, by gi (none: not an item of any tree), then the covering box
    uint32_t covering = 0;                       // the index of that last box
    uint32_t tri_first = 0;                      // gi of triangle 0
    std::vector<uint32_t> tri_rec;               // per triangle: its record of srecs, kRefitNoNode outside the tree
    std::vector<uint32_t> g_level, g_level_off;  // the global BVH's internal nodes by depth
    std::vector<OmBvhNode> tnodes;               // the leaf-record tree (a leaf's left: -(first record + 1))
    std::vector<uint32_t> titems;                // per record of srecs: its box among prim_box (its gi, or `covering`)
    std::vector<uint32_t> t_level, t_level_off;
    std::vector<uint32_t> snode_src;             // per snode: its tnode
    std::vector<uint32_t> b2_src;                // per b2 node (b2nodes, b2h, b2w share the order): child 0's, child 1's tnode
    std::vector<uint32_t> b4_src, b4h_src;       // per b4 node / b4h node: its four children's tnodes
    bool empty() const { return prim_box.empty(); }
};

// internal nodes of a parents-before-children tree grouped by depth
inline void refit_levels(const std::vector<OmBvhNode>& nodes, std::vector<uint32_t>& level, std::vector<uint32_t>& off) {
    level.clear(); off.assign(1, 0u);
    if (nodes.empty()) return;
    std::vector<uint32_t> d(nodes.size(), 0u);
    uint32_t deepest = 0;
    std::vector<uint32_t> count;
    for (size_t n = 0; n < nodes.size(); ++n) {
        if (nodes[n].left < 0) continue;
        d[(uint32_t)nodes[n].left] = d[(uint32_t)nodes[n].right] = d[n] + 1u;
        if (d[n] >= count.size()) count.resize(d[n] + 1u, 0u);
        ++count[d[n]];
        deepest = d[n] > deepest ? d[n] : deepest;
    }
    off.assign(count.size() + 1u, 0u);
    for (size_t l = 0; l < count.size(); ++l) off[l + 1] = off[l] + count[l];
    level.resize(off.back());
    std::vector<uint32_t> at(off.begin(), off.end() - 1);
    for (size_t n = 0; n < nodes.size(); ++n)
        if (nodes[n].left >= 0) level[at[d[n]]++] = (uint32_t)n;
}

// The whole refit on the host, over host copies of the arrays (tests/cpp/refit_check.cpp; the
// kernels of om_refit.hip run the same functions, one thread per element): steps 2 and 3.
struct RefitArrays {
    OmBvhNode* bvh; const uint32_t* bvh_prims; uint32_t n_bvh;
    OmSkipNode* snodes; OmBvh2Node* b2nodes; OmBvh2NodeH* b2h; OmBvh2NodeW* b2w; uint32_t n_b2, n_b2h, n_b2w;
    OmBvh4Node* b4nodes; OmBvh4NodeH* b4h; uint32_t n_b4, n_b4h;
    OmAlwaysRec* always2_rec; uint32_t n_always2;
};
inline void refit_host(RefitTables& t, const RefitArrays& a) {
    for (uint32_t n = 0; n < a.n_bvh; ++n) if (a.bvh[n].left < 0) refit_leaf(a.bvh[n], a.bvh_prims, t.prim_box.data());
    for (size_t l = t.g_level_off.size() - 1; l-- > 0;)
        for (uint32_t k = t.g_level_off[l]; k < t.g_level_off[l + 1]; ++k) refit_internal(a.bvh, t.g_level[k]);
    for (OmBvhNode& n : t.tnodes) if (n.left < 0) refit_leaf(n, t.titems.data(), t.prim_box.data());
    for (size_t l = t.t_level_off.size() - 1; l-- > 0;)
        for (uint32_t k = t.t_level_off[l]; k < t.t_level_off[l + 1]; ++k) refit_internal(t.tnodes.data(), t.t_level[k]);
    float b[6];
    for (size_t i = 0; i < t.snode_src.size(); ++i) { slot_box(t.tnodes.data(), t.snode_src[i], b); planes_skip(a.snodes[i], b); }
    for (size_t i = 0; i < t.b2_src.size(); ++i) {
        const uint32_t n = (uint32_t)(i / 2u); const int k = (int)(i & 1u);
        slot_box(t.tnodes.data(), t.b2_src[i], b);
        if (n < a.n_b2) planes_b2(a.b2nodes[n], k, b);
        if (n < a.n_b2h) planes_b2_half(a.b2h[n].b, k, b);
        if (n < a.n_b2w) planes_b2_half(a.b2w[n].b, k, b);
    }
    for (size_t i = 0; i < t.b4_src.size() && i / 4u < a.n_b4; ++i) planes_b4(a.b4nodes[i / 4u], (int)(i & 3u), t.tnodes.data(), t.b4_src[i]);
    for (size_t i = 0; i < t.b4h_src.size() && i / 4u < a.n_b4h; ++i) planes_b4_half(a.b4h[i / 4u], (int)(i & 3u), t.tnodes.data(), t.b4h_src[i]);
    for (uint32_t i = 0; i < a.n_always2; ++i) planes_always(a.always2_rec[i], t.prim_box.data());
}

}  // namespace om
