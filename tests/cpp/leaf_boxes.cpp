// leaf_boxes.cpp — the boxes every tree layout gives the primitives of a world (host code only).
//
// tests/test_scale_conservative.py builds the worlds of tests/scale_common.py in numpy, writes each
// to a file (scale_common.dump: u32 item count, then per item a u32 tag; 1 sphere_radius: 4 f32;
// 2 sphere, 3 cube: 16 f32 local_to_world; 5 triangle, 6 parallelogram: three points, 9 f32) and
// runs `leaf_boxes NAME FILE [NAME FILE ...]`.  This program adds the items in order, freezes the
// world and prints JSON lines:
//   {"world", "prims", "srecs", "always": [gi ...], "always2": [gi ...], "always2_unbounded": [gi ...],
//    "b2_ok", "b2w_ok", "b4_ok", "b2_lds_bytes", "root": the box of the bounded primitives,
//    "slab_reach": OM_SLAB_REACH, "sphere_reach": OM_SPHERE_REACH (which rays take the reference loop,
//    which spheres stay outside the trees)}
//   {"world", "leaf": gi, "box": [lo xyz, hi xyz]}             the f32 box of a tree-resident primitive
//                                                              (FrozenWorld::srec_box, what the builder unites)
//   {"world", "layout": L, "gi": gi, "chain": [[box] ...]}     the boxes a traversal of layout L tests on
//                                                              its way from the root to the leaf that holds gi
// with L one of bvh (OmBvhNode), sbvh (OmSkipNode), bvh2 (OmBvh2Node), bvh2h (OmBvh2NodeH, half
// planes), bvh2w (OmBvh2NodeW, half planes), bvh4 (OmBvh4Node), bvh4h (OmBvh4NodeH, half planes).
// The BVH2 / BVH4 layouts keep a child's box in its parent, so their chains start below the root.
// An infinite plane is printed as +-1e999, which a JSON reader takes as +-inf.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../raytracingoneweekend_amd/csrc/om_bvh.h"
#include "../../raytracingoneweekend_amd/csrc/om_tuning.h"
#include "../../raytracingoneweekend_amd/csrc/om_world.h"
#include "ottomarcher.h"
#include "world_file.h"

namespace {

int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

struct Box { float v[6]; };
typedef std::vector<Box> Chain;

std::string num(float x) {
    if (std::isinf(x)) return x > 0 ? "1e999" : "-1e999";
    char b[40];
    std::snprintf(b, sizeof b, "%.9g", (double)x);
    return b;
}
std::string box_json(const Box& b) {
    std::string s = "[";
    for (int i = 0; i < 6; ++i) s += (i ? ", " : "") + num(b.v[i]);
    return s + "]";
}
std::string list_json(const std::vector<uint32_t>& v) {
    std::string s = "[";
    for (size_t i = 0; i < v.size(); ++i) s += (i ? ", " : "") + std::to_string(v[i]);
    return s + "]";
}

struct Out {
    const char* world; const char* layout; const om::FrozenWorld& fw;
    void leaf(uint32_t first, uint32_t cnt, const Chain& c) const {
        for (uint32_t k = 0; k < cnt; ++k) {
            uint32_t tag;
            std::memcpy(&tag, &fw.srecs[first + k].pad, 4);
            emit(tag & OM_REC_GI, c);
        }
    }
    void emit(uint32_t gi, const Chain& c) const {
        std::string s = "[";
        for (size_t i = 0; i < c.size(); ++i) s += (i ? ", " : "") + box_json(c[i]);
        std::printf("{\"world\": \"%s\", \"layout\": \"%s\", \"gi\": %u, \"chain\": %s]}\n", world, layout, gi, s.c_str());
    }
};

void walk_bvh(const Out& o, uint32_t n, Chain& c) {
    const OmBvhNode& N = o.fw.bvh[n];
    c.push_back(Box{{N.lo[0], N.lo[1], N.lo[2], N.hi[0], N.hi[1], N.hi[2]}});
    if (N.left < 0) {
        for (int32_t k = 0; k < N.right; ++k) o.emit(o.fw.bvh_prims[(uint32_t)(-N.left - 1) + (uint32_t)k], c);
    } else {
        walk_bvh(o, (uint32_t)N.left, c);
        walk_bvh(o, (uint32_t)N.right, c);
    }
    c.pop_back();
}

void walk_sbvh(const Out& o, uint32_t n, Chain& c) {
    const OmSkipNode& N = o.fw.snodes[n];
    c.push_back(Box{{N.lo[0], N.lo[1], N.lo[2], N.hi[0], N.hi[1], N.hi[2]}});
    if (N.leaf != 0xFFFFFFFFu) o.leaf(N.leaf >> 8, N.leaf & 255u, c);
    else for (uint32_t k = n + 1; k < N.skip; k = o.fw.snodes[k].skip) walk_sbvh(o, k, c);
    c.pop_back();
}

// (first, count) of a 16-bit leaf code (om_trace.h leaf_payload)
void leaf16(const om::FrozenWorld& fw, uint32_t code, uint32_t& first, uint32_t& cnt) {
    if (fw.b2_direct) { first = (code >> kLeafCountBits) & (kDirectFirst16 - 1u); cnt = code & kLeafCountMax; return; }
    const uint32_t l = fw.b2leaves[code & (OM_LEAF - 1u)];
    first = l >> 8; cnt = l & 255u;
}

template <bool HALF>
Box b2_child(const om::FrozenWorld& fw, uint32_t n, int k) {
    Box b;
    for (int i = 0; i < 3; ++i) {
        if (HALF) {
            b.v[i] = om::half_value(fw.b2h[n].b[6 * k + i]);
            b.v[3 + i] = om::half_value(fw.b2h[n].b[6 * k + 3 + i]);
        } else {
            b.v[i] = OM_B2_LO(fw.b2nodes[n], k, i);
            b.v[3 + i] = OM_B2_HI(fw.b2nodes[n], k, i);
        }
    }
    return b;
}
template <bool HALF>
void walk_b2(const Out& o, uint32_t n, Chain& c) {
    for (int k = 0; k < 2; ++k) {
        const uint32_t code = k == 0 ? o.fw.b2nodes[n].c0 : o.fw.b2nodes[n].c1;
        if (HALF) EXPECT(code == (k == 0 ? o.fw.b2h[n].c0 : o.fw.b2h[n].c1));
        c.push_back(b2_child<HALF>(o.fw, n, k));
        if (code & OM_LEAF) { uint32_t f, cnt; leaf16(o.fw, code, f, cnt); o.leaf(f, cnt, c); }
        else walk_b2<HALF>(o, code, c);
        c.pop_back();
    }
}

void walk_b2w(const Out& o, uint32_t n, Chain& c) {
    const OmBvh2NodeW& N = o.fw.b2w[n];
    for (int k = 0; k < 2; ++k) {
        const uint32_t code = k == 0 ? N.c0 : N.c1;
        Box b;
        for (int i = 0; i < 3; ++i) { b.v[i] = om::half_value(N.b[6 * k + i]); b.v[3 + i] = om::half_value(N.b[6 * k + 3 + i]); }
        c.push_back(b);
        if (code & OM_LEAFW) o.leaf((code & ~OM_LEAFW) >> kLeafCountBits, code & kLeafCountMax, c);
        else walk_b2w(o, code, c);
        c.pop_back();
    }
}

void walk_b4(const Out& o, uint32_t n, Chain& c) {
    const OmBvh4Node& N = o.fw.b4nodes[n];
    for (int k = 0; k < 4; ++k) {
        if (N.child[k] == OM_EMPTY) continue;
        c.push_back(Box{{N.lox[k], N.loy[k], N.loz[k], N.hix[k], N.hiy[k], N.hiz[k]}});
        if (N.child[k] & OM_LEAF) { uint32_t f, cnt; leaf16(o.fw, N.child[k], f, cnt); o.leaf(f, cnt, c); }
        else walk_b4(o, N.child[k], c);
        c.pop_back();
    }
}
void walk_b4h(const Out& o, uint32_t n, Chain& c) {
    const OmBvh4NodeH& N = o.fw.b4h[n];
    for (int k = 0; k < 4; ++k) {
        if (N.child[k] == OM_EMPTY) continue;
        Box b;
        for (int p = 0; p < 6; ++p) b.v[p] = om::half_value(N.b[p * 4 + k]);
        c.push_back(b);
        if (N.child[k] & OM_LEAF) { uint32_t f, cnt; leaf16(o.fw, N.child[k], f, cnt); o.leaf(f, cnt, c); }
        else walk_b4h(o, N.child[k], c);
        c.pop_back();
    }
}

void report(const char* name, const om_world* w) {
    om::FrozenWorld fw;
    w->freeze(fw);
    const om::TreePlan p = om::plan_trees(fw);
    std::vector<uint32_t> unbounded;
    for (const OmAlwaysRec& a : fw.always2_rec) if (a.lo[0] == -INFINITY) unbounded.push_back(a.gi);
    Box root{{-INFINITY, -INFINITY, -INFINITY, INFINITY, INFINITY, INFINITY}};
    if (!fw.bvh.empty()) root = Box{{fw.bvh[0].lo[0], fw.bvh[0].lo[1], fw.bvh[0].lo[2], fw.bvh[0].hi[0], fw.bvh[0].hi[1], fw.bvh[0].hi[2]}};
    std::printf("{\"world\": \"%s\", \"prims\": %u, \"srecs\": %zu, \"always\": %s, \"always2\": %s, \"always2_unbounded\": %s, "
                "\"b2_ok\": %d, \"b2w_ok\": %d, \"b4_ok\": %d, \"b2_lds_bytes\": %u, \"root\": %s, \"slab_reach\": %.9g, \"sphere_reach\": %.9g}\n",
                name, fw.offsets[om::K_N], fw.srecs.size(), list_json(fw.always).c_str(), list_json(fw.always2).c_str(),
                list_json(unbounded).c_str(), p.b2_ok ? 1 : 0, p.b2w_ok ? 1 : 0, p.b4_ok ? 1 : 0, p.b2_lds_bytes,
                box_json(root).c_str(), (double)OM_SLAB_REACH, (double)OM_SPHERE_REACH);
    EXPECT(fw.srec_box.size() == fw.srecs.size() * 6u);
    for (size_t r = 0; r < fw.srecs.size(); ++r) {
        uint32_t tag;
        std::memcpy(&tag, &fw.srecs[r].pad, 4);
        Box b;
        for (int i = 0; i < 6; ++i) b.v[i] = fw.srec_box[6 * r + (size_t)i];
        std::printf("{\"world\": \"%s\", \"leaf\": %u, \"box\": %s}\n", name, tag & OM_REC_GI, box_json(b).c_str());
    }
    // the bounded always2 records (barycentric primitives of a world below OM_BARY_TREE_MIN): one box each
    for (const OmAlwaysRec& a : fw.always2_rec) {
        if (a.lo[0] == -INFINITY) continue;
        const Out o{name, "always2", fw};
        o.emit(a.gi, Chain{Box{{a.lo[0], a.lo[1], a.lo[2], a.hi[0], a.hi[1], a.hi[2]}}});
    }
    Chain c;
    if (!fw.bvh.empty()) walk_bvh(Out{name, "bvh", fw}, 0u, c);
    if (!fw.snodes.empty()) walk_sbvh(Out{name, "sbvh", fw}, 0u, c);
    if (p.b2_ok) {
        walk_b2<false>(Out{name, "bvh2", fw}, 0u, c);
        EXPECT(fw.b2h.size() == fw.b2nodes.size());
        walk_b2<true>(Out{name, "bvh2h", fw}, 0u, c);
    }
    if (p.b2w_ok) walk_b2w(Out{name, "bvh2w", fw}, 0u, c);
    if (p.b4_ok) {
        walk_b4(Out{name, "bvh4", fw}, 0u, c);
        EXPECT(fw.b4h.size() == fw.b4nodes.size());
        walk_b4h(Out{name, "bvh4h", fw}, 0u, c);
    }
    EXPECT(c.empty());
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3 || (argc - 1) % 2 != 0) {
        std::fprintf(stderr, "usage: leaf_boxes NAME FILE [NAME FILE ...]\n");
        return 2;
    }
    for (int a = 1; a + 1 < argc; a += 2) {
        om_world* w = nullptr;
        EXPECT(om_world_create(&w) == OM_OK);
        if (!load(argv[a + 1], w)) { std::fprintf(stderr, "FAIL cannot load %s\n", argv[a + 1]); ++g_fail; }
        else report(argv[a], w);
        om_world_destroy(w);
    }
    return g_fail == 0 ? 0 : 1;
}
