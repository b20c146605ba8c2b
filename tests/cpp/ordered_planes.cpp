// ordered_planes.cpp — the ray-ordered LDS copy of the BVH2 nodes decides what the unordered
// node test decides (host code only; DESIGN.md §5.6, om_b2_planes.h).
//
// stage_scene<TR_BVH2_LDS> rewrites every f32 node into an OmBvh2NodeS (b2s_order): per child
// and axis [lo, hi, lo], so that a ray reads (near plane, far plane) at the dword the sign of its
// inverse direction picks, where the unordered test takes smin / smax of the two slab values at
// every visit.  This program freezes the worlds whose BVH2 is staged in LDS -- the regime worlds
// g0, g11, g15, g16, c7x17, c7x18, c8x17 of tree_scenes.h and the mesh worlds handed to it as
// files (`ordered_planes NAME FILE ...`, tests/test_ordered_planes.py writes ico2) -- and checks
//   * the staged copy: lo <= hi on every axis, the third dword repeats the first, the two planes
//     are the node's own, internal codes are scaled and stay below OM_LEAF, leaf codes are kept;
//     an inverted box (the empty second child of a one-leaf tree) is staged (-inf, +inf);
//   * for every node and every ray of a set covering the 8 sign octants, axis-parallel rays with
//     one and two zero components of either sign, origins on the node's own planes and inside its
//     boxes, and random rays: h0, h1 and swap of the ordered read equal those of the unordered
//     test, and near / far of each box are the same bits -- or two zeros of opposite sign, which
//     IEEE minimum / maximum order (-0 < +0) but no compare of the traversal tells apart.  Those
//     cases are counted, not hidden: the report prints them.
// The arithmetic is the device's, statement for statement (om_trace.h: inv_dir, slabs, smin /
// smax as IEEE minimum / maximum), except inv_dir's hardware reciprocal, here 1 / k: the claim
// is about any inverse direction of the ray's sign.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../raytracingoneweekend_amd/csrc/om_b2_planes.h"
#include "../../raytracingoneweekend_amd/csrc/om_tuning.h"
#include "../../raytracingoneweekend_amd/csrc/om_world.h"
#include "ottomarcher.h"
#include "tree_scenes.h"
#include "world_file.h"

namespace {

int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { if (g_fail < 20) std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
// IEEE 754-2019 minimum / maximum (v_minimum3_f32 / v_maximum3_f32): a NaN wins, -0 < +0
float smin(float a, float b) {
    if (a != a) return a;
    if (b != b) return b;
    if (a == 0.f && b == 0.f) return std::signbit(a) ? a : b;
    return b < a ? b : a;
}
float smax(float a, float b) {
    if (a != a) return a;
    if (b != b) return b;
    if (a == 0.f && b == 0.f) return std::signbit(a) ? b : a;
    return a < b ? b : a;
}
float smin3(float a, float b, float c) { return smin(smin(a, b), c); }
float smax3(float a, float b, float c) { return smax(smax(a, b), c); }
float slab_near(float x0, float x1, float y0, float y1, float z0, float z1, float t_lo) {
    return smax3(smin(x0, x1), smin(y0, y1), smax(smin(z0, z1), t_lo));
}
float slab_far(float x0, float x1, float y0, float y1, float z0, float z1, float t_hi) {
    return smin3(smax(x0, x1), smax(y0, y1), smin(smax(z0, z1), t_hi));
}
float inv_dir(float c) {
    const float k = std::fabs(c) > 1e-20f ? c : std::copysign(1e-20f, c);
    return 1.0f / k;
}

struct Ray { float o[3], d[3]; };
struct Out { float n0, f0, n1, f1; bool h0, h1, swap; };

struct Setup {
    float ix, iy, iz, nox, noy, noz, t_lo, t_hi;
    Setup(const Ray& r, float tmin, float closest)
        : ix(inv_dir(r.d[0])), iy(inv_dir(r.d[1])), iz(inv_dir(r.d[2])),
          nox(-r.o[0] * ix), noy(-r.o[1] * iy), noz(-r.o[2] * iz),
          t_lo(tmin * 0.5f - 1e-3f), t_hi(closest * 1.0001f + 1e-3f) {}
};

// the unordered visit (traced_bvh2's slabs over an OmBvh2Node)
Out unordered(const OmBvh2Node& N, const Setup& s) {
    Out r;
    float x0 = std::fmaf(N.lo0[0], s.ix, s.nox), x1 = std::fmaf(N.hi0[0], s.ix, s.nox);
    float y0 = std::fmaf(N.lo0[1], s.iy, s.noy), y1 = std::fmaf(N.hi0[1], s.iy, s.noy);
    float z0 = std::fmaf(N.lo0[2], s.iz, s.noz), z1 = std::fmaf(N.hi0[2], s.iz, s.noz);
    r.n0 = slab_near(x0, x1, y0, y1, z0, z1, s.t_lo);
    r.f0 = slab_far(x0, x1, y0, y1, z0, z1, s.t_hi);
    x0 = std::fmaf(N.lo1[0], s.ix, s.nox); x1 = std::fmaf(N.hi1[0], s.ix, s.nox);
    y0 = std::fmaf(N.lo1[1], s.iy, s.noy); y1 = std::fmaf(N.hi1[1], s.iy, s.noy);
    z0 = std::fmaf(N.lo1[2], s.iz, s.noz); z1 = std::fmaf(N.hi1[2], s.iz, s.noz);
    r.n1 = slab_near(x0, x1, y0, y1, z0, z1, s.t_lo);
    r.f1 = slab_far(x0, x1, y0, y1, z0, z1, s.t_hi);
    r.h0 = !(r.n0 > r.f0); r.h1 = !(r.n1 > r.f1); r.swap = r.n1 < r.n0;
    return r;
}

// the ordered visit (traced_bvh2's slabs over an OmBvh2NodeS): per axis one base dword, picked once per ray
Out ordered(const OmBvh2NodeS& N, const Setup& s) {
    Out r;
    const float* x = N.p + b2s_pair(0u, 0u, s.ix < 0.f ? 1u : 0u);
    const float* y = N.p + b2s_pair(0u, 1u, s.iy < 0.f ? 1u : 0u);
    const float* z = N.p + b2s_pair(0u, 2u, s.iz < 0.f ? 1u : 0u);
    constexpr uint32_t k1 = b2s_pair(1u, 0u, 0u);
    r.n0 = smax3(std::fmaf(x[0], s.ix, s.nox), std::fmaf(y[0], s.iy, s.noy), smax(std::fmaf(z[0], s.iz, s.noz), s.t_lo));
    r.f0 = smin3(std::fmaf(x[1], s.ix, s.nox), std::fmaf(y[1], s.iy, s.noy), smin(std::fmaf(z[1], s.iz, s.noz), s.t_hi));
    r.n1 = smax3(std::fmaf(x[k1], s.ix, s.nox), std::fmaf(y[k1], s.iy, s.noy), smax(std::fmaf(z[k1], s.iz, s.noz), s.t_lo));
    r.f1 = smin3(std::fmaf(x[k1 + 1u], s.ix, s.nox), std::fmaf(y[k1 + 1u], s.iy, s.noy), smin(std::fmaf(z[k1 + 1u], s.iz, s.noz), s.t_hi));
    r.h0 = !(r.n0 > r.f0); r.h1 = !(r.n1 > r.f1); r.swap = r.n1 < r.n0;
    return r;
}

struct Tally { uint64_t tests = 0, zero_sign = 0, mismatch = 0, both = 0, one = 0, none = 0, swaps = 0; };

// the same bits (or NaN both), or two zeros (of opposite sign)
void same(float a, float b, Tally& t) {
    if (bits(a) == bits(b) || (a != a && b != b)) return;
    if (a == 0.f && b == 0.f) { ++t.zero_sign; return; }
    ++t.mismatch;
}

void check(const OmBvh2Node& N, const OmBvh2NodeS& S, const Ray& r, float tmin, float closest, Tally& t) {
    const Setup s(r, tmin, closest);
    const Out u = unordered(N, s), o = ordered(S, s);
    ++t.tests;
    same(u.n0, o.n0, t); same(u.f0, o.f0, t); same(u.n1, o.n1, t); same(u.f1, o.f1, t);
    if (u.h0 != o.h0 || u.h1 != o.h1 || u.swap != o.swap) ++t.mismatch;
    if (u.h0 && u.h1) { ++t.both; t.swaps += u.swap ? 1u : 0u; } else if (u.h0 || u.h1) ++t.one; else ++t.none;
}

struct Lcg {
    uint64_t s;
    float uni() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (float)(s >> 40) * (1.0f / 16777216.0f); }
    float sym() { return uni() * 2.f - 1.f; }
};

// directions: the 8 octants (generic and near-axis), every axis-parallel direction with the other
// two components each +0 or -0, every direction in a coordinate plane's diagonals with the third
// component +0 or -0, and tiny components on either side of inv_dir's 1e-20 clamp
std::vector<Ray> directions() {
    std::vector<Ray> out;
    auto add = [&](float x, float y, float z) { out.push_back(Ray{{0.f, 0.f, 0.f}, {x, y, z}}); };
    const float sg[2] = {1.f, -1.f};
    for (float sx : sg) for (float sy : sg) for (float sz : sg) {
        add(sx * 0.57f, sy * 0.61f, sz * 0.55f);
        add(sx * 0.999f, sy * 0.03f, sz * 0.02f);
        add(sx * 1e-3f, sy * 0.8f, sz * 0.6f);
        add(sx * 1e-21f, sy * 1e-19f, sz * 1.f);          // below / above the clamp
        add(sx * 1e-30f, sy * 1.f, sz * 1e-38f);
    }
    for (int a = 0; a < 3; ++a)
        for (float s : sg) for (float za : sg) for (float zb : sg) {
            float d[3];
            d[a] = s; d[(a + 1) % 3] = za * 0.f; d[(a + 2) % 3] = zb * 0.f;   // two zero components
            add(d[0], d[1], d[2]);
        }
    for (int a = 0; a < 3; ++a)
        for (float s : sg) for (float sb : sg) for (float z : sg) {
            float d[3];
            d[a] = s * 0.6f; d[(a + 1) % 3] = sb * 0.8f; d[(a + 2) % 3] = z * 0.f;   // one zero component
            add(d[0], d[1], d[2]);
        }
    return out;
}

void world(const char* name, const om_world* w, const std::vector<Ray>& dirs) {
    om::FrozenWorld fw;
    w->freeze(fw);
    const om::TreePlan p = om::plan_trees(fw);
    EXPECT(p.b2_ok && p.b2_lds_bytes != 0u);              // a world of this program stages its BVH2 in LDS
    constexpr uint32_t scale = OM_B2_NODE_STRIDE / 16u;
    std::vector<OmBvh2NodeS> staged;
    uint32_t inverted = 0, infinite = 0;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (const OmBvh2Node& n : fw.b2nodes) {
        const OmBvh2NodeS s = b2s_order(n, scale);
        for (uint32_t k = 0; k < 2u; ++k)
            for (uint32_t a = 0; a < 3u; ++a) {
                const float l = OM_B2_LO(n, k, a), h = OM_B2_HI(n, k, a);
                const float* t = s.p + b2s_pair(k, a, 0u);
                EXPECT(t[0] <= t[1]);
                EXPECT(bits(t[2]) == bits(t[0]));
                EXPECT((bits(t[0]) == bits(l) && bits(t[1]) == bits(h)) || (bits(t[0]) == bits(h) && bits(t[1]) == bits(l)));
                if (h < l) { ++inverted; EXPECT(t[0] == -INFINITY && t[1] == INFINITY && l == INFINITY && h == -INFINITY); }
                if (std::isinf(l) || std::isinf(h)) ++infinite;
                if (std::isfinite(l) && std::isfinite(h)) { lo[a] = std::fmin(lo[a], l); hi[a] = std::fmax(hi[a], h); }
            }
        const uint32_t c[2] = {n.c0, n.c1}, sc[2] = {s.c0, s.c1};
        for (int k = 0; k < 2; ++k) {
            if (c[k] < OM_LEAF) EXPECT(sc[k] == c[k] * scale && sc[k] < OM_LEAF && c[k] < fw.b2nodes.size());
            else EXPECT(sc[k] == c[k]);
        }
        staged.push_back(s);
    }
    // a one-leaf tree's second child is the builder's only inverted box (om_bvh.cpp emit_bvh2)
    EXPECT(inverted == (fw.b2nodes.size() == 1u && fw.b2leaves.size() == 2u && (fw.b2leaves[1] & 255u) == 0u ? 3u : 0u));

    Tally t;
    Lcg g{0x0DDB1A5E5BA5Eull ^ (uint64_t)fw.b2nodes.size()};
    const float tmin = 0.001f;
    const float closests[3] = {100.0f, 3.0f, 0.25f};
    // rays shared by every node: each direction from the scene's centre, from outside it and from
    // random points of its box; random rays
    std::vector<Ray> shared;
    for (const Ray& d : dirs) {
        Ray r = d;
        for (int a = 0; a < 3; ++a) r.o[a] = 0.5f * (lo[a] + hi[a]);
        shared.push_back(r);
        for (int a = 0; a < 3; ++a) r.o[a] = hi[a] + 1.0f;
        shared.push_back(r);
        for (int a = 0; a < 3; ++a) r.o[a] = lo[a] + (hi[a] - lo[a]) * g.uni();
        shared.push_back(r);
    }
    for (int k = 0; k < 96; ++k) {
        Ray r;
        for (int a = 0; a < 3; ++a) { r.o[a] = lo[a] + (hi[a] - lo[a]) * (g.uni() * 1.2f - 0.1f); r.d[a] = g.sym(); }
        shared.push_back(r);
    }
    for (size_t i = 0; i < fw.b2nodes.size(); ++i) {
        const OmBvh2Node& N = fw.b2nodes[i];
        const OmBvh2NodeS& S = staged[i];
        for (size_t k = 0; k < shared.size(); ++k) check(N, S, shared[k], tmin, closests[k % 3u], t);
        // per node: every direction from a corner of child 0's box, the opposite corner of child
        // 1's (origins on the planes themselves: exact zeros in the slab values), and a point
        // inside child 0's box
        for (size_t k = 0; k < dirs.size(); ++k) {
            Ray r = dirs[k];
            for (int a = 0; a < 3; ++a) r.o[a] = std::isfinite(N.lo0[a]) ? N.lo0[a] : 0.f;
            check(N, S, r, tmin, closests[k % 3u], t);
            for (int a = 0; a < 3; ++a) r.o[a] = std::isfinite(N.hi1[a]) ? N.hi1[a] : 0.f;
            check(N, S, r, tmin, closests[(k + 1u) % 3u], t);
            for (int a = 0; a < 3; ++a) r.o[a] = std::isfinite(N.lo0[a]) ? N.lo0[a] + (N.hi0[a] - N.lo0[a]) * g.uni() : 0.f;
            check(N, S, r, tmin, closests[(k + 2u) % 3u], t);
        }
    }
    EXPECT(t.mismatch == 0u);
    std::printf("{\"world\": \"%s\", \"b2nodes\": %zu, \"inverted_axes\": %u, \"infinite_planes\": %u, \"directions\": %zu, "
                "\"tests\": %llu, \"mismatch\": %llu, \"zero_sign\": %llu, \"both\": %llu, \"one\": %llu, \"none\": %llu, \"swaps\": %llu}\n",
                name, fw.b2nodes.size(), inverted, infinite, dirs.size(), (unsigned long long)t.tests, (unsigned long long)t.mismatch,
                (unsigned long long)t.zero_sign, (unsigned long long)t.both, (unsigned long long)t.one, (unsigned long long)t.none,
                (unsigned long long)t.swaps);
}

}  // namespace

int main(int argc, char** argv) {
    if ((argc - 1) % 2 != 0) {
        std::fprintf(stderr, "usage: ordered_planes [NAME FILE ...]\n");
        return 2;
    }
    const std::vector<Ray> dirs = directions();
    // the normalisation itself on planes no builder emits: NaN stays in both, zeros keep lo <= hi
    {
        OmBvh2Node n{};
        n.lo0[0] = NAN; n.hi0[0] = 1.f; n.lo0[1] = 2.f; n.hi0[1] = NAN; n.lo0[2] = 0.f; n.hi0[2] = -0.f;
        n.lo1[0] = 3.f; n.hi1[0] = -3.f; n.c0 = 7u; n.c1 = OM_LEAF | 7u;
        const OmBvh2NodeS s = b2s_order(n, 5u);
        EXPECT(std::isnan(s.p[0]) && std::isnan(s.p[1]) && std::isnan(s.p[2]));
        EXPECT(std::isnan(s.p[3]) && std::isnan(s.p[4]) && std::isnan(s.p[5]));
        EXPECT(s.p[6] == 0.f && s.p[7] == 0.f);
        EXPECT(s.p[9] == -3.f && s.p[10] == 3.f && s.p[11] == -3.f);
        EXPECT(s.c0 == 35u && s.c1 == (OM_LEAF | 7u));
        // a NaN plane: both forms visit the box
        Tally t;
        for (const Ray& d : dirs) check(n, s, d, 0.001f, 100.f, t);
        EXPECT(t.mismatch == 0u && t.none == 0u);
    }
    const char* lds_worlds[] = {"g0", "g11", "g15", "g16", "c7x17", "c7x18", "c8x17"};
    for (const TreeScene& sc : kTreeScenes) {
        bool use = false;
        for (const char* n : lds_worlds) use = use || std::strcmp(n, sc.name) == 0;
        if (!use) continue;
        om_world* w = nullptr;
        EXPECT(om_world_create(&w) == OM_OK);
        EXPECT(build_tree_scene(sc, w));
        world(sc.name, w, dirs);
        om_world_destroy(w);
    }
    for (int a = 1; a + 1 < argc; a += 2) {
        om_world* w = nullptr;
        EXPECT(om_world_create(&w) == OM_OK);
        if (!load(argv[a + 1], w)) { std::fprintf(stderr, "FAIL cannot load %s\n", argv[a + 1]); ++g_fail; }
        else world(argv[a], w, dirs);
        om_world_destroy(w);
    }
    if (g_fail) std::fprintf(stderr, "%d checks failed\n", g_fail);
    return g_fail == 0 ? 0 : 1;
}
