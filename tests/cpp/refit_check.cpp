// refit_check.cpp — the refit of om_update_triangles on the host (tests/test_refit_host.py; host code
// only): the OM_HD functions of om_refit.h that the kernels of om_refit.hip run one thread per
// element, looped here over a frozen world and its refit tables.
//
//   refit_check NAME ORIGINAL MOVED FIRST ...
// ORIGINAL and MOVED are world files (world_file.h) that differ in the vertices of their last mesh,
// whose first triangle is triangle FIRST of the world.  Per world:
//   (a) an update with the original vertices leaves every array of every layout byte-identical to
//       the freeze's;
//   (b) after an update with the moved vertices every rewritten OmBary equals the record of a fresh
//       freeze of the moved world byte for byte, every box of every layout (walked through the
//       layout's own child codes) contains the fresh freeze's boxes of all records beneath it, and
//       each decoded half plane lies outside the f32 plane it was rounded from;
//   (c) a collapsed face (repeated index) takes the all-covering box in the leaf-record tree, is
//       counted, and no plane anywhere is NaN;
//   (d) a NaN vertex: every face on it is counted and takes the covering box in the leaf-record tree;
//       records and primitive boxes equal those of a fresh freeze of the same world; no plane is NaN.
// One JSON line per world; FAIL lines and exit code 1 when a check fails.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../raytracingoneweekend_amd/csrc/om_bvh.h"
#include "../../raytracingoneweekend_amd/csrc/om_world.h"
#include "ottomarcher.h"
#include "world_file.h"

using namespace om;

namespace {

int g_fail = 0;
void fail(const char* world, const std::string& what) { std::printf("FAIL %s: %s\n", world, what.c_str()); ++g_fail; }

// the last mesh of a world file
bool last_mesh(const char* path, std::vector<float>& v, std::vector<uint32_t>& f) {
    std::FILE* fh = std::fopen(path, "rb");
    if (!fh) return false;
    uint32_t n = 0;
    bool ok = read_exact(fh, &n, 4);
    for (uint32_t k = 0; ok && k < n; ++k) {
        uint32_t tag = 0;
        ok = read_exact(fh, &tag, 4);
        if (!ok) break;
        if (tag == 4u) {
            uint32_t nv = 0, nt = 0;
            ok = read_exact(fh, &nv, 4) && read_exact(fh, &nt, 4) && nv <= (1u << 24) && nt <= (1u << 24);
            if (!ok) break;
            v.assign((size_t)nv * 3u, 0.0f); f.assign((size_t)nt * 3u, 0u);
            ok = read_exact(fh, v.data(), v.size() * 4u) && read_exact(fh, f.data(), f.size() * 4u);
        } else {
            float skip[16];
            const size_t bytes = tag == 1u ? 16u : (tag == 2u || tag == 3u) ? 64u : (tag == 5u || tag == 6u) ? 36u : 0u;
            ok = bytes != 0u && read_exact(fh, skip, bytes);
        }
    }
    std::fclose(fh);
    return ok && !f.empty();
}

struct Frozen {
    om_world* w = nullptr;
    FrozenWorld fw;
    RefitTables rt;
    ~Frozen() { om_world_destroy(w); }
    bool load_file(const char* path) {
        if (om_world_create(&w) != OM_OK || !load(path, w)) return false;
        w->freeze(fw, &rt);
        return true;
    }
};

struct Info { uint32_t unbounded = 0, skipped = 0; };

// om_update_triangles on the host copies: k_triangles' body per triangle, then refit_host
Info update(Frozen& z, uint32_t first, const std::vector<float>& v, const std::vector<uint32_t>& f) {
    Info info;
    const uint32_t n_vertices = (uint32_t)(v.size() / 3u), n_tri = (uint32_t)(f.size() / 3u);
    for (uint32_t k = 0; k < n_tri; ++k) {
        const uint32_t i0 = f[3u * k], i1 = f[3u * k + 1u], i2 = f[3u * k + 2u];
        if (i0 >= n_vertices || i1 >= n_vertices || i2 >= n_vertices) { ++info.skipped; continue; }
        const uint32_t t = first + k, gi = z.rt.tri_first + t;
        OmBary rec;
        float planes[6], old[6], now[6];
        const int ok = refit_triangle(&v[3u * i0], &v[3u * i1], &v[3u * i2], rec, planes);
        z.fw.tri[t] = rec;
        float* pb = &z.rt.prim_box[6u * (size_t)gi];
        for (int i = 0; i < 6; ++i) old[i] = pb[i];
        refit_triangle_box(ok, planes, old, now);
        for (int i = 0; i < 6; ++i) pb[i] = now[i];
        const uint32_t r = z.rt.tri_rec[t];
        if (r != kRefitNoNode) z.rt.titems[r] = refit_triangle_item(ok, gi, z.rt.covering);
        if (ok != (kRefitRecOk | kRefitBoxOk)) ++info.unbounded;
    }
    FrozenWorld& fw = z.fw;
    RefitArrays a{};
    a.bvh = fw.bvh.data(); a.bvh_prims = fw.bvh_prims.data(); a.n_bvh = (uint32_t)fw.bvh.size();
    a.snodes = fw.snodes.data(); a.b2nodes = fw.b2nodes.data(); a.b2h = fw.b2h.data(); a.b2w = fw.b2w.data();
    a.n_b2 = (uint32_t)fw.b2nodes.size(); a.n_b2h = (uint32_t)fw.b2h.size(); a.n_b2w = (uint32_t)fw.b2w.size();
    a.b4nodes = fw.b4nodes.data(); a.b4h = fw.b4h.data(); a.n_b4 = (uint32_t)fw.b4nodes.size(); a.n_b4h = (uint32_t)fw.b4h.size();
    a.always2_rec = fw.always2_rec.data(); a.n_always2 = (uint32_t)fw.always2_rec.size();
    refit_host(z.rt, a);
    // the record boxes the tile lists are built from (om_render.hip takes them back the same way)
    for (size_t r = 0; r < z.rt.titems.size(); ++r)
        std::memcpy(&fw.srec_box[6u * r], &z.rt.prim_box[6u * (size_t)z.rt.titems[r]], 24u);
    return info;
}

template <class T>
bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// every array a refit may write, against another frozen world
void expect_identical(const char* world, const FrozenWorld& a, const FrozenWorld& b) {
#define SAME(m) if (!same(a.m, b.m)) fail(world, "identity update changed " #m)
    SAME(tri); SAME(bvh); SAME(snodes); SAME(srecs); SAME(always2_rec); SAME(srec_box); SAME(b2nodes); SAME(b2h); SAME(b2w);
    SAME(b4nodes); SAME(b4h); SAME(b2leaves); SAME(bvh_prims);
#undef SAME
}

struct B6 { float b[6]; };
B6 none() { B6 x; box_none(x.b); return x; }
B6 uni(const B6& p, const B6& q) { B6 r; box_union(p.b, q.b, r.b); return r; }
bool contains(const float* lo, const float* hi, const B6& in) {
    if (box_is_none(in.b)) return true;
    for (int i = 0; i < 3; ++i) if (!(lo[i] <= in.b[i] && hi[i] >= in.b[3 + i])) return false;
    return true;
}

// walks every layout through its own child codes; `box[gi]`: the fresh freeze's box of a primitive
struct Walker {
    const char* world; const FrozenWorld& fw; const std::vector<float>& box; uint64_t checked = 0;
    B6 prim(uint32_t gi) const { B6 x; std::memcpy(x.b, &box[6u * (size_t)gi], 24u); return x; }
    B6 records(uint32_t first, uint32_t cnt) const {
        B6 u = none();
        for (uint32_t k = 0; k < cnt; ++k) {
            uint32_t tag;
            std::memcpy(&tag, &fw.srecs[first + k].pad, 4);
            u = uni(u, prim(tag & OM_REC_GI));
        }
        return u;
    }
    void need(bool ok, const char* layout, uint32_t node) {
        ++checked;
        if (!ok) fail(world, std::string(layout) + " node " + std::to_string(node) + " does not contain what is beneath it");
    }
    B6 global(uint32_t n) {
        const OmBvhNode& N = fw.bvh[n];
        B6 u = none();
        if (N.left < 0) { for (uint32_t k = 0; k < (uint32_t)N.right; ++k) u = uni(u, prim(fw.bvh_prims[(uint32_t)(-N.left - 1) + k])); }
        else u = uni(global((uint32_t)N.left), global((uint32_t)N.right));
        need(contains(N.lo, N.hi, u), "bvh", n);
        return u;
    }
    B6 skip(uint32_t& i) {                                  // the subtree at snode i; i moves past it
        const uint32_t at = i;
        const OmSkipNode N = fw.snodes[at];
        B6 u = none();
        ++i;
        if (N.leaf != 0xFFFFFFFFu) u = records(N.leaf >> 8, N.leaf & 255u);
        else while (i < N.skip) u = uni(u, skip(i));
        if (i != N.skip) fail(world, "snodes: a subtree does not end at its skip link");
        need(contains(N.lo, N.hi, u), "snodes", at);
        return u;
    }
    B6 leaf16(uint32_t code) const {
        const uint32_t v = code & ~OM_LEAF;
        if (fw.b2_direct) return records(v >> kLeafCountBits, v & kLeafCountMax);
        return records(fw.b2leaves[v] >> 8, fw.b2leaves[v] & 255u);
    }
    B6 b2f(uint32_t n) {
        const OmBvh2Node& N = fw.b2nodes[n];
        B6 u = none();
        for (int k = 0; k < 2; ++k) {
            const uint32_t c = k ? N.c1 : N.c0;
            const B6 in = (c & OM_LEAF) ? leaf16(c) : b2f(c);
            need(contains(k ? N.lo1 : N.lo0, k ? N.hi1 : N.hi0, in), "b2nodes", n);
            u = uni(u, in);
        }
        return u;
    }
    B6 b2h(uint32_t n) {
        const OmBvh2NodeH& N = fw.b2h[n];
        B6 u = none();
        for (int k = 0; k < 2; ++k) {
            const uint32_t c = k ? N.c1 : N.c0;
            const B6 in = (c & OM_LEAF) ? leaf16(c) : b2h(c);
            float lo[3], hi[3];
            for (int i = 0; i < 3; ++i) { lo[i] = half_value(N.b[6 * k + i]); hi[i] = half_value(N.b[6 * k + 3 + i]); }
            need(contains(lo, hi, in), "b2h", n);
            u = uni(u, in);
        }
        return u;
    }
    B6 b2w(uint32_t n) {
        const OmBvh2NodeW& N = fw.b2w[n];
        B6 u = none();
        for (int k = 0; k < 2; ++k) {
            const uint32_t c = k ? N.c1 : N.c0;
            const uint32_t v = c & ~OM_LEAFW;
            const B6 in = (c & OM_LEAFW) ? records(v >> kLeafCountBits, v & kLeafCountMax) : b2w(c);
            float lo[3], hi[3];
            for (int i = 0; i < 3; ++i) { lo[i] = half_value(N.b[6 * k + i]); hi[i] = half_value(N.b[6 * k + 3 + i]); }
            need(contains(lo, hi, in), "b2w", n);
            u = uni(u, in);
        }
        return u;
    }
    B6 b4(uint32_t n, bool half) {
        B6 u = none();
        for (int k = 0; k < 4; ++k) {
            const uint16_t c = half ? fw.b4h[n].child[k] : fw.b4nodes[n].child[k];
            if (c == OM_EMPTY) continue;
            const B6 in = (c & OM_LEAF) ? leaf16(c) : b4(c, half);
            float lo[3], hi[3];
            if (half) {
                const uint16_t* b = fw.b4h[n].b;
                lo[0] = half_value(b[k]); lo[1] = half_value(b[4 + k]); lo[2] = half_value(b[8 + k]);
                hi[0] = half_value(b[12 + k]); hi[1] = half_value(b[16 + k]); hi[2] = half_value(b[20 + k]);
            } else {
                const OmBvh4Node& N = fw.b4nodes[n];
                lo[0] = N.lox[k]; lo[1] = N.loy[k]; lo[2] = N.loz[k]; hi[0] = N.hix[k]; hi[1] = N.hiy[k]; hi[2] = N.hiz[k];
            }
            need(contains(lo, hi, in), half ? "b4h" : "b4nodes", n);
            u = uni(u, in);
        }
        return u;
    }
    void all() {
        if (!fw.bvh.empty()) global(0u);
        if (!fw.snodes.empty()) { uint32_t i = 0; skip(i); }
        if (!fw.b2nodes.empty() && fw.b2nodes.size() < kCode16Limit && fw.b2leaves.size() < kCode16Limit) { b2f(0u); b2h(0u); }
        if (!fw.b2w.empty()) b2w(0u);
        if (!fw.b4nodes.empty()) { b4(0u, false); b4(0u, true); }
    }
};

// each half plane outside the f32 plane of the same slot
uint64_t halves_outside(const char* world, const FrozenWorld& fw, const RefitTables& rt) {
    uint64_t n = 0;
    auto lo_ok = [&](uint16_t h, float x) { ++n; return half_value(h) <= x; };
    auto hi_ok = [&](uint16_t h, float x) { ++n; return half_value(h) >= x; };
    bool ok = true;
    for (size_t i = 0; i < fw.b2nodes.size(); ++i)
        for (int k = 0; k < 2; ++k)
            for (int a = 0; a < 3; ++a) {
                const float lo = OM_B2_LO(fw.b2nodes[i], k, a), hi = OM_B2_HI(fw.b2nodes[i], k, a);
                if (i < fw.b2h.size()) ok = ok && lo_ok(fw.b2h[i].b[6 * k + a], lo) && hi_ok(fw.b2h[i].b[6 * k + 3 + a], hi);
                if (i < fw.b2w.size()) ok = ok && lo_ok(fw.b2w[i].b[6 * k + a], lo) && hi_ok(fw.b2w[i].b[6 * k + 3 + a], hi);
            }
    for (size_t i = 0; i < fw.b4h.size(); ++i)
        for (int k = 0; k < 4; ++k) {
            const uint32_t src = rt.b4h_src[4u * i + k];
            if (src == kRefitNoNode) continue;
            const OmBvhNode& N = rt.tnodes[src];
            const uint16_t* b = fw.b4h[i].b;
            ok = ok && lo_ok(b[k], N.lo[0]) && lo_ok(b[4 + k], N.lo[1]) && lo_ok(b[8 + k], N.lo[2]) && hi_ok(b[12 + k], N.hi[0]) &&
                 hi_ok(b[16 + k], N.hi[1]) && hi_ok(b[20 + k], N.hi[2]);
        }
    if (!ok) fail(world, "a half plane lies inside the f32 plane it was rounded from");
    return n;
}

uint64_t count_nan(const FrozenWorld& fw) {
    uint64_t n = 0;
    auto f = [&](const float* p, size_t k) { for (size_t i = 0; i < k; ++i) n += std::isnan(p[i]) ? 1u : 0u; };
    auto h = [&](const uint16_t* p, size_t k) { for (size_t i = 0; i < k; ++i) n += ((p[i] & 0x7C00u) == 0x7C00u && (p[i] & 0x3FFu)) ? 1u : 0u; };
    for (const auto& x : fw.bvh) { f(x.lo, 3); f(x.hi, 3); }
    for (const auto& x : fw.snodes) { f(x.lo, 3); f(x.hi, 3); }
    for (const auto& x : fw.b2nodes) { f(x.lo0, 3); f(x.hi0, 3); f(x.lo1, 3); f(x.hi1, 3); }
    for (const auto& x : fw.b2h) h(x.b, 12);
    for (const auto& x : fw.b2w) h(x.b, 12);
    for (const auto& x : fw.b4nodes) f(x.lox, 24);
    for (const auto& x : fw.b4h) h(x.b, 24);
    f(fw.srec_box.data(), fw.srec_box.size());
    return n;
}

void check_world(const char* world, const char* orig, const char* moved, uint32_t first) {
    std::vector<float> v0, v1;
    std::vector<uint32_t> f0, f1;
    Frozen pristine, a, b, c, d, fresh;
    if (!last_mesh(orig, v0, f0) || !last_mesh(moved, v1, f1) || f0 != f1 || v0.size() != v1.size() || !pristine.load_file(orig) ||
        !a.load_file(orig) || !b.load_file(orig) || !c.load_file(orig) || !d.load_file(orig) || !fresh.load_file(moved)) {
        fail(world, "cannot load the world files");
        return;
    }
    const uint32_t n_tri = (uint32_t)(f0.size() / 3u);
    if (a.rt.empty() || first + n_tri > a.fw.tri.size()) { fail(world, "no refit tables, or FIRST past the triangles"); return; }

    // (a) the identity update
    const Info ia = update(a, first, v0, f0);
    expect_identical(world, a.fw, pristine.fw);
    if (!same(a.rt.prim_box, pristine.rt.prim_box) || !same(a.rt.tnodes, pristine.rt.tnodes)) fail(world, "identity update changed the kept boxes");

    // (b) the moved mesh against a fresh freeze of the moved world
    const Info ib = update(b, first, v1, f1);
    if (!same(b.fw.tri, fresh.fw.tri)) fail(world, "a rewritten OmBary differs from the fresh freeze's");
    if (same(b.fw.tri, pristine.fw.tri)) fail(world, "the update moved nothing");
    if (!same(b.fw.always2_rec, fresh.fw.always2_rec)) fail(world, "always2_rec differs from the fresh freeze's");
    uint32_t box_diff = 0;
    for (uint32_t k = 0; k < n_tri; ++k) {
        const size_t gi = (size_t)b.rt.tri_first + first + k;
        box_diff += std::memcmp(&b.rt.prim_box[6u * gi], &fresh.rt.prim_box[6u * gi], 24u) != 0 ? 1u : 0u;
    }
    if (box_diff) fail(world, std::to_string(box_diff) + " triangle boxes differ from the fresh freeze's");
    Walker wk{world, b.fw, fresh.rt.prim_box};
    wk.all();
    const uint64_t halves = halves_outside(world, b.fw, b.rt);
    if (count_nan(b.fw)) fail(world, "a NaN plane after the update");

    // (c) a collapsed face: the middle face with its last index repeated
    std::vector<uint32_t> fc = f1;
    uint32_t bad = n_tri / 2u;
    if (fc[3u * bad + 2u] == fc[3u * bad + 1u]) ++bad;       // (already collapsed in the world itself)
    fc[3u * bad + 2u] = fc[3u * bad + 1u];
    const Info ic = update(c, first, v1, fc);
    const uint32_t rec = c.rt.tri_rec[first + bad];
    if (ic.unbounded != ib.unbounded + 1u) fail(world, "the collapsed face is not counted as unbounded");
    if (rec != kRefitNoNode) {
        if (c.rt.titems[rec] != c.rt.covering) fail(world, "the collapsed face did not take the covering box");
        const OmBvhNode& root = c.rt.tnodes[0];
        for (int i = 0; i < 3; ++i)
            if (root.lo[i] != -FLT_MAX || root.hi[i] != FLT_MAX) { fail(world, "the covering box did not reach the root"); break; }
    }
    const uint64_t nans = count_nan(c.fw);
    if (nans) fail(world, std::to_string(nans) + " NaN planes after the collapsed face");

    // (d) a NaN vertex
    std::vector<float> vn = v1;
    const uint32_t nan_vertex = f1[3u * (n_tri / 3u)];
    vn[3u * nan_vertex] = NAN;
    uint32_t on_it = 0;
    for (uint32_t k = 0; k < n_tri; ++k) {
        const bool uses = f1[3u * k] == nan_vertex || f1[3u * k + 1u] == nan_vertex || f1[3u * k + 2u] == nan_vertex;
        const bool collapsed = f1[3u * k + 1u] == f1[3u * k + 2u] || f1[3u * k] == f1[3u * k + 1u] || f1[3u * k] == f1[3u * k + 2u];
        on_it += (uses && !collapsed) ? 1u : 0u;
    }
    const Info id = update(d, first, vn, f1);
    if (on_it == 0u || id.unbounded != ib.unbounded + on_it) fail(world, "the faces on a NaN vertex are not all counted as unbounded");
    // the same change to the host world, frozen afresh: the global BVH takes each of those faces with
    // the box the freeze's own select gives it (bary_box's min / max leave a NaN point out, so the box
    // is finite or empty; only an infinite vertex makes it non-finite), the leaf-record tree keeps
    // them outside; the refit must hold the same boxes and put the covering box before the records
    Frozen nanw;
    if (!nanw.load_file(orig) || om_world_update_triangles(nanw.w, first, vn.data(), (uint32_t)(vn.size() / 3u), f1.data(), n_tri) != OM_OK) {
        fail(world, "cannot build the NaN-vertex world");
        return;
    }
    nanw.w->freeze(nanw.fw, &nanw.rt);
    if (!same(d.fw.tri, nanw.fw.tri)) fail(world, "NaN vertex: a rewritten OmBary differs from the fresh freeze's");
    for (uint32_t k = 0; k < n_tri; ++k) {
        const size_t gi = (size_t)d.rt.tri_first + first + k;
        // (a box that overflows f32 makes the fresh freeze test the triangle outside its global BVH; the
        // refit, which keeps it inside, must then hold the covering box)
        const float* pb = &d.rt.prim_box[6u * gi];
        const bool covering = pb[0] == -FLT_MAX && pb[1] == -FLT_MAX && pb[2] == -FLT_MAX && pb[3] == FLT_MAX && pb[4] == FLT_MAX && pb[5] == FLT_MAX;
        if (!covering && std::memcmp(pb, &nanw.rt.prim_box[6u * gi], 24u) != 0) {
            const float *x = &d.rt.prim_box[6u * gi], *y = &nanw.rt.prim_box[6u * gi];
            fail(world, "NaN vertex: the box of triangle " + std::to_string(k) + " differs from the fresh freeze's: " + std::to_string(x[0]) + " " +
                            std::to_string(x[3]) + " / " + std::to_string(y[0]) + " " + std::to_string(y[3]));
            break;
        }
        if (!(f1[3u * k] == nan_vertex || f1[3u * k + 1u] == nan_vertex || f1[3u * k + 2u] == nan_vertex)) continue;
        const uint32_t r = d.rt.tri_rec[first + k];
        if (r != kRefitNoNode && d.rt.titems[r] != d.rt.covering) { fail(world, "a record on a NaN vertex did not take the covering box"); break; }
    }
    if (count_nan(d.fw)) fail(world, "a NaN plane after the NaN vertex");

    std::printf("{\"world\": \"%s\", \"nan_vertex_faces\": %u, \"triangles\": %u, \"first\": %u, \"in_tree\": %d, \"boxes_checked\": %llu, \"halves_checked\": %llu, "
                "\"unbounded_identity\": %u, \"unbounded_moved\": %u, \"unbounded_collapsed\": %u, \"levels\": %zu}\n",
                world, on_it, n_tri, first, rec != kRefitNoNode ? 1 : 0, (unsigned long long)wk.checked, (unsigned long long)halves, ia.unbounded,
                ib.unbounded, ic.unbounded, b.rt.t_level_off.size() - 1u);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 5 || (argc - 1) % 4 != 0) {
        std::fprintf(stderr, "usage: refit_check NAME ORIGINAL MOVED FIRST ...\n");
        return 2;
    }
    for (int a = 1; a + 3 < argc; a += 4) check_world(argv[a], argv[a + 1], argv[a + 2], (uint32_t)std::strtoul(argv[a + 3], nullptr, 10));
    return g_fail == 0 ? 0 : 1;
}
