// wide_regimes.cpp — the wide BVH2 (OmBvh2NodeW: 32-bit child codes) on the host:
// which worlds get it, and that it is the same tree as the 16-bit one (host code only; the
// counterpart of mesh_regimes.cpp for trees around and past the 15-bit codes).
//
// tests/test_wide_regimes.py writes worlds in mesh_common.dump's format (u32 item count, then per
// item a u32 tag; 1 sphere_radius: 4 f32; 2 sphere, 3 cube: 16 f32 local_to_world; 4 mesh: u32 V,
// u32 T, 3V f32, 3T u32) and runs `wide_regimes NAME FILE [NAME FILE ...]`.  Per world this program
// freezes, plans, checks the structure below and prints one JSON line, which the Python side pins:
//   * a world with both trees (b2_ok): b2h and the wide nodes walked in lockstep from the root have
//     bit-equal planes, leaves at the same places and the same record range per leaf;
//   * every world with wide nodes: each record lies in exactly one leaf, every decoded child box
//     contains the srec_box of every record below it, no plane is NaN and none of a non-empty
//     child is infinite, the deepest path is b2w_depth and no leaf holds more than 15 records;
//   * om_world_tree_info reports the plan.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../raytracingoneweekend_amd/csrc/om_bvh.h"
#include "../../raytracingoneweekend_amd/csrc/om_tuning.h"
#include "../../raytracingoneweekend_amd/csrc/om_world.h"
#include "ottomarcher.h"
#include "world_file.h"

namespace {

int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { if (g_fail < 20) std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

struct Range { uint32_t first, count; };
bool wide_leaf(uint32_t c) { return c >= OM_LEAFW; }
Range wide_range(uint32_t c) { return Range{(c & ~OM_LEAFW) >> kLeafCountBits, c & kLeafCountMax}; }
Range narrow_range(const om::FrozenWorld& fw, uint32_t c) {
    if (fw.b2_direct) return Range{(c >> kLeafCountBits) & (kDirectFirst16 - 1u), c & kLeafCountMax};
    const uint32_t l = fw.b2leaves[c & (OM_LEAF - 1u)];
    return Range{l >> 8, l & 255u};
}

// b2h and b2w from the root in lockstep: -> nodes visited
size_t lockstep(const om::FrozenWorld& fw) {
    std::vector<std::pair<uint32_t, uint32_t>> st{{0u, 0u}};
    size_t visited = 0;
    while (!st.empty()) {
        const auto [h, w] = st.back();
        st.pop_back();
        if (h >= fw.b2h.size() || w >= fw.b2w.size()) { EXPECT(!"child index out of range"); break; }
        ++visited;
        const OmBvh2NodeH& H = fw.b2h[h];
        const OmBvh2NodeW& W = fw.b2w[w];
        EXPECT(std::memcmp(H.b, W.b, sizeof H.b) == 0);
        const uint32_t hc[2] = {H.c0, H.c1}, wc[2] = {W.c0, W.c1};
        for (int k = 0; k < 2; ++k) {
            const bool hl = (hc[k] & OM_LEAF) != 0u;
            EXPECT(hl == wide_leaf(wc[k]));
            if (hl != wide_leaf(wc[k])) continue;
            if (hl) {
                const Range a = narrow_range(fw, hc[k]), b = wide_range(wc[k]);
                EXPECT(a.count == b.count && (a.count == 0u || a.first == b.first));
            } else {
                st.push_back({hc[k], wc[k]});
            }
        }
    }
    return visited;
}

struct Walk {
    const om::FrozenWorld& fw;
    std::vector<uint32_t> seen;          // visits per record
    uint32_t depth = 0, max_leaf = 0, leaves = 0, bad_planes = 0, bad_boxes = 0, nodes = 0;
    // child k of node n: checks its decoded box against the records below it; -> their box
    void child(uint32_t n, int k, uint32_t d, float lo[3], float hi[3]) {
        const OmBvh2NodeW& N = fw.b2w[n];
        const uint32_t c = k ? N.c1 : N.c0;
        for (int i = 0; i < 3; ++i) { lo[i] = INFINITY; hi[i] = -INFINITY; }
        if (wide_leaf(c)) {
            const Range r = wide_range(c);
            if (r.count == 0u) return;                       // the empty second child of a one-leaf tree
            ++leaves;
            max_leaf = std::max(max_leaf, r.count);
            for (uint32_t j = 0; j < r.count; ++j) {
                if (r.first + j >= fw.srecs.size()) { EXPECT(!"record index out of range"); return; }
                ++seen[r.first + j];
                const float* b = &fw.srec_box[(size_t)(r.first + j) * 6u];
                for (int i = 0; i < 3; ++i) { lo[i] = std::min(lo[i], b[i]); hi[i] = std::max(hi[i], b[3 + i]); }
            }
        } else {
            if (c >= fw.b2w.size()) { EXPECT(!"node index out of range"); return; }
            node(c, d + 1u, lo, hi);
        }
        for (int i = 0; i < 3; ++i) {
            const float plo = om::half_value(N.b[6 * k + i]), phi = om::half_value(N.b[6 * k + 3 + i]);
            if (!std::isfinite(plo) || !std::isfinite(phi)) ++bad_planes;
            if (!(plo <= lo[i] && phi >= hi[i])) ++bad_boxes;
        }
    }
    void node(uint32_t n, uint32_t d, float lo[3], float hi[3]) {
        ++nodes;
        depth = std::max(depth, d);
        float l0[3], h0[3], l1[3], h1[3];
        child(n, 0, d, l0, h0);
        child(n, 1, d, l1, h1);
        for (int i = 0; i < 3; ++i) { lo[i] = std::min(l0[i], l1[i]); hi[i] = std::max(h0[i], h1[i]); }
    }
};

void report(const char* name, const om_world* w) {
    om::FrozenWorld fw;
    w->freeze(fw);
    const om::TreePlan p = om::plan_trees(fw);
    size_t lock = 0;
    if (p.b2_ok && !fw.b2w.empty()) {
        EXPECT(fw.b2h.size() == fw.b2w.size());
        lock = lockstep(fw);
        EXPECT(lock == fw.b2w.size());
    }
    Walk wk{fw, std::vector<uint32_t>(fw.srecs.size(), 0u)};
    uint32_t once = 0;
    if (!fw.b2w.empty()) {
        EXPECT(fw.srec_box.size() == fw.srecs.size() * 6u);
        float lo[3], hi[3];
        wk.node(0u, 1u, lo, hi);
        for (uint32_t s : wk.seen) once += s == 1u ? 1u : 0u;
        EXPECT(once == fw.srecs.size());
        EXPECT(wk.nodes == fw.b2w.size());
        EXPECT(wk.depth == fw.b2w_depth);
        EXPECT(wk.max_leaf == fw.b2_max_leaf && wk.max_leaf <= kLeafCountMax);
        EXPECT(wk.bad_planes == 0u && wk.bad_boxes == 0u);
    }
    om_tree_info ti{};
    EXPECT(om_world_tree_info(w, &ti) == OM_OK);
    EXPECT(ti.records == fw.srecs.size() && ti.always_tested == fw.always2.size());
    EXPECT(ti.b2_nodes == fw.b2nodes.size() && ti.b2_leaves == fw.b2leaves.size() && ti.b2_max_leaf == fw.b2_max_leaf);
    EXPECT(ti.regime == (p.b2_ok ? (p.b2_lds_bytes ? OM_TREE_LDS : OM_TREE_L2) : p.b2w_ok ? OM_TREE_WIDE
                         : fw.bvh.size() <= 1u ? OM_TREE_NONE : OM_TREE_FALLBACK_BVH));
    std::printf("{\"world\": \"%s\", \"prims\": %u, \"triangles\": %u, \"srecs\": %zu, \"always2\": %zu, "
                "\"b2_ok\": %d, \"b2nodes\": %zu, \"b2leaves\": %zu, \"b2_lds_bytes\": %u, \"b2_direct\": %u, "
                "\"b2w_ok\": %d, \"b2w_nodes\": %zu, \"b2w_depth\": %u, \"b2w_stack\": %u, \"max_leaf\": %u, "
                "\"lockstep_nodes\": %zu, \"walk_leaves\": %u, \"records_once\": %u, \"bad_planes\": %u, \"bad_boxes\": %u, "
                "\"regime\": %d, \"lds_bytes\": %u, \"info_depth\": %u, \"wide_stack_bound\": %u}\n",
                name, fw.offsets[om::K_N], fw.offsets[om::K_TRI + 1] - fw.offsets[om::K_TRI], fw.srecs.size(), fw.always2.size(),
                p.b2_ok ? 1 : 0, fw.b2nodes.size(), fw.b2leaves.size(), p.b2_lds_bytes, p.b2_direct, p.b2w_ok ? 1 : 0,
                fw.b2w.size(), fw.b2w_depth, p.b2w_stack, fw.b2_max_leaf, lock, wk.leaves, once, wk.bad_planes, wk.bad_boxes,
                (int)ti.regime, ti.lds_bytes, ti.b2_depth, kB2WideStack);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3 || (argc - 1) % 2 != 0) {
        std::fprintf(stderr, "usage: wide_regimes NAME FILE [NAME FILE ...]\n");
        return 2;
    }
    static_assert(sizeof(OmBvh2NodeW) == 32 && sizeof(om_tree_info) == 32, "layouts");
    for (int a = 1; a + 1 < argc; a += 2) {
        om_world* w = nullptr;
        EXPECT(om_world_create(&w) == OM_OK);
        if (!load(argv[a + 1], w)) { std::fprintf(stderr, "FAIL cannot load %s\n", argv[a + 1]); ++g_fail; }
        else report(argv[a], w);
        om_world_destroy(w);
    }
    // an empty world: no trees, nothing walked
    {
        om_world* w = nullptr;
        EXPECT(om_world_create(&w) == OM_OK);
        om_tree_info ti{};
        EXPECT(om_world_tree_info(w, &ti) == OM_OK && ti.regime == OM_TREE_NONE && ti.records == 0u && ti.lds_bytes == 0u);
        EXPECT(om_world_tree_info(nullptr, &ti) == OM_ERR_INVALID && om_world_tree_info(w, nullptr) == OM_ERR_INVALID);
        om_world_destroy(w);
    }
    return g_fail == 0 ? 0 : 1;
}
