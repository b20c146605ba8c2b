// tree_regimes.cpp — which traversal regime each test world lands in (host code only).
//
// The traversal a world gets is decided by a handful of size thresholds (om::plan_trees in
// om_world.h, the builder's leaf and code limits in om_bvh.cpp): BVH2 staged whole in LDS or
// read through L2, direct leaf codes or the leaf table, the max-leaf fallback from ~32k
// primitives, the BVH4 and megakernel LDS cuts.  This program builds the worlds that
// tests/test_gpu_tree_regimes.py renders on the device, freezes them and prints one JSON line
// per world with the planned values, so that tests/test_tree_regimes.py can pin the regime of
// each: retuning a budget, the node stride or a leaf cap then fails there by name instead of
// silently moving a world out of the regime it was chosen for.
//
// The worlds are the named ones of tree_scenes.h.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "../../raytracingoneweekend_amd/csrc/om_tuning.h"
#include "../../raytracingoneweekend_amd/csrc/om_world.h"
#include "ottomarcher.h"
#include "tree_scenes.h"

namespace {

constexpr uint32_t kB2Stride = OM_B2_NODE_STRIDE;   // LDS slot of a staged f32 BVH2 node (om_wavefront.hip)
constexpr uint32_t kWfBlock = OM_WF_BLOCK;         // lanes per wavefront workgroup (one lane stack each)

int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

void report(const char* name, const om_world* w) {
    om::FrozenWorld fw;
    w->freeze(fw);
    const om::TreePlan p = om::plan_trees(fw);
    std::map<uint32_t, uint32_t> hist;
    uint32_t max_first = 0, max_leaf = 0;
    for (uint32_t l : fw.b2leaves) {
        hist[l & 255u]++;
        if (l & 255u) max_first = std::max(max_first, l >> 8);
        max_leaf = std::max(max_leaf, l & 255u);
    }
    std::string h = "{";
    for (const auto& kv : hist) h += (h.size() > 1 ? ", \"" : "\"") + std::to_string(kv.first) + "\": " + std::to_string(kv.second);
    h += "}";
    // what the wavefront's TR_BVH2_LDS launch asks for: padded nodes + leaf table, and one
    // lane stack of b2_stack 16-bit entries per lane
    const uint32_t staged = (uint32_t)(fw.b2nodes.size() * kB2Stride + fw.b2leaves.size() * 4u);
    const uint32_t request = p.b2_lds_bytes ? ((staged + 15u) & ~15u) + kWfBlock * p.b2_stack * 2u : 0u;
    std::printf("{\"world\": \"%s\", \"prims\": %u, \"srecs\": %zu, \"b2_ok\": %d, \"b2nodes\": %zu, \"b2leaves\": %zu, "
                "\"b2_depth\": %u, \"b2_direct\": %u, \"b2_stack\": %u, \"b2_lds_bytes\": %u, \"staged_bytes\": %u, "
                "\"wf_lds_request\": %u, \"leaf_hist\": %s, \"max_leaf\": %u, \"max_first\": %u, "
                "\"b4_ok\": %d, \"b4nodes\": %zu, \"b4_depth\": %u, \"b4_stack\": %u, \"b4_lds_bytes\": %u, "
                "\"snodes\": %zu, \"lds_bytes\": %u}\n",
                name, fw.offsets[om::K_N], fw.srecs.size(), p.b2_ok ? 1 : 0, fw.b2nodes.size(), fw.b2leaves.size(),
                fw.b2_depth, p.b2_direct, p.b2_stack, p.b2_lds_bytes, staged, request, h.c_str(), max_leaf, max_first,
                p.b4_ok ? 1 : 0, fw.b4nodes.size(), fw.b4_depth, p.b4_stack, p.b4_lds_bytes, fw.snodes.size(), p.lds_bytes);
}

}  // namespace

int main(int argc, char** argv) {
    std::printf("{\"budgets\": 1, \"kB2LdsBudget\": %u, \"kB4LdsBudget\": %u, \"kLdsBudget\": %u, \"kB2Stride\": %u, "
                "\"wf_block\": %u}\n", kB2LdsBudget, kB4LdsBudget, kLdsBudget, kB2Stride, kWfBlock);
    for (const TreeScene& sc : kTreeScenes) {
        if (argc > 1 && std::strcmp(argv[1], sc.name) != 0) continue;
        om_world* w = nullptr;
        EXPECT(om_world_create(&w) == OM_OK);
        EXPECT(build_tree_scene(sc, w));
        report(sc.name, w);
        om_world_destroy(w);
    }
    return g_fail == 0 ? 0 : 1;
}
