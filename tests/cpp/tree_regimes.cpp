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
// Worlds: `g<N>` is random_scene(0x5EED, grid_half=N) (`x`: extras=False), `c<P>x<S>` a field
// of S x S clusters of P spheres over the ground sphere (tests/scenes_common.py cluster_world
// builds the same world in the same order), `line4000` an adversarial input for the builder's
// depth bound (not rendered); `g11t` (S-full), `marched` and `basic` are the other shipped scenes.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "../../raytracingoneweekend_amd/csrc/om_tuning.h"
#include "../../raytracingoneweekend_amd/csrc/om_world.h"
#include "ottomarcher.h"

namespace {

constexpr uint32_t kB2Stride = OM_B2_NODE_STRIDE;   // LDS slot of a staged f32 BVH2 node (om_wavefront.hip)
constexpr uint32_t kWfBlock = OM_WF_BLOCK;         // lanes per wavefront workgroup (one lane stack each)

int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

// the tie scene's palette (tests/scenes_common.py)
om_material palette(uint32_t n) {
    switch (n % 5u) {
        case 0: return om_material_lambertian(0.8f, 0.3f, 0.2f);
        case 1: return om_material_metal_fuzz(0.7f, 0.8f, 0.9f, 0.1f);
        case 2: return om_material_dielectric(1.5f);
        case 3: return om_material_lambertian(0.1f, 0.6f, 0.2f);
        default: return om_material_metal_fuzz(0.9f, 0.6f, 0.3f, 0.4f);
    }
}

// ground, then side x side clusters of `per` nearly coincident spheres (f32 arithmetic in this
// order: the Python side repeats it)
void cluster_world(om_world* w, uint32_t per, uint32_t side) {
    uint32_t n = 0;
    om_material m = palette(n++);
    const float g[3] = {0.f, -1000.f, 0.f};
    EXPECT(om_world_add_sphere_radius(w, g, 1000.f, &m) == OM_OK);
    const float half = (float)side * 0.5f;
    for (uint32_t a = 0; a < side; ++a)
        for (uint32_t b = 0; b < side; ++b)
            for (uint32_t k = 0; k < per; ++k) {
                const float dk = 0.01f * (float)k;
                const float c[3] = {((float)a - half) + dk, 0.2f, ((float)b - half) - dk};
                const float r = 0.2f + 0.005f * (float)k;
                m = palette(n++);
                EXPECT(om_world_add_sphere_radius(w, c, r, &m) == OM_OK);
            }
}

// 4000 spheres on a line, spacing and radius growing geometrically (x_i = 250 * 1.0015^i, the
// radius a quarter of the gap): a SAH split peels the far end off level after level.  The radii run
// from 0.094 to 38, inside what the builder keeps in its trees (a sphere whose margin cannot cover
// its test's rounding from 16 away, and a bound above 200, both stay outside them);
// the line spans e^6 where it once spanned e^16 (ratio 1.004 from x = 1e-3), so the peeling is milder.
void line_world(om_world* w) {
    double x = 250.0;
    for (uint32_t i = 0; i < 4000u; ++i) {
        const double gap = x * 0.0015;
        const float c[3] = {(float)x, 0.f, 0.f};
        const om_material m = palette(i);
        EXPECT(om_world_add_sphere_radius(w, c, (float)(0.25 * gap), &m) == OM_OK);
        x += gap;
    }
}

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
    struct Grid { const char* name; uint32_t flags; int32_t grid; };
    const Grid grids[] = {{"g0x", 2u, 0}, {"g0", 0u, 0}, {"g11", 0u, 11}, {"g15", 0u, 15}, {"g16", 0u, 16},
                          {"g17", 0u, 17}, {"g22", 0u, 22}, {"g23", 0u, 23}, {"g50x", 2u, 50}, {"g91x", 2u, 91}};
    for (const Grid& g : grids) {
        if (argc > 1 && std::strcmp(argv[1], g.name) != 0) continue;
        om_world* w = nullptr;
        EXPECT(om_world_create(&w) == OM_OK);
        EXPECT(om_world_random_scene(w, 0x5EED, g.flags, g.grid) == OM_OK);
        report(g.name, w);
        om_world_destroy(w);
    }
    struct Cluster { const char* name; uint32_t per, side; };
    const Cluster clusters[] = {{"c7x17", 7u, 17u}, {"c7x18", 7u, 18u}, {"c8x17", 8u, 17u}};
    for (const Cluster& c : clusters) {
        if (argc > 1 && std::strcmp(argv[1], c.name) != 0) continue;
        om_world* w = nullptr;
        EXPECT(om_world_create(&w) == OM_OK);
        cluster_world(w, c.per, c.side);
        report(c.name, w);
        om_world_destroy(w);
    }
    // the other shipped scenes (S-full, S-marched, basic_scene): reported, not regime worlds
    for (const char* name : {"g11t", "marched", "basic"}) {
        if (argc > 1 && std::strcmp(argv[1], name) != 0) continue;
        om_world* w = nullptr;
        EXPECT(om_world_create(&w) == OM_OK);
        if (name[0] == 'g') EXPECT(om_world_random_scene(w, 0x5EED, 1u, 11) == OM_OK);
        else if (name[0] == 'm') EXPECT(om_world_marched_scene(w) == OM_OK);
        else EXPECT(om_world_basic_scene(w) == OM_OK);
        report(name, w);
        om_world_destroy(w);
    }
    if (argc <= 1 || std::strcmp(argv[1], "line4000") == 0) {
        om_world* w = nullptr;
        EXPECT(om_world_create(&w) == OM_OK);
        line_world(w);
        report("line4000", w);
        om_world_destroy(w);
    }
    return g_fail == 0 ? 0 : 1;
}
