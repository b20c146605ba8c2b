// mesh_regimes.cpp — which traversal regime each mesh test world lands in, and where its triangles
// are kept (host code only; the mesh counterpart of tree_regimes.cpp).
//
// From OM_BARY_TREE_MIN triangles + parallelograms on, select (om_bvh.cpp) puts them into
// the SBVH / BVH2 / BVH4 leaves as OM_REC_BARY records beside the spheres and cubes; below it they
// stay in always2.  tests/test_mesh_regimes.py builds the worlds of
// tests/mesh_common.py in numpy, writes each to a file (mesh_common.dump: u32 item count, then per
// item a u32 tag; 1 sphere_radius: 4 f32; 2 sphere, 3 cube: 16 f32 local_to_world; 4 mesh: u32 V,
// u32 T, 3V f32, 3T u32) and runs `mesh_regimes NAME FILE [NAME FILE ...]`; this program adds the
// items in order (a mesh through om_world_add_triangles), freezes the world and prints one JSON
// line with its plan, which the Python side pins by name.
//
// Worlds and the regimes they land in (sizes chosen in tests/mesh_common.py):
//   ico2    320 triangles, 324 records   BVH2 staged in LDS, direct leaf codes
//   ico2x2  640 triangles, 644 records   the same; every triangle has an exact duplicate
//   hf48    4608 triangles, 4612 records leaf table (>= 2048 records), tree read through L2 with
//                                        half-precision nodes, one record per leaf
//   below   15 triangles                 no barycentric record in srecs, all 15 in always2 with
//                                        their boxes: the layout of every world before meshes
//   degen   32 triangles + 1 degenerate  the degenerate one in always2 and unbounded, 32 in the tree
// The regime "staged in LDS with a leaf table" needs >= 2048 records in a tree of at most 40 KiB:
// tree_regimes' c7x18 reaches it with 7-sphere clusters that fill 7-record leaves; a mesh's
// triangles do not pile up like that (the SAH builder leaves 1-2 per leaf, so 2048 records take
// > 1000 nodes of 64 B), and no mesh world of this file reaches it.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../raytracingoneweekend_amd/csrc/om_tuning.h"
#include "../../raytracingoneweekend_amd/csrc/om_world.h"
#include "ottomarcher.h"
#include "world_file.h"

namespace {

int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

void report(const char* name, const om_world* w) {
    om::FrozenWorld fw;
    w->freeze(fw);
    const om::TreePlan p = om::plan_trees(fw);
    const uint32_t t0 = fw.offsets[om::K_TRI], t1 = fw.offsets[om::K_TRI + 1];
    // barycentric records of the leaves; triangles of always2, with a box / unbounded
    uint32_t rec_bary = 0, rec_other = 0, max_leaf = 0, mixed = 0, always_tri_boxed = 0, always_tri_unbounded = 0;
    bool nonfinite = false;
    for (const OmAffineTest& r : fw.srecs) {
        uint32_t tag;
        std::memcpy(&tag, &r.pad, 4);
        if (tag & OM_REC_BARY) { ++rec_bary; EXPECT((tag & OM_REC_GI) >= t0 && (tag & OM_REC_GI) < t1); } else ++rec_other;
    }
    for (uint32_t l : fw.b2leaves) {
        max_leaf = std::max(max_leaf, l & 255u);
        uint32_t nb = 0;
        for (uint32_t k = 0; k < (l & 255u); ++k) {
            uint32_t tag;
            std::memcpy(&tag, &fw.srecs[(l >> 8) + k].pad, 4);
            nb += (tag & OM_REC_BARY) ? 1u : 0u;
        }
        mixed += (nb != 0u && nb != (l & 255u)) ? 1u : 0u;
    }
    for (const OmAlwaysRec& a : fw.always2_rec) {
        if (a.gi < t0 || a.gi >= t1) continue;
        if (a.lo[0] == -INFINITY) ++always_tri_unbounded; else ++always_tri_boxed;
    }
    // no cull may see a non-finite plane: nodes of every tree, the always2 boxes (+-inf = unbounded is fine)
    for (const OmSkipNode& n : fw.snodes)
        for (int i = 0; i < 3; ++i) nonfinite = nonfinite || !std::isfinite(n.lo[i]) || !std::isfinite(n.hi[i]);
    for (const OmAlwaysRec& a : fw.always2_rec)
        for (int i = 0; i < 3; ++i) nonfinite = nonfinite || std::isnan(a.lo[i]) || std::isnan(a.hi[i]);
    EXPECT(rec_bary == fw.n_srec_bary);
    EXPECT(fw.srec_box.size() == fw.srecs.size() * 6u);
    std::printf("{\"world\": \"%s\", \"prims\": %u, \"triangles\": %u, \"srecs\": %zu, \"rec_bary\": %u, \"rec_other\": %u, "
                "\"always2\": %zu, \"always_tri_boxed\": %u, \"always_tri_unbounded\": %u, \"nonfinite_planes\": %d, "
                "\"b2_ok\": %d, \"b2nodes\": %zu, \"b2leaves\": %zu, \"b2_depth\": %u, \"b2_direct\": %u, \"b2_lds_bytes\": %u, "
                "\"max_leaf\": %u, \"mixed_leaves\": %u, \"b4_ok\": %d, \"b4_lds_bytes\": %u, \"snodes\": %zu, \"lds_bytes\": %u, "
                "\"bary_tree_min\": %d}\n",
                name, fw.offsets[om::K_N], t1 - t0, fw.srecs.size(), rec_bary, rec_other, fw.always2.size(), always_tri_boxed,
                always_tri_unbounded, nonfinite ? 1 : 0, p.b2_ok ? 1 : 0, fw.b2nodes.size(), fw.b2leaves.size(), fw.b2_depth,
                p.b2_direct, p.b2_lds_bytes, max_leaf, mixed, p.b4_ok ? 1 : 0, p.b4_lds_bytes, fw.snodes.size(), p.lds_bytes,
                (int)OM_BARY_TREE_MIN);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3 || (argc - 1) % 2 != 0) {
        std::fprintf(stderr, "usage: mesh_regimes NAME FILE [NAME FILE ...]\n");
        return 2;
    }
    for (int a = 1; a + 1 < argc; a += 2) {
        om_world* w = nullptr;
        EXPECT(om_world_create(&w) == OM_OK);
        if (!load(argv[a + 1], w)) { std::fprintf(stderr, "FAIL cannot load %s\n", argv[a + 1]); ++g_fail; }
        else report(argv[a], w);
        om_world_destroy(w);
    }
    // the bulk call's contract on the host (tests/test_mesh_api.py checks it through the library)
    {
        om_world* w = nullptr;
        EXPECT(om_world_create(&w) == OM_OK);
        const om_material m = om_material_lambertian(0.5f, 0.5f, 0.5f);
        const float v[9] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f};
        const uint32_t good[3] = {0u, 1u, 2u}, bad[6] = {0u, 1u, 2u, 0u, 1u, 3u};
        uint32_t c[8];
        EXPECT(om_world_add_triangles(w, v, 3u, bad, 2u, &m) == OM_ERR_INVALID);
        EXPECT(om_world_counts(w, c) == OM_OK && c[2] == 0u);
        EXPECT(om_world_add_triangles(w, nullptr, 0u, nullptr, 0u, &m) == OM_OK);
        EXPECT(om_world_add_triangles(w, v, 3u, good, 1u, &m) == OM_OK);
        EXPECT(om_world_counts(w, c) == OM_OK && c[2] == 1u);
        om_world_destroy(w);
    }
    return g_fail == 0 ? 0 : 1;
}
