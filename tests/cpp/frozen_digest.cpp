// frozen_digest.cpp — a digest of every member of a frozen world (host code only).
//
// For a change to the builders that must leave the frozen worlds as they are: build this program
// before and after the change, run both over the same worlds and diff the outputs
// (profiles/bvh_stages/ holds such a pair).  Per world it prints one line per FrozenWorld member:
// the member's name, its element count and the 64-bit FNV-1a of its bytes; scalars, counts and
// offsets are printed as values.  Worlds: `frozen_digest [NAME FILE ...]` freezes every named world
// of tree_scenes.h, then the world files given (world_file.h).  No test pins these values.
#include <cstdio>
#include <vector>

#include "../../raytracingoneweekend_amd/csrc/om_world.h"
#include "ottomarcher.h"
#include "tree_scenes.h"
#include "world_file.h"

namespace {

template <class T>
void arr(const char* world, const char* name, const std::vector<T>& v) {
    uint64_t h = 0xcbf29ce484222325ull;
    const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    std::printf("%s %s %zu %016llx\n", world, name, v.size(), (unsigned long long)h);
}
void val(const char* world, const char* name, uint32_t v) { std::printf("%s %s = %u\n", world, name, v); }

void digest(const char* world, const om_world* w) {
    om::FrozenWorld fw;
    w->freeze(fw);
    // every member of FrozenWorld, in its order: a new member is added here with it
#define ARR(m) arr(world, #m, fw.m)
#define VAL(m) val(world, #m, fw.m)
    ARR(sph_test); ARR(cube_test); ARR(sph_hit); ARR(cube_hit); ARR(sph_bound); ARR(cube_bound); ARR(tri); ARR(para);
    ARR(plane); ARR(msph); ARR(mbox); ARR(mtor); ARR(msdf); ARR(msdf_ops); ARR(mats); ARR(bloom);
    ARR(bvh); ARR(bvh_prims); ARR(always);
    ARR(snodes); ARR(srecs); VAL(n_srec_bary); ARR(always2); ARR(always2_rec); ARR(srec_box);
    ARR(b2nodes); ARR(b2h); ARR(b2leaves); VAL(b2_depth); VAL(b2_direct);
    ARR(b2w); VAL(b2w_depth); VAL(b2_max_leaf);
    ARR(b4nodes); ARR(b4h); VAL(b4_depth);
#undef ARR
#undef VAL
    for (int k = 0; k < om::K_N; ++k) std::printf("%s counts[%d] = %u\n", world, k, fw.counts[k]);
    for (int k = 0; k <= om::K_N; ++k) std::printf("%s offsets[%d] = %u\n", world, k, fw.offsets[k]);
}

}  // namespace

int main(int argc, char** argv) {
    if ((argc - 1) % 2 != 0) {
        std::fprintf(stderr, "usage: frozen_digest [NAME FILE ...]\n");
        return 2;
    }
    int fail = 0;
    for (const TreeScene& sc : kTreeScenes) {
        om_world* w = nullptr;
        if (om_world_create(&w) != OM_OK || !build_tree_scene(sc, w)) { std::fprintf(stderr, "FAIL cannot build %s\n", sc.name); ++fail; }
        else digest(sc.name, w);
        om_world_destroy(w);
    }
    for (int a = 1; a + 1 < argc; a += 2) {
        om_world* w = nullptr;
        if (om_world_create(&w) != OM_OK || !load(argv[a + 1], w)) { std::fprintf(stderr, "FAIL cannot load %s\n", argv[a + 1]); ++fail; }
        else digest(argv[a], w);
        om_world_destroy(w);
    }
    return fail == 0 ? 0 : 1;
}
