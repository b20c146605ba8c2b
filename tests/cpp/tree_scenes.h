// tree_scenes.h — the named worlds of tree_regimes.cpp, built on the host (frozen_digest.cpp
// freezes the same ones).
//
// `g<N>` is random_scene(0x5EED, grid_half=N) (`x`: extras=False), `c<P>x<S>` a field of S x S
// clusters of P spheres over the ground sphere (tests/scenes_common.py cluster_world builds the same
// world in the same order), `line4000` an adversarial input for the builder's depth bound (not
// rendered); `g11t` (S-full), `marched` and `basic` are the other shipped scenes.
#pragma once
#include <cstdint>
#include <cstring>

#include "ottomarcher.h"

// the tie scene's palette (tests/scenes_common.py)
inline om_material palette(uint32_t n) {
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
inline bool cluster_world(om_world* w, uint32_t per, uint32_t side) {
    uint32_t n = 0;
    om_material m = palette(n++);
    const float g[3] = {0.f, -1000.f, 0.f};
    bool ok = om_world_add_sphere_radius(w, g, 1000.f, &m) == OM_OK;
    const float half = (float)side * 0.5f;
    for (uint32_t a = 0; a < side; ++a)
        for (uint32_t b = 0; b < side; ++b)
            for (uint32_t k = 0; k < per; ++k) {
                const float dk = 0.01f * (float)k;
                const float c[3] = {((float)a - half) + dk, 0.2f, ((float)b - half) - dk};
                const float r = 0.2f + 0.005f * (float)k;
                m = palette(n++);
                ok = om_world_add_sphere_radius(w, c, r, &m) == OM_OK && ok;
            }
    return ok;
}

// 4000 spheres on a line, spacing and radius growing geometrically (x_i = 250 * 1.0015^i, the
// radius a quarter of the gap): a SAH split peels the far end off level after level.  The radii run
// from 0.094 to 38, inside what the builder keeps in its trees (a sphere whose margin cannot cover
// its test's rounding from 16 away, and a bound above 200, both stay outside them);
// the line spans e^6 where it once spanned e^16 (ratio 1.004 from x = 1e-3), so the peeling is milder.
inline bool line_world(om_world* w) {
    double x = 250.0;
    bool ok = true;
    for (uint32_t i = 0; i < 4000u; ++i) {
        const double gap = x * 0.0015;
        const float c[3] = {(float)x, 0.f, 0.f};
        const om_material m = palette(i);
        ok = om_world_add_sphere_radius(w, c, (float)(0.25 * gap), &m) == OM_OK && ok;
        x += gap;
    }
    return ok;
}

// every named world, in the order tree_regimes reports them (g11t, marched, basic: the other
// shipped scenes, reported but not regime worlds)
struct TreeScene { const char* name; char kind; uint32_t a; int32_t b; };   // g: flags, grid; c: per, side
constexpr TreeScene kTreeScenes[] = {
    {"g0x", 'g', 2u, 0}, {"g0", 'g', 0u, 0}, {"g11", 'g', 0u, 11}, {"g15", 'g', 0u, 15}, {"g16", 'g', 0u, 16},
    {"g17", 'g', 0u, 17}, {"g22", 'g', 0u, 22}, {"g23", 'g', 0u, 23}, {"g50x", 'g', 2u, 50}, {"g91x", 'g', 2u, 91},
    {"c7x17", 'c', 7u, 17}, {"c7x18", 'c', 7u, 18}, {"c8x17", 'c', 8u, 17},
    {"g11t", 'g', 1u, 11}, {"marched", 'm', 0u, 0}, {"basic", 'b', 0u, 0}, {"line4000", 'l', 0u, 0}};

inline bool build_tree_scene(const TreeScene& s, om_world* w) {
    switch (s.kind) {
        case 'g': return om_world_random_scene(w, 0x5EED, s.a, s.b) == OM_OK;
        case 'c': return cluster_world(w, s.a, (uint32_t)s.b);
        case 'm': return om_world_marched_scene(w) == OM_OK;
        case 'b': return om_world_basic_scene(w) == OM_OK;
        default: return line_world(w);
    }
}
