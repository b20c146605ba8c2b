// world_file.h — the world files the Python tests hand the host drivers (mesh_common.dump,
// scale_common.dump): u32 item count, then per item a u32 tag; 1 sphere_radius: 4 f32; 2 sphere,
// 3 cube: 16 f32 local_to_world; 4 mesh: u32 V, u32 T, 3V f32, 3T u32; 5 triangle, 6 parallelogram:
// three points, 9 f32.  load adds the items to the world in order, every one with the same material.
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ottomarcher.h"

inline bool read_exact(std::FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

inline bool load(const char* path, om_world* w) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    const om_material m = om_material_lambertian(0.5f, 0.5f, 0.5f);
    uint32_t n = 0;
    bool ok = read_exact(f, &n, 4);
    for (uint32_t k = 0; ok && k < n; ++k) {
        uint32_t tag = 0;
        ok = read_exact(f, &tag, 4);
        if (!ok) break;
        if (tag == 1u) {
            float v[4];
            ok = read_exact(f, v, sizeof v) && om_world_add_sphere_radius(w, v, v[3], &m) == OM_OK;
        } else if (tag == 2u || tag == 3u) {
            float l2w[16];
            ok = read_exact(f, l2w, sizeof l2w) &&
                 (tag == 2u ? om_world_add_sphere(w, l2w, &m) : om_world_add_cube(w, l2w, &m)) == OM_OK;
        } else if (tag == 4u) {
            uint32_t nv = 0, nt = 0;
            ok = read_exact(f, &nv, 4) && read_exact(f, &nt, 4) && nv <= (1u << 24) && nt <= (1u << 24);
            if (!ok) break;
            std::vector<float> v((size_t)nv * 3u);
            std::vector<uint32_t> idx((size_t)nt * 3u);
            ok = read_exact(f, v.data(), v.size() * 4u) && read_exact(f, idx.data(), idx.size() * 4u) &&
                 om_world_add_triangles(w, v.data(), nv, idx.data(), nt, &m) == OM_OK;
        } else if (tag == 5u || tag == 6u) {
            float p[9];
            ok = read_exact(f, p, sizeof p) &&
                 (tag == 5u ? om_world_add_triangle(w, p, p + 3, p + 6, &m) : om_world_add_parallelogram(w, p, p + 3, p + 6, &m)) == OM_OK;
        } else {
            ok = false;
        }
    }
    std::fclose(f);
    return ok;
}
