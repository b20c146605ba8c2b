// test_query.cpp — the C++ mirror's ray queries (include/ottomarcher.hpp: FrozenHittableList::hit /
// hit_rays, HittableList::material_of), driven by tests/test_cpp_query.py.
//
//   test_query cpu                material_of over a composed world, in id order; its errors and
//                                 the null-argument errors of om_hit_rays* (no device calls)
//   test_query gpu RAYS_IN HITS_OUT
//                                 S-traced frozen through the API; reads n om_ray records, writes the
//                                 n om_hit records of hit_rays (the Python side compares them with
//                                 the CPU oracle); hit() on the first rays must equal the batch
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "ottomarcher.hpp"

using namespace ottomarcher;

static int g_fail = 0;
#define EXPECT(c)                                                                  \
    do {                                                                           \
        if (!(c)) { std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } \
    } while (0)

static bool same_material(const om_material& a, const om_material& b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static int run_cpu() {
    static_assert(sizeof(om_ray) == 24 && sizeof(om_hit) == 32 && sizeof(om_query_params) == 16, "query records");
    // added out of type order: ids follow the type order of hits.rs:370-371, not the order of +=
    const Material plane = Material::new_lambertian(Color(.5f, .5f, .5f)), cube = Material::new_metal_fuzz(Color(.9f, .6f, .2f), .25f),
                   s0 = Material::new_dielectric(1.5f), s1 = Material::new_metal(Color(.7f, .8f, .9f)),
                   msph = Material::new_lambertian(Color(.1f, .2f, .3f));
    HittableList w = HittableList::new_();
    w += MarchedSphere{Point3(0.f, 1.f, 0.f), .5f, msph};
    w += InfinitePlane::new_(Point3(0.f, 0.f, 0.f), Vec3(0.f, 1.f, 0.f), plane);
    w += Sphere::new_with_radius(Point3(0.f, 1.f, -2.f), 1.f, s0);
    w += Cube::new_with_length(Point3(2.f, .5f, 0.f), 1.f, cube);
    w += Sphere::new_with_radius(Point3(3.f, 1.f, -2.f), 1.f, s1);
    const Material* want[] = {&s0, &s1, &cube, &plane, &msph};      // spheres, cubes, planes, marched spheres
    for (uint32_t id = 1; id <= 5; ++id) EXPECT(same_material(w.material_of(id).raw, want[id - 1]->raw));
    for (uint32_t bad : {0u, 6u, 0xFFFFFFFFu}) {
        bool threw = false;
        try { (void)w.material_of(bad); } catch (const Error& e) { threw = e.status == OM_ERR_INVALID; }
        EXPECT(threw);
    }
    om_material m;
    EXPECT(om_world_object_material(nullptr, 1, &m) == OM_ERR_INVALID);
    EXPECT(om_world_object_material(w.handle(), 1, nullptr) == OM_ERR_INVALID);
    const om_query_params q{0.001f, 100.0f, 1024u, 0u};
    om_ray r{{0.f, 0.f, 0.f}, {0.f, 0.f, -1.f}};
    om_hit h;
    EXPECT(om_hit_rays(nullptr, &q, &r, 1, &h) == OM_ERR_INVALID);
    EXPECT(om_hit_rays_device(nullptr, &q, &r, 1, &h, nullptr) == OM_ERR_INVALID);
    EXPECT(om_query_max_grid(nullptr) == 0u);
    if (!g_fail) std::printf("cpu ok\n");
    return g_fail;
}

static int run_gpu(const char* rays_in, const char* hits_out) {
    std::ifstream f(rays_in, std::ios::binary | std::ios::ate);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", rays_in); return 1; }
    const size_t bytes = (size_t)f.tellg();
    std::vector<om_ray> rays(bytes / sizeof(om_ray));
    f.seekg(0);
    f.read((char*)rays.data(), (std::streamsize)(rays.size() * sizeof(om_ray)));
    HittableList w = HittableList::new_();
    check(om_world_random_scene(w.handle(), 0x5EED, 0, 11));
    const Camera cam = Camera::new_(Point3(13.f, 2.f, 3.f), Point3(0.f, 0.f, 0.f), Vec3(0.f, 1.f, 0.f), 20.f, 1.5f, 0.1f, 10.f);
    FrozenHittableList frozen = w.freeze(cam);
    const std::vector<om_hit> hits = frozen.hit_rays(rays, 0.001f, 100.0f);
    EXPECT(hits.size() == rays.size());
    EXPECT(frozen.hit_rays({}, 0.001f, 100.0f).empty());            // n == 0: OM_OK, nothing launched
    size_t n_hit = 0;
    for (size_t i = 0; i < rays.size() && i < 16; ++i) {            // the one-ray form == the batch's record
        om_hit one;
        const bool some = frozen.hit(Vec3(rays[i].orig[0], rays[i].orig[1], rays[i].orig[2]),
                                     Vec3(rays[i].dir[0], rays[i].dir[1], rays[i].dir[2]), 0.001f, 100.0f, one);
        EXPECT(std::memcmp(&one, &hits[i], sizeof one) == 0);
        EXPECT(some == (hits[i].obj != 0u));
        if (some) { ++n_hit; (void)w.material_of(one.obj); }        // every reported id names an object
        else EXPECT(std::isinf(one.t) && one.t > 0.f);
    }
    bool threw = false;                                             // reserved != 0 -> the library's error
    try {
        const om_query_params bad{0.001f, 100.0f, 1024u, 1u};
        om_hit h;
        check(om_hit_rays(frozen.ctx(), &bad, rays.data(), 1u, &h), frozen.ctx());
    } catch (const Error& e) { threw = e.status == OM_ERR_INVALID; }
    EXPECT(threw);
    std::ofstream o(hits_out, std::ios::binary);
    o.write((const char*)hits.data(), (std::streamsize)(hits.size() * sizeof(om_hit)));
    if (!g_fail) std::printf("gpu ok (%zu rays, %zu of the first 16 hit)\n", rays.size(), n_hit);
    return g_fail;
}

int main(int argc, char** argv) {
    try {
        if (argc >= 2 && std::string(argv[1]) == "cpu") return run_cpu() ? 1 : 0;
        if (argc >= 4 && std::string(argv[1]) == "gpu") return run_gpu(argv[2], argv[3]) ? 1 : 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 2;
    }
    std::fprintf(stderr, "usage: test_query cpu | gpu RAYS_IN HITS_OUT\n");
    return 64;
}
