// test_refit.cpp — the C++ mirror's update_triangles / update_info (include/ottomarcher.hpp),
// driven by tests/test_cpp_refit.py.
//
//   test_refit cpu                the statuses of om_*update_triangles that need no device, and
//                                 HittableList::update_triangles == a world built from the new vertices
//   test_refit gpu MESH_IN RAYS_IN HITS_OUT
//                                 MESH_IN: u32 V, u32 T, 3V f32 vertices, 3V f32 moved vertices, 3T u32
//                                 faces.  The mesh over a ground sphere is frozen, moved through
//                                 FrozenHittableList::update_triangles and traced: the n om_hit
//                                 records of hit_rays go to HITS_OUT (the Python side compares them
//                                 with the CPU oracle's for a world built from the moved vertices)
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

static const float kV[12] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
static const float kV2[12] = {0.f, 0.5f, 0.f, 1.5f, 0.f, 0.f, 0.f, 1.f, 0.25f, 0.f, 0.f, 2.f};
static const uint32_t kF[6] = {0u, 1u, 2u, 0u, 2u, 3u};

static bool same_triangle(const HittableList& a, const HittableList& b, uint32_t i) {
    float x[29], y[29];
    return om_world_export(a.handle(), 2, i, x, 29) == OM_OK && om_world_export(b.handle(), 2, i, y, 29) == OM_OK &&
           std::memcmp(x, y, sizeof x) == 0;
}

static int run_cpu() {
    static_assert(sizeof(om_update_info) == 16, "om_update_info");
    const Material m = Material::new_lambertian(Color(.5f, .5f, .5f));
    HittableList w = HittableList::new_(), want = HittableList::new_();
    w.add_triangles(kV, 4, kF, 2, m);
    want.add_triangles(kV2, 4, kF, 2, m);
    w.update_triangles(kV2, 4, kF, 2);
    EXPECT(same_triangle(w, want, 0) && same_triangle(w, want, 1));
    bool threw = false;
    const uint32_t bad[6] = {0u, 1u, 2u, 0u, 2u, 4u};
    try { w.update_triangles(kV, 4, bad, 2); } catch (const Error& e) { threw = e.status == OM_ERR_INVALID; }
    EXPECT(threw && same_triangle(w, want, 0) && same_triangle(w, want, 1));      // all or nothing
    threw = false;
    try { w.update_triangles(kV, 4, kF, 2, 1); } catch (const Error& e) { threw = e.status == OM_ERR_INVALID; }
    EXPECT(threw);                                                                  // past the last triangle
    EXPECT(om_world_update_triangles(nullptr, 0, kV, 4, kF, 2) == OM_ERR_INVALID);
    EXPECT(om_update_triangles(nullptr, 0, kV, 4, kF, 2) == OM_ERR_INVALID);
    EXPECT(om_update_triangles_device(nullptr, 0, kV, 4, kF, 2, nullptr) == OM_ERR_INVALID);
    om_update_info u;
    EXPECT(om_get_update_info(nullptr, &u) == OM_ERR_INVALID);
    if (!g_fail) std::printf("cpu ok\n");
    return g_fail;
}

static int run_gpu(const char* mesh_in, const char* rays_in, const char* hits_out) {
    std::ifstream mf(mesh_in, std::ios::binary);
    uint32_t nv = 0, nt = 0;
    mf.read((char*)&nv, 4); mf.read((char*)&nt, 4);
    std::vector<float> v((size_t)nv * 3u), v2((size_t)nv * 3u);
    std::vector<uint32_t> f((size_t)nt * 3u);
    mf.read((char*)v.data(), v.size() * 4u); mf.read((char*)v2.data(), v2.size() * 4u); mf.read((char*)f.data(), f.size() * 4u);
    std::ifstream rf(rays_in, std::ios::binary | std::ios::ate);
    if (!mf || !rf) { std::fprintf(stderr, "cannot read the inputs\n"); return 1; }
    const size_t n = (size_t)rf.tellg() / sizeof(om_ray);
    rf.seekg(0);
    std::vector<om_ray> rays(n);
    rf.read((char*)rays.data(), n * sizeof(om_ray));

    HittableList w = HittableList::new_();
    w += Sphere::new_with_radius(Point3(0.f, -1000.f, 0.f), 1000.f, Material::new_lambertian(Color(.5f, .5f, .5f)));
    w.add_triangles(v.data(), nv, f.data(), nt, Material::new_lambertian(Color(.2f, .4f, .9f)));
    const Camera cam = Camera::new_(Point3(3.2f, 2.f, 4.f), Point3(0.f, 1.f, 0.f), Vec3(0.f, 1.f, 0.f), 35.f, 1.5f, 0.f, 5.f);
    FrozenHittableList fz = w.freeze(cam);
    EXPECT(fz.update_info().updates == 0u);
    fz.update_triangles(v2.data(), nv, f.data(), nt);
    const om_update_info u = fz.update_info();
    EXPECT(u.updates == 1u && u.triangles == nt && u.unbounded == 0u && u.skipped == 0u);
    bool threw = false;
    std::vector<uint32_t> bad = f;
    bad[1] = nv;
    try { fz.update_triangles(v.data(), nv, bad.data(), nt); } catch (const Error& e) { threw = e.status == OM_ERR_INVALID; }
    EXPECT(threw && fz.update_info().updates == 1u);                                // refused: nothing written
    const std::vector<om_hit> hits = fz.hit_rays(rays, 0.001f, 100.0f);
    std::ofstream of(hits_out, std::ios::binary);
    of.write((const char*)hits.data(), hits.size() * sizeof(om_hit));
    if (!g_fail) std::printf("gpu ok %zu rays\n", n);
    return g_fail;
}

int main(int argc, char** argv) {
    try {
        if (argc == 2 && std::string(argv[1]) == "cpu") return run_cpu() ? 1 : 0;
        if (argc == 5 && std::string(argv[1]) == "gpu") return run_gpu(argv[2], argv[3], argv[4]) ? 1 : 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    std::fprintf(stderr, "usage: test_refit cpu | gpu MESH_IN RAYS_IN HITS_OUT\n");
    return 2;
}
