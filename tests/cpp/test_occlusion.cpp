// test_occlusion.cpp — the C++ mirror's any-hit queries and per-ray windows (include/ottomarcher.hpp:
// FrozenHittableList::occluded / occluded_rays / hit_rays with windows), driven by
// tests/test_cpp_occlusion.py.
//
//   test_occlusion cpu            record sizes and the null-argument errors (no device calls)
//   test_occlusion gpu RAYS_IN WINDOWS_IN OCC_OUT HITS_OUT
//                                 S-traced frozen through the API; reads n om_ray and n om_ray_window
//                                 records, writes the n bytes of occluded_rays and the n om_hit records
//                                 of hit_rays, both with the per-ray windows (the Python side compares
//                                 them with the CPU oracle); occluded() on the first rays must equal
//                                 the batch without windows
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

static int run_cpu() {
    static_assert(sizeof(om_ray_window) == 8, "window record");
    const om_query_params q{0.001f, 100.0f, 1024u, 0u};
    om_ray r{{0.f, 0.f, 0.f}, {0.f, 0.f, -1.f}};
    om_ray_window win{0.001f, 1.0f};
    om_hit h;
    uint8_t occ = 0xAA;
    EXPECT(om_occluded_rays(nullptr, &q, &r, &win, 1, &occ) == OM_ERR_INVALID);
    EXPECT(om_occluded_rays_device(nullptr, &q, &r, nullptr, 1, &occ, nullptr) == OM_ERR_INVALID);
    EXPECT(om_hit_rays_windows(nullptr, &q, &r, &win, 1, &h) == OM_ERR_INVALID);
    EXPECT(om_hit_rays_windows_device(nullptr, &q, &r, &win, 1, &h, nullptr) == OM_ERR_INVALID);
    EXPECT(occ == 0xAA);
    if (!g_fail) std::printf("cpu ok\n");
    return g_fail;
}

template <class T>
static bool read_records(const char* path, std::vector<T>& out) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", path); return false; }
    out.resize((size_t)f.tellg() / sizeof(T));
    f.seekg(0);
    f.read((char*)out.data(), (std::streamsize)(out.size() * sizeof(T)));
    return true;
}

static int run_gpu(const char* rays_in, const char* windows_in, const char* occ_out, const char* hits_out) {
    std::vector<om_ray> rays;
    std::vector<om_ray_window> windows;
    if (!read_records(rays_in, rays) || !read_records(windows_in, windows)) return 1;
    EXPECT(rays.size() == windows.size());
    HittableList w = HittableList::new_();
    check(om_world_random_scene(w.handle(), 0x5EED, 0, 11));
    const Camera cam = Camera::new_(Point3(13.f, 2.f, 3.f), Point3(0.f, 0.f, 0.f), Vec3(0.f, 1.f, 0.f), 20.f, 1.5f, 0.1f, 10.f);
    FrozenHittableList frozen = w.freeze(cam);
    const std::vector<uint8_t> occ = frozen.occluded_rays(rays, 0.001f, 100.0f, windows);
    const std::vector<om_hit> hits = frozen.hit_rays(rays, 0.001f, 100.0f, windows);
    EXPECT(occ.size() == rays.size() && hits.size() == rays.size());
    EXPECT(frozen.occluded_rays({}, 0.001f, 100.0f).empty());       // n == 0: OM_OK, nothing launched
    const std::vector<uint8_t> call = frozen.occluded_rays(rays, 0.001f, 100.0f);
    const std::vector<om_hit> closest = frozen.hit_rays(rays, 0.001f, 100.0f);
    size_t n_occ = 0;
    for (size_t i = 0; i < rays.size(); ++i) {
        EXPECT(call[i] == (closest[i].obj != 0u ? 1u : 0u));        // any-hit == closest-hit's is_some
        EXPECT(occ[i] == (hits[i].obj != 0u ? 1u : 0u));
        if (i < 16) {                                               // the one-ray form == the batch's byte
            const bool one = frozen.occluded(Vec3(rays[i].orig[0], rays[i].orig[1], rays[i].orig[2]),
                                             Vec3(rays[i].dir[0], rays[i].dir[1], rays[i].dir[2]), 0.001f, 100.0f);
            EXPECT(one == (call[i] != 0u));
            n_occ += one ? 1u : 0u;
        }
    }
    bool threw = false;                                             // one window per ray
    try { (void)frozen.occluded_rays(rays, 0.001f, 100.0f, std::vector<om_ray_window>(1)); }
    catch (const Error& e) { threw = e.status == OM_ERR_INVALID; }
    EXPECT(threw || rays.size() == 1);
    std::ofstream o(occ_out, std::ios::binary);
    o.write((const char*)occ.data(), (std::streamsize)occ.size());
    std::ofstream oh(hits_out, std::ios::binary);
    oh.write((const char*)hits.data(), (std::streamsize)(hits.size() * sizeof(om_hit)));
    if (!g_fail) std::printf("gpu ok (%zu rays, %zu of the first 16 occluded)\n", rays.size(), n_occ);
    return g_fail;
}

int main(int argc, char** argv) {
    try {
        if (argc >= 2 && std::string(argv[1]) == "cpu") return run_cpu() ? 1 : 0;
        if (argc >= 6 && std::string(argv[1]) == "gpu") return run_gpu(argv[2], argv[3], argv[4], argv[5]) ? 1 : 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 2;
    }
    std::fprintf(stderr, "usage: test_occlusion cpu | gpu RAYS_IN WINDOWS_IN OCC_OUT HITS_OUT\n");
    return 64;
}
