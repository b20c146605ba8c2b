// test_paths.cpp — the C++ mirror's radiance queries (include/ottomarcher.hpp:
// FrozenHittableList::ray_color), driven by tests/test_cpp_ray_color.py.
//
//   test_paths cpu                record layouts, om_path_rng_state's advance rule, and the errors of
//                                 om_ray_color* / om_set_path_batch that need no device
//   test_paths gpu PATHS_IN RECORDS_OUT
//                                 S-traced frozen through the API; reads n records of (om_ray, uint64
//                                 state), 32 B each, writes the n om_radiance records of ray_color (the
//                                 Python side compares them with the CPU oracle); the implicit streams
//                                 and the batch knob must agree with the explicit call
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
    static_assert(sizeof(om_path_params) == 32 && sizeof(om_radiance) == 20, "radiance query records");
    // a draw moves the Weyl counter in the low word by 0x9E3779B9 (mod 2^32) and leaves the key
    const uint64_t s0 = om_path_rng_state(7, 1234, 5, 0);
    for (uint32_t draws : {1u, 2u, 7u, 0xFFFFFFFFu}) {
        const uint64_t s = om_path_rng_state(7, 1234, 5, draws);
        EXPECT((s >> 32) == (s0 >> 32));
        EXPECT((uint32_t)s == (uint32_t)s0 + draws * 0x9E3779B9u);
    }
    EXPECT(om_path_rng_state(7, 1234, 5, 0) != om_path_rng_state(7, 1235, 5, 0));
    EXPECT(om_path_rng_state(7, 1234, 5, 0) != om_path_rng_state(8, 1234, 5, 0));
    const om_path_params p{0.001f, 100.0f, 1024u, 50u, 1u, 0u, 0u};
    om_ray r{{0.f, 0.f, 0.f}, {0.f, 0.f, -1.f}};
    om_radiance out;
    std::memset(&out, 0xAB, sizeof out);
    const om_radiance before = out;
    EXPECT(om_ray_color(nullptr, &p, &r, nullptr, 1, &out) == OM_ERR_INVALID);
    EXPECT(om_ray_color_device(nullptr, &p, &r, nullptr, 1, &out, nullptr) == OM_ERR_INVALID);
    EXPECT(om_set_path_batch(nullptr, 0) == OM_ERR_INVALID);
    EXPECT(std::memcmp(&out, &before, sizeof out) == 0);            // a failed call writes nothing
    if (!g_fail) std::printf("cpu ok\n");
    return g_fail;
}

struct PathIn { om_ray ray; uint64_t state; };
static_assert(sizeof(PathIn) == 32, "input record");

static int run_gpu(const char* paths_in, const char* records_out) {
    std::ifstream f(paths_in, std::ios::binary | std::ios::ate);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", paths_in); return 1; }
    std::vector<PathIn> in((size_t)f.tellg() / sizeof(PathIn));
    f.seekg(0);
    f.read((char*)in.data(), (std::streamsize)(in.size() * sizeof(PathIn)));
    std::vector<om_ray> rays(in.size());
    std::vector<uint64_t> states(in.size());
    for (size_t i = 0; i < in.size(); ++i) { rays[i] = in[i].ray; states[i] = in[i].state; }
    HittableList w = HittableList::new_();
    check(om_world_random_scene(w.handle(), 0x5EED, 0, 11));
    const Camera cam = Camera::new_(Point3(13.f, 2.f, 3.f), Point3(0.f, 0.f, 0.f), Vec3(0.f, 1.f, 0.f), 20.f, 1.5f, 0.1f, 10.f);
    FrozenHittableList frozen = w.freeze(cam);
    const om_path_params p{0.001f, 100.0f, 1024u, 50u, 7u, 11u, 2u};
    const std::vector<om_radiance> rec = frozen.ray_color(rays, p, states);
    EXPECT(rec.size() == rays.size());
    EXPECT(frozen.ray_color({}, p).empty());                        // n == 0: OM_OK, nothing launched
    // many small batches == one batch
    frozen.set_path_batch(6);
    const std::vector<om_radiance> small = frozen.ray_color(rays, p, states);
    frozen.set_path_batch(0);
    EXPECT(small.size() == rec.size() && std::memcmp(small.data(), rec.data(), rec.size() * sizeof(om_radiance)) == 0);
    // the implicit streams == their states given explicitly
    std::vector<uint64_t> implicit(rays.size());
    for (size_t i = 0; i < rays.size(); ++i) implicit[i] = om_path_rng_state(p.seed, p.stream_base + (uint32_t)i, p.sample, 0);
    const std::vector<om_radiance> a = frozen.ray_color(rays, p), b = frozen.ray_color(rays, p, implicit);
    EXPECT(a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(om_radiance)) == 0);
    bool threw = false;                                             // one state per ray
    try { (void)frozen.ray_color(rays, p, std::vector<uint64_t>(1)); } catch (const Error& e) { threw = e.status == OM_ERR_INVALID; }
    EXPECT(threw || rays.size() == 1);
    threw = false;                                                  // the knob's range
    try { frozen.set_path_batch(5); } catch (const Error& e) { threw = e.status == OM_ERR_INVALID; }
    EXPECT(threw);
    std::ofstream o(records_out, std::ios::binary);
    o.write((const char*)rec.data(), (std::streamsize)(rec.size() * sizeof(om_radiance)));
    if (!g_fail) std::printf("gpu ok (%zu paths)\n", rays.size());
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
    std::fprintf(stderr, "usage: test_paths cpu | gpu PATHS_IN RECORDS_OUT\n");
    return 64;
}
