// test_render_rays.cpp — the C++ mirror's frames from caller-given rays (include/ottomarcher.hpp:
// FrozenHittableList::render_rays), driven by tests/test_cpp_render_rays.py.
//
//   test_render_rays cpu          the errors of om_render_rays* that need no device
//   test_render_rays gpu W H SPP RAYS_IN STATS_OUT
//                                 S-traced frozen through the API; reads SPP * W * H records of (om_ray,
//                                 uint64 state), 32 B each, sample-major; renders the adaptive frame in
//                                 one call and writes its W * H om_pixel_stats (the Python side compares
//                                 them with the CPU oracle); the same frame must come out of one call
//                                 per sample, of small batches and of a pixel list that names the frame;
//                                 the wrapper's size checks throw
#include <cstdio>
#include <cstdlib>
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

static om_render_params params(uint32_t W, uint32_t H, uint32_t spp, uint32_t count) {
    om_render_params p{};
    p.width = W; p.height = H; p.spp_total = spp; p.sample_count = count;
    p.max_depth = 50; p.tmin = 0.001f; p.tmax = 100.0f; p.march_steps = 1024; p.adaptive = 1; p.seed = 7;
    return p;
}

static int run_cpu() {
    const om_render_params p = params(2, 2, 4, 1);
    std::vector<om_ray> rays(4, om_ray{{0.f, 0.f, 0.f}, {0.f, 0.f, -1.f}});
    std::vector<om_pixel_stats> stats(4);
    std::memset(stats.data(), 0xAB, stats.size() * sizeof(om_pixel_stats));
    const std::vector<om_pixel_stats> before = stats;
    om_counters c{};
    EXPECT(om_render_rays(nullptr, &p, rays.data(), nullptr, nullptr, 4, stats.data(), &c) == OM_ERR_INVALID);
    EXPECT(om_render_rays_device(nullptr, &p, rays.data(), nullptr, nullptr, 4, stats.data(), nullptr) == OM_ERR_INVALID);
    EXPECT(std::memcmp(stats.data(), before.data(), stats.size() * sizeof(om_pixel_stats)) == 0);   // nothing written
    EXPECT(c.samples == 0 && c.credited == 0);
    if (!g_fail) std::printf("cpu ok\n");
    return g_fail;
}

struct PathIn { om_ray ray; uint64_t state; };
static_assert(sizeof(PathIn) == 32, "input record");

static bool same(const std::vector<om_pixel_stats>& a, const std::vector<om_pixel_stats>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(om_pixel_stats)) == 0;
}

static int run_gpu(uint32_t W, uint32_t H, uint32_t spp, const char* rays_in, const char* stats_out) {
    const size_t n = (size_t)W * H;
    std::ifstream f(rays_in, std::ios::binary | std::ios::ate);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", rays_in); return 1; }
    std::vector<PathIn> in((size_t)f.tellg() / sizeof(PathIn));
    f.seekg(0);
    f.read((char*)in.data(), (std::streamsize)(in.size() * sizeof(PathIn)));
    if (in.size() != n * spp) { std::fprintf(stderr, "%s: %zu records, expected %zu\n", rays_in, in.size(), n * spp); return 1; }
    std::vector<om_ray> rays(in.size());
    std::vector<uint64_t> states(in.size());
    for (size_t i = 0; i < in.size(); ++i) { rays[i] = in[i].ray; states[i] = in[i].state; }
    HittableList w = HittableList::new_();
    check(om_world_random_scene(w.handle(), 0x5EED, 0, 11));
    const Camera cam = Camera::new_(Point3(13.f, 2.f, 3.f), Point3(0.f, 0.f, 0.f), Vec3(0.f, 1.f, 0.f), 20.f, 1.5f, 0.1f, 10.f);
    FrozenHittableList frozen = w.freeze(cam);

    std::vector<om_pixel_stats> frame(n);                           // zeroed Stats
    const om_counters c = frozen.render_rays(frame, rays, params(W, H, spp, spp), states);
    uint64_t taken = 0;
    for (const om_pixel_stats& px : frame) taken += px.n;
    EXPECT(c.samples == taken && c.credited == n * spp && c.segments >= c.samples);

    // one call per sample
    std::vector<om_pixel_stats> steps(n);
    om_counters sum{};
    for (uint32_t s = 0; s < spp; ++s) {
        const std::vector<om_ray> r(rays.begin() + s * n, rays.begin() + (s + 1) * n);
        const std::vector<uint64_t> g(states.begin() + s * n, states.begin() + (s + 1) * n);
        const om_counters cs = frozen.render_rays(steps, r, params(W, H, spp, 1), g);
        sum.samples += cs.samples; sum.credited += cs.credited;
    }
    EXPECT(same(steps, frame) && sum.samples == c.samples && sum.credited == c.credited);
    // a finished frame takes nothing more
    const om_counters again = frozen.render_rays(steps, rays, params(W, H, spp, spp), states);
    EXPECT(same(steps, frame) && again.samples == 0 && again.segments == 0);
    // many small batches == one batch
    frozen.set_path_batch(6);
    std::vector<om_pixel_stats> small(n);
    frozen.render_rays(small, rays, params(W, H, spp, spp), states);
    frozen.set_path_batch(0);
    EXPECT(same(small, frame));
    // the frame named by a list, backwards: entry k is pixel n-1-k, so every sample row is reversed
    std::vector<uint32_t> pixels(n);
    std::vector<om_ray> rrays(rays.size());
    std::vector<uint64_t> rstates(states.size());
    for (size_t k = 0; k < n; ++k) pixels[k] = (uint32_t)(n - 1 - k);
    for (uint32_t s = 0; s < spp; ++s)
        for (size_t k = 0; k < n; ++k) { rrays[s * n + k] = rays[s * n + n - 1 - k]; rstates[s * n + k] = states[s * n + n - 1 - k]; }
    std::vector<om_pixel_stats> listed(n);
    frozen.render_rays(listed, rrays, params(W, H, spp, spp), rstates, pixels);
    EXPECT(same(listed, frame));
    // the wrapper's size checks
    int threw = 0;
    try { (void)frozen.render_rays(frame, std::vector<om_ray>(n - 1), params(W, H, spp, 1)); } catch (const Error& e) { threw += e.status == OM_ERR_INVALID; }
    try { (void)frozen.render_rays(frame, rays, params(W, H, spp, spp), std::vector<uint64_t>(1)); } catch (const Error& e) { threw += e.status == OM_ERR_INVALID; }
    try { std::vector<om_pixel_stats> shorter(n - 1); (void)frozen.render_rays(shorter, rays, params(W, H, spp, spp)); } catch (const Error& e) { threw += e.status == OM_ERR_INVALID; }
    try { pixels[0] = (uint32_t)n; (void)frozen.render_rays(listed, rrays, params(W, H, spp, spp), rstates, pixels); } catch (const Error& e) { threw += e.status == OM_ERR_INVALID; }
    EXPECT(threw == 4);
    EXPECT(same(listed, frame));                                    // the refused calls wrote nothing

    std::ofstream o(stats_out, std::ios::binary);
    o.write((const char*)frame.data(), (std::streamsize)(frame.size() * sizeof(om_pixel_stats)));
    if (!g_fail) std::printf("gpu ok (%zu pixels, %u samples)\n", n, spp);
    return g_fail;
}

int main(int argc, char** argv) {
    try {
        if (argc >= 2 && std::string(argv[1]) == "cpu") return run_cpu() ? 1 : 0;
        if (argc >= 7 && std::string(argv[1]) == "gpu")
            return run_gpu((uint32_t)std::atoi(argv[2]), (uint32_t)std::atoi(argv[3]), (uint32_t)std::atoi(argv[4]), argv[5], argv[6]) ? 1 : 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 2;
    }
    std::fprintf(stderr, "usage: test_render_rays cpu | gpu W H SPP RAYS_IN STATS_OUT\n");
    return 64;
}
