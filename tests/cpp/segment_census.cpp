// segment_census.cpp — how evenly a batch's paths sit in the queue segments after bounce 0
// (DESIGN.md §5.5, §8), counted on the host with the oracle's ray_color.
//
// A path stays in the segment (= workgroup) bounce 0 put it in until the tail, so the segment counts
// at bounce b follow whichever camera samples the segment was given.  This program takes one fixed-spp
// call over the S-traced frame (bench.py's scene, camera and render seed; the tile-ordered pixel list;
// the batches and the segment count of the library's own formulas on a 256-CU device), takes every
// path's segment count from the oracle and sums, per bounce, the paths still alive per segment of
// every batch under two orders:
//   contiguous  segment s holds the samples [s * segcap, (s + 1) * segcap)   (the order before the deal)
//   dealt       om_deal.h: 64-sample blocks round-robin over the segments, D blocks at a time
// and prints per bounce: paths, non-empty segments, max / mean and the coefficient of variation of the
// counts, and makespan / ideal of an in-order list schedule of the nseg workgroups on `slots`
// resident slots with a workgroup's time taken as proportional to its paths (a model: neither that
// nor the device's dispatch order is measured here).
//   segment_census [W H spp [every [D [streams]]]]     every: count every n-th listed pixel (1 = all)
// (1920 1080 16 7 1 1: one 16-spp batch of the benchmark's frame, 15 s on 4 threads)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <queue>
#include <thread>
#include <vector>

#include "../../oracle/om_oracle.cpp"
#include "../../raytracingoneweekend_amd/csrc/om_deal.h"
#include "../../raytracingoneweekend_amd/csrc/om_shard.h"
#include "../../raytracingoneweekend_amd/csrc/om_tuning.h"

namespace omi {
om_status global_error(om_status code, const std::string&) { return code; }
}

namespace {

constexpr uint32_t kBounces = 8, kCus = 256;

struct Row { uint64_t paths; uint32_t nonempty; double max_mean, cv, makespan; };

Row reduce(const std::vector<uint64_t>& cnt, uint32_t slots) {
    Row r{0, 0, 0.0, 0.0, 0.0};
    uint64_t mx = 0;
    for (uint64_t c : cnt) { r.paths += c; r.nonempty += c != 0; mx = std::max(mx, c); }
    if (r.paths == 0) return r;
    const double mean = (double)r.paths / cnt.size();
    double var = 0.0;
    for (uint64_t c : cnt) var += ((double)c - mean) * ((double)c - mean);
    r.max_mean = mx / mean;
    r.cv = std::sqrt(var / cnt.size()) / mean;
    // in-order list scheduling: the next workgroup starts on the slot that frees first
    std::priority_queue<uint64_t, std::vector<uint64_t>, std::greater<uint64_t>> free_at;
    for (uint32_t s = 0; s < slots; ++s) free_at.push(0);
    uint64_t end = 0;
    for (uint64_t c : cnt) {
        const uint64_t t = free_at.top() + c;
        free_at.pop(); free_at.push(t);
        end = std::max(end, t);
    }
    r.makespan = (double)end / ((double)r.paths / slots);
    return r;
}

}  // namespace

int main(int argc, char** argv) {
    const uint32_t W = argc > 2 ? (uint32_t)std::atoi(argv[1]) : 480u, H = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 270u;
    const uint32_t spp = argc > 3 ? (uint32_t)std::atoi(argv[3]) : 2u;
    const uint32_t every = argc > 4 ? std::max(1, std::atoi(argv[4])) : 1u;
    const uint32_t D = argc > 5 ? std::max(1, std::atoi(argv[5])) : (uint32_t)OM_WF_DEAL_BLOCKS;
    const uint32_t streams = argc > 6 ? std::max(1, std::atoi(argv[6])) : 2u;
    oro::World world;
    oro_world_random_scene(&world, 0x5EED, 0u, 11);
    world.assign_ids();
    world.march_steps = 1024;
    const oro::Camera cam = oro::camera_new(oro::v3(13.f, 2.f, 3.f), oro::v3(0.f, 0.f, 0.f), oro::v3(0.f, 1.f, 0.f), 20.f,
                                            (float)W / (float)H, 0.1f, 10.f);
    const uint64_t seed = 1;
    const std::vector<float> jt = oro::jitter_table(seed, spp);
    const uint64_t skey = oro::seed_key(seed);
    std::vector<uint32_t> pixels;
    oms::deal(W, H, 0, 1, pixels);                               // the tile-ordered list of a whole frame
    const uint64_t n_px = pixels.size(), paths = n_px * spp;
    // the batches of a fixed-spp call (om_wavefront.hip render()): at most 2^OM_WF_MIN_PATHS_LOG2 paths
    // (OM_WF_BATCH_SPP samples of a larger frame, within 2^OM_WF_MAX_PATHS_LOG2), and at most
    // 1 / streams of the call, so that a call of two samples on two streams is two batches
    const uint64_t max_paths = std::min<uint64_t>(1ull << OM_WF_MAX_PATHS_LOG2,
                                                  std::max<uint64_t>(1ull << OM_WF_MIN_PATHS_LOG2, (uint64_t)OM_WF_BATCH_SPP * n_px));
    uint32_t batch = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(spp, max_paths / n_px));
    if (streams >= 2u && spp >= 2u) batch = std::min(batch, (spp + streams - 1u) / streams);
    const uint32_t nb = (spp + batch - 1u) / batch;
    const uint32_t nseg = deal_segments(n_px * batch, kCus, OM_WF_LANES_PER_CU, OM_WF_BLOCK, OM_WF_TAIL_SPB);
    const uint32_t slots = kCus * (uint32_t)(OM_WF_WAVES * 256 / OM_WF_BLOCK);
    const uint32_t segcap = make_deal(n_px * batch, nseg, 1u).capacity();

    // segments traced per path (ray_color), for every `every`-th listed pixel
    std::vector<uint8_t> segs(paths, 0);
    const unsigned nth = std::max(1u, std::min(4u, std::thread::hardware_concurrency()));
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nth; ++t)
        th.emplace_back([&, t] {
            for (uint64_t kk = (uint64_t)t * every; kk < n_px; kk += (uint64_t)nth * every) {
                const uint32_t pxl = pixels[kk], line = pxl / W, col = pxl - W * line;
                for (uint32_t s = 0; s < spp; ++s) {             // render_pixel's camera sample (a fresh frame: Stats.n == s)
                    oro::PathRng g = oro::path_rng(skey, pxl, s);
                    const float i_rand = (g.rand() + jt[2 * s]) / 2.0f, j_rand = (g.rand() + jt[2 * s + 1]) / 2.0f;
                    const float u = ((float)col + i_rand) / ((float)W - 1.0f), v = 1.0f - ((float)line + j_rand) / ((float)H - 1.0f);
                    const oro::Ray r = oro::camera_get_ray(cam, u, v, g);
                    const oro::SampleResult sr = oro::ray_color(world, r, 50, 0.001f, 100.0f, g);
                    segs[(uint64_t)s * n_px + kk] = (uint8_t)std::min<uint32_t>(sr.segments, 255u);
                }
            }
        });
    for (auto& t : th) t.join();

    std::printf("{\"frame\": [%u, %u], \"spp\": %u, \"every\": %u, \"paths\": %llu, \"batches\": %u, \"batch_spp\": %u, \"nseg\": %u, "
                "\"segcap\": %u, \"slots\": %u, \"D\": %u}\n", W, H, spp, every, (unsigned long long)paths, nb, batch, nseg, segcap, slots, D);
    for (uint32_t b = 1; b <= kBounces; ++b) {
        // the segments of every batch of the call, batch after batch (each batch has its own queues)
        std::vector<uint64_t> cont((size_t)nb * nseg, 0), dealt((size_t)nb * nseg, 0);
        for (uint32_t k = 0; k < nb; ++k) {
            const uint64_t first = (uint64_t)k * batch * n_px, n = std::min<uint64_t>((uint64_t)batch * n_px, paths - first);
            const uint32_t cap = make_deal(n, nseg, 1u).capacity();   // this batch's contiguous split
            for (uint64_t i = 0; i < n; ++i) {
                if (segs[first + i] <= b) continue;              // ended before bounce b (or not counted)
                cont[(size_t)k * nseg + i / cap]++;
                dealt[(size_t)k * nseg + ((i / 64u) / D) % nseg]++;
            }
        }
        const Row c = reduce(cont, slots), d = reduce(dealt, slots);
        std::printf("{\"bounce\": %u, \"paths\": %llu, \"contiguous\": {\"nonempty\": %u, \"max_mean\": %.3f, \"cv\": %.3f, \"makespan\": %.3f}, "
                    "\"dealt\": {\"nonempty\": %u, \"max_mean\": %.3f, \"cv\": %.3f, \"makespan\": %.3f}}\n",
                    b, (unsigned long long)c.paths, c.nonempty, c.max_mean, c.cv, c.makespan, d.nonempty, d.max_mean, d.cv, d.makespan);
    }
    return 0;
}
