// fused_census.cpp — how full a bounce-1 trace would be if it ran inside the bounce-0 launch, on the
// lanes bounce 0 left alive and before any compaction, counted on the
// host with the oracle's ray_color.
//
// Bounce 0 runs the batch's camera samples in 64-sample blocks (om_deal.h: block u = samples
// [64u, 64u + 64), in full tiles one 8x8 tile of one sample), one block per wave iteration.  A fused
// second segment traces on the same lanes: a block with no survivor skips it, every other block pays
// one wave trace whatever its survivors.  This program takes one fixed-spp batch over the S-traced
// frame (bench.py's scene, camera and render seed; the tile-ordered pixel list), takes every path's
// segment count from the oracle and reports, over the blocks it counts:
//   the share of blocks with no survivor, the mean and the distribution of survivors per non-empty
//   block, and the lane occupancy of the fused trace = survivors / (64 x non-empty blocks).
//   fused_census [W H spp [every]]     every: count every n-th block (1 = all)
// (1920 1080 16 7: one 16-spp batch of the benchmark's frame, a seventh of its tiles)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../../oracle/om_oracle.cpp"
#include "../../raytracingoneweekend_amd/csrc/om_deal.h"
#include "../../raytracingoneweekend_amd/csrc/om_shard.h"

namespace omi {
om_status global_error(om_status code, const std::string&) { return code; }
}

int main(int argc, char** argv) {
    const uint32_t W = argc > 2 ? (uint32_t)std::atoi(argv[1]) : 480u, H = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 270u;
    const uint32_t spp = argc > 3 ? (uint32_t)std::atoi(argv[3]) : 2u;
    const uint32_t every = argc > 4 ? std::max(1, std::atoi(argv[4])) : 1u;
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
    const uint64_t n_px = pixels.size();
    const Deal dl = make_deal(n_px * spp, 1u, 1u);               // the batch's blocks, as bounce 0 numbers them

    // survivors of bounce 0 (paths of two segments or more) per counted block
    std::vector<uint8_t> alive((size_t)dl.blocks, 0), lanes((size_t)dl.blocks, 0);
    const unsigned nth = std::max(1u, std::min(4u, std::thread::hardware_concurrency()));
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nth; ++t)
        th.emplace_back([&, t] {
            for (uint64_t u = (uint64_t)t * every; u < dl.blocks; u += (uint64_t)nth * every)
                for (uint64_t i = u * 64u; i < std::min<uint64_t>(u * 64u + 64u, dl.paths); ++i) {
                    const uint32_t s = (uint32_t)(i / n_px), pxl = pixels[i - (uint64_t)s * n_px];
                    const uint32_t line = pxl / W, col = pxl - W * line;
                    oro::PathRng g = oro::path_rng(skey, pxl, s);   // render_pixel's camera sample (a fresh frame: Stats.n == s)
                    const float i_rand = (g.rand() + jt[2 * s]) / 2.0f, j_rand = (g.rand() + jt[2 * s + 1]) / 2.0f;
                    const float uu = ((float)col + i_rand) / ((float)W - 1.0f), vv = 1.0f - ((float)line + j_rand) / ((float)H - 1.0f);
                    const oro::Ray r = oro::camera_get_ray(cam, uu, vv, g);
                    const oro::SampleResult sr = oro::ray_color(world, r, 50, 0.001f, 100.0f, g);
                    lanes[u]++;
                    alive[u] += sr.segments > 1u;
                }
        });
    for (auto& t : th) t.join();

    uint64_t counted = 0, empty = 0, full = 0, paths = 0, survivors = 0, hist[8] = {};
    for (uint64_t u = 0; u < dl.blocks; u += every) {
        counted++; paths += lanes[u]; survivors += alive[u];
        if (alive[u] == 0) { empty++; continue; }
        full += alive[u] == 64;
        hist[(alive[u] - 1u) / 8u]++;                            // 1-8, 9-16, ..., 57-64 survivors
    }
    const uint64_t nonempty = counted - empty;
    std::printf("{\"frame\": [%u, %u], \"spp\": %u, \"every\": %u, \"blocks\": %llu, \"counted_blocks\": %llu, \"paths\": %llu, "
                "\"survivors\": %llu, \"survivor_share\": %.4f}\n", W, H, spp, every, (unsigned long long)dl.blocks,
                (unsigned long long)counted, (unsigned long long)paths, (unsigned long long)survivors,
                paths ? (double)survivors / (double)paths : 0.0);
    std::printf("{\"empty_blocks\": %llu, \"empty_share\": %.4f, \"nonempty_blocks\": %llu, \"full_blocks\": %llu, "
                "\"mean_survivors\": %.3f, \"survivors_hist_by_8\": [%llu, %llu, %llu, %llu, %llu, %llu, %llu, %llu], "
                "\"fused_lane_occupancy\": %.4f}\n", (unsigned long long)empty, counted ? (double)empty / (double)counted : 0.0,
                (unsigned long long)nonempty, (unsigned long long)full, nonempty ? (double)survivors / (double)nonempty : 0.0,
                (unsigned long long)hist[0], (unsigned long long)hist[1], (unsigned long long)hist[2], (unsigned long long)hist[3],
                (unsigned long long)hist[4], (unsigned long long)hist[5], (unsigned long long)hist[6], (unsigned long long)hist[7],
                nonempty ? (double)survivors / (64.0 * (double)nonempty) : 0.0);
    return 0;
}
