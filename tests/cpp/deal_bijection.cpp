// Bounce 0's deal (raytracingoneweekend_amd/csrc/om_deal.h), exhaustively on the host
// (tests/test_deal.py): over every (paths, nseg, D) of the lists below, every sample index of the
// batch is produced exactly once over all (workgroup, block), each workgroup's share fits the segment
// capacity the host sizes the queues with, its blocks rise, and blocks_of / paths_of agree with the
// enumeration.  Prints one line per case; exit status 1 on the first violation.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../raytracingoneweekend_amd/csrc/om_deal.h"
#include "../../raytracingoneweekend_amd/csrc/om_tuning.h"

static int check(uint64_t paths, uint32_t nseg, uint32_t d) {
    const Deal dl = make_deal(paths, nseg, d);
    const uint32_t cap = dl.capacity();
    std::vector<uint8_t> seen(paths, 0);
    uint64_t total = 0;
    uint32_t most = 0;
    if (cap % 64u) { std::printf("capacity %u is no multiple of 64\n", cap); return 1; }
    for (uint32_t g = 0; g < nseg; ++g) {
        const uint32_t nb = dl.blocks_of(g);
        uint64_t mine = 0, prev = 0;
        for (uint32_t c = 0; c < nb; ++c) {
            const uint64_t u = dl.block(g, c);
            if (c && u <= prev) { std::printf("g %u: block %u (%llu) does not rise\n", g, c, (unsigned long long)u); return 1; }
            if ((u / d) % nseg != g) { std::printf("g %u: block %llu belongs elsewhere\n", g, (unsigned long long)u); return 1; }
            if (u >= dl.blocks) { std::printf("g %u: block %llu past the batch\n", g, (unsigned long long)u); return 1; }
            prev = u;
            for (uint32_t lane = 0; lane < 64u; ++lane) {
                const uint64_t i = u * 64u + lane;
                if (i >= paths) continue;                      // the kernels' bound on the partial last block
                if (seen[i]++) { std::printf("sample %llu produced twice\n", (unsigned long long)i); return 1; }
                ++mine;
            }
        }
        if (mine != dl.paths_of(g)) { std::printf("g %u: paths_of %u, enumerated %llu\n", g, dl.paths_of(g), (unsigned long long)mine); return 1; }
        if (mine > cap) { std::printf("g %u: %llu paths exceed the capacity %u\n", g, (unsigned long long)mine, cap); return 1; }
        if (mine > most) most = (uint32_t)mine;
        total += mine;
    }
    if (total != paths) { std::printf("%llu of %llu samples produced\n", (unsigned long long)total, (unsigned long long)paths); return 1; }
    // D == 1 keeps the capacity of the contiguous split: ceil(paths / nseg) to whole waves
    if (d == 1u && cap != ((paths + nseg - 1u) / nseg + 63u) / 64u * 64u) { std::printf("capacity %u differs from the even split's\n", cap); return 1; }
    std::printf("paths %llu nseg %u D %u: capacity %u, fullest %u ok\n", (unsigned long long)paths, nseg, d, cap, most);
    return 0;
}

int main() {
    const uint32_t nsegs[] = {1u, 2u, 48u}, ds[] = {1u, 2u, 4u, 8u, (uint32_t)OM_WF_DEAL_BLOCKS};
    for (uint32_t nseg : nsegs) {
        const uint64_t n = nseg;
        const uint64_t paths[] = {0u, 1u, 63u, 64u, 65u, 64u * n - 1u, 64u * n, 64u * n + 1u, 64u * (3u * n + 5u) + 17u};
        for (uint64_t p : paths)
            for (uint32_t d : ds)
                if (check(p, nseg, d)) { std::printf("FAILED at paths %llu nseg %u D %u\n", (unsigned long long)p, nseg, d); return 1; }
    }
    // the largest batch (2^27 paths, 2048 segments): the 64-bit arithmetic; totals only
    for (uint32_t d : ds) {
        const Deal dl = make_deal((1ull << 27) - 5u, 2048u, d);
        uint64_t total = 0;
        for (uint32_t g = 0; g < 2048u; ++g) {
            if (dl.paths_of(g) > dl.capacity()) { std::printf("2^27: g %u over capacity\n", g); return 1; }
            total += dl.paths_of(g);
        }
        if (total != dl.paths) { std::printf("2^27 D %u: total %llu\n", d, (unsigned long long)total); return 1; }
    }
    std::printf("all ok\n");
    return 0;
}
