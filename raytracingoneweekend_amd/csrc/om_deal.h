// om_deal.h — how bounce 0 deals a batch's camera samples to the workgroups.
// The batch's samples i in [0, paths) are numbered in blocks of 64 (block u = [64u, 64u + 64): in
// full tiles one 8x8 tile of one sample).  D consecutive blocks form a group (D = OM_WF_DEAL_BLOCKS),
// and the groups go round-robin to the nseg workgroups: workgroup g takes the blocks u with
// (u / D) % nseg == g, in rising order.  Every sample is then produced exactly once, and the
// workgroups' shares differ by at most one group.  One arithmetic for the kernels (k_bounce's FIRST
// branch, k_raygen), the host's queue sizing and the CPU test (tests/cpp/deal_bijection.cpp); 64-bit
// wherever `paths` (up to 2^27) enters.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OM_DEAL_HD __host__ __device__
#else
#define OM_DEAL_HD
#endif

struct Deal {
    uint64_t paths;   // camera samples of the batch
    uint64_t blocks;  // 64-sample blocks, the last one partial where paths % 64 != 0
    uint32_t nseg;    // workgroups (= queue segments)
    uint32_t d;       // consecutive blocks per group

    // groups of d blocks, the last one short where blocks % d != 0
    OM_DEAL_HD uint64_t groups() const { return (blocks + d - 1u) / d; }
    // blocks of workgroup g
    OM_DEAL_HD uint32_t blocks_of(uint32_t g) const {
        const uint64_t ng = groups();
        if (g >= ng) return 0u;
        const uint64_t mine = (ng - 1u - g) / nseg + 1u;           // groups g, g + nseg, ...
        uint64_t b = mine * d;
        if ((ng - 1u) % nseg == g) b -= ng * d - blocks;           // the short last group is g's
        return (uint32_t)b;
    }
    // the c-th block of workgroup g (c < blocks_of(g)), rising in c
    OM_DEAL_HD uint64_t block(uint32_t g, uint32_t c) const {
        return ((uint64_t)(c / d) * nseg + g) * d + c % d;
    }
    // camera samples of workgroup g
    OM_DEAL_HD uint32_t paths_of(uint32_t g) const {
        uint64_t n = (uint64_t)blocks_of(g) * 64u;
        if (blocks && ((blocks - 1u) / d) % nseg == g) n -= blocks * 64u - paths;   // the partial last block is g's
        return (uint32_t)n;
    }
    // the largest paths_of over the workgroups, to whole groups: the segment capacity the out queue
    // needs.  A multiple of 64; for d == 1 it is ceil(paths / nseg) rounded up to 64.
    OM_DEAL_HD uint32_t capacity() const {
        return (uint32_t)((groups() + nseg - 1u) / nseg * d * 64u);
    }
};

// Queue segments (= bounce workgroups) of a call whose largest batch has max_paths paths: one per
// `blk` paths, at most lanes_per_cu / blk per CU, a multiple of the marched tail's grouping `spb`.
inline uint32_t deal_segments(uint64_t max_paths, uint32_t cus, uint32_t lanes_per_cu, uint32_t blk, uint32_t spb) {
    const uint64_t want = (max_paths + blk - 1u) / blk, cap = (uint64_t)cus * (lanes_per_cu / blk);
    const uint32_t nseg = (uint32_t)(want < cap ? want : cap);
    return (nseg + spb - 1u) / spb * spb;
}

OM_DEAL_HD inline Deal make_deal(uint64_t paths, uint32_t nseg, uint32_t d) {
    return Deal{paths, (paths + 63u) / 64u, nseg, d};
}
