// om_tuning.h — the wavefront pipeline's tunable sizes.  These
// are numbers, not code variants: every value renders the same bits (results are keyed by slot
// and (pixel, sample)), and tools/ablate.sh sweeps them by -D.  The measurements behind each
// default are in DESIGN.md; the code variants that measured slower are gone (git history and
// DESIGN.md §8 keep their numbers).
#pragma once

// Workgroup = one queue segment.  512 lanes share one LDS copy of the BVH2 nodes between 8
// waves, so LDS stops capping occupancy, and 8 waves/SIMD (<= 64 VGPRs) hide the incoherent
// bounces' latency.  C1 (r01): 256/no hint 3770, 256/8 3671, 512/- 3802, 512/8 3929, 1024/8 3368.
#ifndef OM_WF_BLOCK
#define OM_WF_BLOCK 512
#endif
#ifndef OM_WF_WAVES
#define OM_WF_WAVES 8
#endif
// marched tail: queue segments per tail workgroup
#ifndef OM_WF_TAIL_SPB
#define OM_WF_TAIL_SPB 2
#endif
// traced tail: workgroups per CU of its resident grid (the queue's paths are dealt over them in
// 64-path units); at most OM_WF_WAVES * 256 / OM_WF_BLOCK stay resident.
// A tail workgroup holds its tree copy and the count prefix in LDS (C1: 41 KB) for as long as its
// last wave runs, beside the other batch's bounce workgroups: the smallest grid measured best.
// C1 at the old threshold 16: 4 / 3 / 2 / 1 -> 6972 / 7151 / 7313 / 7302 Msamples/s (parent 7224);
// with the threshold of each: 2 (T 10) / 1 (T 8) -> C1 7331 / 7307, C3 4532 / 4615, C4 7742 / 7698,
// C1 adaptive 18.55 / 18.3 ms per frame (profiles/balanced_tail/sweep.txt)
#ifndef OM_WF_TAIL_WGS_PER_CU
#define OM_WF_TAIL_WGS_PER_CU 1
#endif
// paths per batch: 2^OM_WF_MIN_PATHS_LOG2 (16 spp of 1080p), raised to OM_WF_BATCH_SPP samples of
// the frame for frames above 2M pixels, within 2^OM_WF_MAX_PATHS_LOG2
#ifndef OM_WF_MAX_PATHS_LOG2
#define OM_WF_MAX_PATHS_LOG2 27
#endif
#ifndef OM_WF_BATCH_SPP
#define OM_WF_BATCH_SPP 16
#endif
#ifndef OM_WF_MIN_PATHS_LOG2
#define OM_WF_MIN_PATHS_LOG2 25
#endif
// radiance queries (om_ray_color*): default paths per batch, 2^25 as ottomarcher.h documents it
// (om_set_path_batch).  The render's batch floor above has the same value today; the two are tuned apart.
#ifndef OM_WF_QUERY_PATHS_LOG2
#define OM_WF_QUERY_PATHS_LOG2 25
#endif
// A BVH2 too big for LDS (S-10k: 107 KB of half nodes) stages its breadth-first prefix, up to this
// many bytes of nodes, into LDS; deeper nodes are read through L2 (0 = every node from L2).  C3 with
// half nodes (r04_ab5/ab6): 8 / 12 / 16 / 20 / 24 / 28 KB -> 4113 / 4137 / 4135 / 4067 / 4069 / 3676.
#ifndef OM_WF_HYB_BYTES
#define OM_WF_HYB_BYTES 16384
#endif
// The same for the wide BVH2 (32-bit child codes behind a u32 lane stack), whose
// stack alone takes 2 KiB per level: 0, every node through L2.  Measured (MI355X, one session, tools/
// mesh_bench.py --heightfield 512: C1's world + 524 288 triangles, depth 20 = 40 KiB of stack), 0 / 8 / 16
// KiB -> render 50.4 / 53.8 / 70.5-72.9 ms, shuffled closest hit 1.169 / 1.505 / 1.724 ms, secondary
// closest hit 1.017 / 1.005 / 1.420 ms (profiles/mesh/large_mesh_bench.json).
#ifndef OM_WF_HYBW_BYTES
#define OM_WF_HYBW_BYTES 0
#endif
// The same for the half-precision 4-wide tree (OM_KERNEL_BVH4 on a tree too big for LDS, §5.7).
// C3 (r05_b4h): 0 / 4 / 8 / 12 KB -> 4028 / 3943 / 3895-3918 / 3918 Msamples/s: lanes whose node
// is in LDS and lanes whose node is not run both loads, so every node comes through L1/L2.
#ifndef OM_WF_HYB4_BYTES
#define OM_WF_HYB4_BYTES 0
#endif
// k_march refills its idle lanes once at least this many of a wave's 64 wait
#ifndef OM_WF_REFILL
#define OM_WF_REFILL 16
#endif
// marched tail: a wave shades its ended marches once this many of its lanes wait (1 = at once).
// r04's sweep ran with a ballot that made every value behave as 1; with the ballots
// fixed (r05_p1, C2, two runs each): 1 / 8 / 16 -> 3422, 3389 / 3407, 3384 / 3377, 3360: no gain, 1.
#ifndef OM_WF_TAIL_SHADE
#define OM_WF_TAIL_SHADE 1
#endif
// marched tail: march steps per check, and the refill threshold (k_march's by default)
// C2 (r04_tmu, r04_tmu2, two runs each): 4 / 8 / 12 / 16 / 24 / 32 -> 3105 / 3275, 3279 / 3316, 3305 /
// 3333, 3349, 3361, 3366 / 3399, 3426 / 3399, 3387; refill 8 / 16 / 32 -> 3205, 3200 / 3275, 3279 / 3226, 3247
#ifndef OM_WF_TAIL_UNROLL
#define OM_WF_TAIL_UNROLL 24
#endif
// marched tail: waves per SIMD requested (8: 64 VGPRs, the 24-step loop spills 32 B per lane)
#ifndef OM_WF_TAIL_MARCH_WAVES
#define OM_WF_TAIL_MARCH_WAVES 8
#endif
#ifndef OM_WF_TAIL_REFILL
#define OM_WF_TAIL_REFILL OM_WF_REFILL
#endif
// marched worlds: first bounce run by the lane-refilling tail (0: the camera paths too; DESIGN.md
// §5.8).  C2 T = 12 / 6 / 4 / 3 / 2 / 1 -> 2906 / 3064 / 3081 / 3077 / 3209 / 3274 Msamples/s (r04_sw1-
// sw3, means of two runs); on the tuned tail T = 0 / 1 -> 2843, 2916 / 3425, 3413 (r04_q3)
#ifndef OM_WF_TAIL_MARCHED
#define OM_WF_TAIL_MARCHED 1
#endif
// k_march: march steps per refill check (the check costs three ballots and its branches).
// C2 (r03_v16/v17): 1 / 2 / 4 / 6 / 8 steps -> 2500 / 2587 / 2650 / 2661 / 2682 Msamples/s.
#ifndef OM_MARCH_UNROLL
#define OM_MARCH_UNROLL 8
#endif
// Adaptive calls: the live pixels are dealt to the streams by 64-entry chunks of the
// call's pixel list, and each stream renders ITS pixels in at most OM_WF_ADAPTIVE_BATCHES batches per
// call, from a live list its own k_accumulate compacts (ThreadPixels, render_thread.rs:68-102).  A
// batch's sample count is planned on the device from the stream's live count c: enough samples to
// give 2^OM_WF_ADAPTIVE_PATHS_LOG2 paths (c x b), at least an even share of the call's remaining
// samples over the batches left, at most the remainder.
#ifndef OM_WF_ADAPTIVE_BATCHES
#define OM_WF_ADAPTIVE_BATCHES 3
#endif
#ifndef OM_WF_ADAPTIVE_PATHS_LOG2
#define OM_WF_ADAPTIVE_PATHS_LOG2 22
#endif
// the queue capacity an adaptive call may raise its forced even share to (more batches beyond it)
#ifndef OM_WF_ADAPTIVE_CAP_LOG2
#define OM_WF_ADAPTIVE_CAP_LOG2 26
#endif
// tail threshold for adaptive batches (the per-bounce launches of a light batch are latency-bound);
// on the balanced tail 6 / 8 / 10 / 12 -> 18.35 / 18.3 / 18.45 / 18.75 ms per C1 adaptive frame
#ifndef OM_WF_ADAPTIVE_TAIL
#define OM_WF_ADAPTIVE_TAIL 8
#endif
// Queue segments (= bounce workgroups) per CU: OM_WF_LANES_PER_CU / OM_WF_BLOCK; marched worlds
// and BVH2s read through L2 use the WIDE count.  2048 is one resident round of
// workgroups: with bounce 0's even deal (OM_WF_DEAL_BLOCKS) the segments are alike, and the second
// round per slot that evened out the stripes' unequal segments (4096, through r07) no longer pays.
#ifndef OM_WF_LANES_PER_CU
#define OM_WF_LANES_PER_CU 2048
#endif
#ifndef OM_WF_LANES_PER_CU_WIDE
#define OM_WF_LANES_PER_CU_WIDE 8192
#endif
// Bounce 0's deal (om_deal.h): consecutive 64-sample blocks a workgroup takes
// before the round-robin moves on to the next workgroup.  1 spreads every stripe of the frame over
// all segments, but a later bounce's wave then holds the survivors of tiles from all over the frame;
// larger values keep neighbouring tiles' paths together in the segment (and their candidate lists
// in one CU's scalar cache).  C1, plain bench, alternating on one box, parent (contiguous ranges)
// 7226, 7293: 1 / 2 / 4 / 8 -> 7030, 6980 / 7097, 7092 / 7256, 7192 / 7335, 7345; a second box,
// parent 7375, 7344: 8 / 16 / 32 / 64 -> 7508, 7479 / 7370, 7401 / 7565, 7541 / 7502, 7516, and
// with OM_WF_LANES_PER_CU 2048: 1 / 8 / 32 -> 7440, 7415 / 7766, 7752 / 7470, 7447
// (profiles/even_deal; one stream: parent 5252, 1 -> 5811, 8 -> 5988 Msamples/s).
#ifndef OM_WF_DEAL_BLOCKS
#define OM_WF_DEAL_BLOCKS 8
#endif
// Traced worlds: 1, the launch of bounce 0 also traces and shades bounce 1 on the lanes whose path
// goes on, and compacts them into bounce 2's queue (k_bounce's FUSE): the
// 64 B per path that bounce 0 would write and bounce 1 read back (C1: 26.0 M paths, 3.3 GB per 16-spp
// batch) stay in registers.  Bounce 0's waves are 8x8 tiles and the paths that end there end in sky,
// so 20.6 % of C1's blocks have no survivor and skip the second segment, and the others trace it
// at 98.6 % lane occupancy (tests/cpp/fused_census.cpp, profiles/fused_b01/census.jsonl).  The
// default tail thresholds count per-bounce launches, so the tail starts one bounce later and the
// launches per batch are the same.  0: bounce 1 is a launch of its own over queue 1.
#ifndef OM_WF_FUSE_B1
#define OM_WF_FUSE_B1 1
#endif
// k_accumulate: samples whose loads are issued together before their adds in sample order
#ifndef OM_ACC_GROUP
#define OM_ACC_GROUP 8
#endif
// BVH2 f32 nodes staged whole in LDS: bytes between consecutive nodes (64 = packed).  A wave's
// node reads are ds_read_b128/b96 at random nodes; at a 64-B stride word k of every node falls
// in one of 4 (b128) / 2 (b96) bank slots, at 80 B in one of 16 / 8 (r06, VERDICT r05 #1b).
// C1 (r06_ab1, r06_ab2): 80 -> 7128, 7118 / 6902, 6911 vs 64 -> 7077, 7107 / 6863, 6874 Msamples/s.
#ifndef OM_B2_NODE_STRIDE
#define OM_B2_NODE_STRIDE 80
#endif
// BVH2 f32 nodes staged whole in LDS: 1, the LDS copy keeps every (child, axis) plane pair as
// [lo, hi, lo] (om_b2_planes.h) and a lane reads (near, far) at the dword its ray's sign picks:
// 4 min/max per box instead of 10, three more node addresses per visit.  Needs
// the 80-B slot (a smaller OM_B2_NODE_STRIDE builds 0).  0: the node is copied as it is in memory
// and the visit orders the planes.  The first launch keeps the plain node either way (TR_PLAIN_NODES,
// om_wavefront.hip).  Measurements: DESIGN.md §8, profiles/ordered_planes/final_ab.txt.
#ifndef OM_B2_PLANES
#define OM_B2_PLANES 1
#endif
// Triangles + parallelograms (counted together; only the bounded ones with finite records) from
// which select (om_bvh.cpp) puts them into the SBVH / BVH2 / BVH4 leaves beside the spheres and cubes
// (DESIGN.md §5.17); a world with fewer keeps them in always2 and its frozen layout byte for byte.
// NOT a measured crossover: 16 is above every world the repository renders, tests or benchmarks
// with barycentric primitives in always2 (random_scene, tie_scene and kitchen_sink hold 2 each), so
// that tests/test_tree_regimes.py, the launch counts pinned in tests/test_gpu_production_shapes.py
// and bench.py's four configs run exactly what they ran before.  The crossover itself is open.
#ifndef OM_BARY_TREE_MIN
#define OM_BARY_TREE_MIN 16
#endif
// Ray queries: the reach of the slab test (far_origin in om_wavefront.hip).  With the
// origin d (largest axis distance, 0 inside) from the box of the bounded primitives, of diagonal R,
// the origin is at most sqrt(3) d from the box and a root inside it at most t = sqrt(3) d + R away;
// the slab test (reciprocal to 1 ulp, one fma per plane) places a plane to within 2u (|o - box| + t),
// u = 2^-24, beyond what the 1e-5 |coord| term of the inflation carries.  That stays below the
// inflation's floor of 1e-3 while 2 sqrt(3) d + R <= 1e-3 / 2u = 8389; a ray with more takes the
// reference loop -- every ray of a world whose bounded primitives span more than that.
#ifndef OM_SLAB_REACH
#define OM_SLAB_REACH 8192.0f
#endif
// The distance of a ray origin from a sphere or ellipsoid up to which its box must cover the worst
// case of Sphere::hit's rounding (thin_sphere in om_bvh.cpp): the reference scene's own camera distance,
// 13.4, rounded up to a power of two.  A sphere whose margin cannot do that stays outside the trees.
// Beyond it the culls hold for the typical, not the worst, rounding.
#ifndef OM_SPHERE_REACH
#define OM_SPHERE_REACH 16.0
#endif
