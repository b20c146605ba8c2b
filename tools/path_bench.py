"""Radiance-query rate (om_ray_color_device) against the render of the same paths, in
one process, build and world: C1's world (S-traced) at 1920x1080.

  query    the frame's pixel-centre rays x 16 samples in ONE call: the rays repeated 16 times
           (33.2M paths, one 2^25-path batch less 0.4M), implicit streams (seed, stream_base + i, 0)
  render   om_render_device of 16 samples per pixel of the same frame, fixed spp (33.2M samples),
           with the ctx's default schedule (two batches in flight)

Both are timed with HIP events around `--reps` calls on a dedicated stream after `--warmup` calls,
`--groups` times; the file keeps every group.  Work counting is off (the production kernels).  The
two runs trace different rays (pixel centres against jittered thin-lens rays) and different streams:
the figure compares rates, not records.

    python tools/path_bench.py            (GPU box)  -> profiles/path_query/path_bench.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/path_bench.py --query-only --warmup 1 --reps 1 --groups 1
                                          where the query's time goes, launch by launch (no file written)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP = 1920, 1080, 16


def pinhole_rays(cam, device):
    """(W*H, 6) float32 centre rays, row-major, no lens offset, normalised once in f32."""
    r = cam.raw
    t = lambda v: torch.tensor(list(v), dtype=torch.float32, device=device)
    org, hor, ver, llc = t(r.origin), t(r.horizontal), t(r.vertical), t(r.lower_left_corner)
    j, i = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=device),
                          torch.arange(W, dtype=torch.float32, device=device), indexing="ij")
    u = (i.reshape(-1) + 0.5) / W
    v = 1.0 - (j.reshape(-1) + 0.5) / H
    d = llc[None, :] + u[:, None] * hor[None, :] + v[:, None] * ver[None, :] - org[None, :]
    d = d / d.norm(dim=1, keepdim=True)
    return torch.cat([org.expand_as(d), d], dim=1).contiguous()


def timed(stream, call, warmup, reps, groups):
    """ms per call: `groups` figures, each from events around `reps` calls."""
    for _ in range(warmup):
        call()
    out = []
    for _ in range(groups):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(reps):
            call()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return out


def summary(ms, n):
    med = statistics.median(ms)
    return {"paths": n, "ms": [round(x, 3) for x in ms], "ms_median": round(med, 3), "ms_min": round(min(ms), 3),
            "ms_max": round(max(ms), 3), "mpaths_per_s": round(n / med / 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--groups", type=int, default=3)
    ap.add_argument("--query-only", action="store_true", help="time the query alone and write no file (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_query", "path_bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import raytracingoneweekend_amd as om
    from raytracingoneweekend_amd import _lib as L

    world = om.random_scene(0x5EED)
    cam = om.default_camera(W / H)
    fz = world.freeze(cam)
    L.check(L.lib.om_set_counting(fz.ctx, 0), fz.ctx)
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    n = W * H * SPP
    with torch.cuda.stream(stream):
        rays = pinhole_rays(cam, "cuda").repeat(SPP, 1).contiguous()
        out = torch.empty((n, 5), dtype=torch.float32, device="cuda")
        stats = torch.zeros(W * H * 40, dtype=torch.uint8, device="cuda")
    stream.synchronize()
    query = lambda: fz.ray_color(rays, seed=1, out=out, stream=stream.cuda_stream)
    q_ms = timed(stream, query, args.warmup, args.reps, args.groups)
    if args.query_only:
        print(json.dumps({"query": summary(q_ms, n)}))
        return
    spp_total = SPP * (args.warmup + args.reps * args.groups)
    p = om.make_params(50, 0.001, 100.0, spp_total, W, H, sample_count=SPP, seed=1, adaptive=False)
    render = lambda: L.check(L.lib.om_render_device(fz.ctx, C.byref(cam.raw), C.byref(p), C.c_void_p(stats.data_ptr()), sp), fz.ctx)
    r_ms = timed(stream, render, args.warmup, args.reps, args.groups)
    q, r = summary(q_ms, n), summary(r_ms, n)
    hit = int((out[:, 4].view(torch.int32) != 0).sum())
    res = {"device": torch.cuda.get_device_name(0), "build_id": L.build_id(), "world": "C1 (random_scene 0x5EED)", "frame": [W, H],
           "samples": SPP, "depth": 50, "first_hit_share": round(hit / n, 4), "query": q, "render": r,
           "ratio_query_over_render": round(q["mpaths_per_s"] / r["mpaths_per_s"], 4)}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
