"""Rate of a frame rendered from caller-given rays (om_render_rays_device) against the
render of the same frame, in one process, build and world: C1's world (S-traced) at 1920x1080, 16
samples per call, fixed spp.

  render   om_render_device of 16 samples per pixel, with the ctx's default schedule (two batches in flight)
  rays     om_render_rays_device of the same 16 samples from that frame's own thin-lens rays and RNG
           states (33.2M rays, 24 + 8 bytes each), made once on the device before timing: the om-rng
           v2 stream, the jitter table's rows and Camera::get_ray restated with torch in float32.
           The restatement follows the reference's operation order but is not held to its bits (torch
           may fuse or reorder); it gives the timed call rays of the render's distribution, and the
           tests, not this tool, compare frames.  Every call draws the same 16 samples (the Stats
           buffer is sized for all of them: spp_total is 16 x the number of calls).

Both are timed with HIP events around `--reps` calls on a dedicated stream after `--warmup` calls,
`--groups` times; the file keeps every group.  Work counting is off (the production kernels).

    python tools/frame_rays_bench.py     (GPU box)  -> profiles/frame_rays/bench.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/frame_rays_bench.py --rays-only --warmup 1 --reps 1 --groups 1
                                          where the call's time goes, launch by launch (no file written)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, SEED = 1920, 1080, 16, 1
M64 = (1 << 64) - 1


def _mix64_host(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _i64(v):
    """A uint64 constant as the int64 torch holds."""
    return v - (1 << 64) if v >= (1 << 63) else v


def _shr(z, k):
    """Logical right shift of int64 tensors holding uint64 bits."""
    return (z >> k) & ((1 << (64 - k)) - 1)


def _mix64(z):
    z = (z ^ _shr(z, 30)) * _i64(0xBF58476D1CE4E5B9)
    z = (z ^ _shr(z, 27)) * _i64(0x94D049BB133111EB)
    return z ^ _shr(z, 31)


def _draw(s, k):
    """One om-rng v2 draw: (s, k) int64 tensors holding the 32-bit words -> (float32 in [0, 1), s')."""
    m = 0xFFFFFFFF
    s = (s + 0x9E3779B9) & m
    x = s ^ k
    x = x ^ (x >> 16)
    x = (x * 0x21F0AAAD) & m
    x = x ^ (x >> 15)
    x = (x * 0x735A2D97) & m
    x = x ^ (x >> 15)
    return (x >> 8).to(torch.float32) * 5.9604644775390625e-8, s


def thin_lens_table(om, cam, device):
    """-> rays (SPP, W*H, 6) float32, states (SPP, W*H) int64: sample s of every pixel as om_render
    draws it for Stats.n == s of a SPP-sample frame (render_thread.rs:176-192, camera.rs:60-78)."""
    from oracle import oracle as O                                  # the jitter table only
    jt = torch.from_numpy(O.jitter_table(SEED, SPP)).to(device)
    r = cam.raw
    t = lambda v: torch.tensor(list(v), dtype=torch.float32, device=device)
    org, hor, ver, llc, cu, cv = t(r.origin), t(r.horizontal), t(r.vertical), t(r.lower_left_corner), t(r.u_of_plane), t(r.v_of_plane)
    skey = _i64(_mix64_host((SEED + 0x632BE59BD9B4E019) & M64))
    px = torch.arange(W * H, dtype=torch.int64, device=device)
    col, line = (px % W).to(torch.float32), (px // W).to(torch.float32)
    rays = torch.empty((SPP, W * H, 6), dtype=torch.float32, device=device)
    states = torch.empty((SPP, W * H), dtype=torch.int64, device=device)
    for s in range(SPP):
        z = _mix64(((px << 32) | s) ^ skey)
        k, w = _shr(z, 32), z & 0xFFFFFFFF
        d0, w = _draw(w, k)
        d1, w = _draw(w, k)
        u = (col + (d0 + jt[s, 0]) / 2.0) / (W - 1.0)
        v = 1.0 - (line + (d1 + jt[s, 1]) / 2.0) / (H - 1.0)
        x = torch.zeros_like(u)
        y = torch.zeros_like(u)
        todo = torch.ones_like(px, dtype=torch.bool)
        while bool(todo.any()):                                     # rand_in_unit_disc, vec3.rs:108-113
            a, w2 = _draw(w, k)
            b, w2 = _draw(w2, k)
            xa, yb = a * 2.0 - 1.0, b * 2.0 - 1.0
            x, y, w = torch.where(todo, xa, x), torch.where(todo, yb, y), torch.where(todo, w2, w)
            todo = todo & ~(xa * xa + yb * yb < 1.0)
        off = (r.lens_radius * x)[:, None] * cu + (r.lens_radius * y)[:, None] * cv
        o = org + off
        d = llc + u[:, None] * hor + v[:, None] * ver - org - off
        d = d / torch.linalg.vector_norm(d, dim=1, keepdim=True)
        rays[s, :, :3], rays[s, :, 3:] = o, d
        states[s] = (k << 32) | w
    return rays, states


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
    return {"samples": n, "ms": [round(x, 3) for x in ms], "ms_median": round(med, 3), "ms_min": round(min(ms), 3),
            "ms_max": round(max(ms), 3), "msamples_per_s": round(n / med / 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--groups", type=int, default=3)
    ap.add_argument("--rays-only", action="store_true", help="time om_render_rays_device alone and write no file (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_rays", "bench.json"))
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
    calls = args.warmup + args.reps * args.groups
    with torch.cuda.stream(stream):
        rays, states = thin_lens_table(om, cam, "cuda")
        stats_a = torch.zeros(W * H * 40, dtype=torch.uint8, device="cuda")
        stats_b = torch.zeros(W * H * 40, dtype=torch.uint8, device="cuda")
    stream.synchronize()
    p = om.make_params(50, 0.001, 100.0, SPP * calls, W, H, sample_count=SPP, seed=SEED, adaptive=False)
    from_rays = lambda: L.check(L.lib.om_render_rays_device(fz.ctx, C.byref(p), C.c_void_p(rays.data_ptr()), C.c_void_p(states.data_ptr()),
                                                            None, W * H, C.c_void_p(stats_b.data_ptr()), sp), fz.ctx)
    b_ms = timed(stream, from_rays, args.warmup, args.reps, args.groups)
    if args.rays_only:
        print(json.dumps({"rays": summary(b_ms, n)}))
        return
    render = lambda: L.check(L.lib.om_render_device(fz.ctx, C.byref(cam.raw), C.byref(p), C.c_void_p(stats_a.data_ptr()), sp), fz.ctx)
    a_ms = timed(stream, render, args.warmup, args.reps, args.groups)
    stream.synchronize()
    # the first call's 16 samples are the render's own if the restatement kept every bit; reported, not required
    na = np.frombuffer(stats_a.cpu().numpy().tobytes(), dtype=L.PIXEL_STATS_DTYPE)
    nb = np.frombuffer(stats_b.cpu().numpy().tobytes(), dtype=L.PIXEL_STATS_DTYPE)
    a, b = summary(a_ms, n), summary(b_ms, n)
    res = {"device": torch.cuda.get_device_name(0), "build_id": L.build_id(), "world": "C1 (random_scene 0x5EED)", "frame": [W, H],
           "samples_per_call": SPP, "depth": 50, "calls_each": calls, "n_per_pixel": [int(na["n"].min()), int(nb["n"].min())],
           "mean_colour_sum": [round(float(na["sum"].mean()), 4), round(float(nb["sum"].mean()), 4)],
           "render": a, "rays": b, "ratio_rays_over_render": round(b["msamples_per_s"] / a["msamples_per_s"], 4)}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
