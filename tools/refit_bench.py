"""Moving a mesh by om_update_triangles_device against the parent commit's only way, a re-upload
(DESIGN.md §5.21): C1's world (S-traced random_scene(0x5EED)) plus an N x N-cell heightfield over
[-3, 3]^2 at y = 1 + 0.3 sin(2.1 x + phase) cos(1.7 z), N = 128 (32 768 triangles) and 512 (524 288),
the phase advancing by 0.2 per wave step; 1920x1080.

  update_ms        device time of one om_update_triangles_device (all triangles): HIP events around
                   `--reps` calls on a dedicated stream after `--warmup` calls, `--groups` figures.  The calls
                   are back to back on one stream, so the figure is one whole update, its launches (one per
                   tree level) included; an update waits on the host only for the root-box copy of the
                   update before the previous one (two pinned nodes)
  upload_ms        host wall time of om_upload_world of the same moved world (it synchronises): the
                   freeze, the frees, the copies; `--uploads` figures
  freeze_ms        host wall time of om_world_tree_info of the same world (a freeze alone, the method
                   of profiles/bvh_stages/freeze_time.txt): comparable across commits
  after K steps    K = 1, 8, 32 successive wave steps of refit, then closest hits of the frame's
                   centre rays (Grays/s) and depth-50 render calls of 4 samples a pixel, fixed spp, every
                   call taking its samples (Msamples/s), each against a
                   fresh upload at the same vertices; the hit records of both must be identical

    python tools/refit_bench.py            -> profiles/refit/refit_bench.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from query_bench import pinhole_rays, timed  # noqa: E402

W, H, SPP, DEPTH = 1920, 1080, 4, 50
F = np.float32


def field(om, n, phase):
    fn = lambda x, z: (F(0.3) * np.sin(F(2.1) * x.astype(F) + F(phase), dtype=F) * np.cos(F(1.7) * z.astype(F), dtype=F) + F(1.0)).astype(F)
    return om.heightfield(n, n, fn, extent=((-3., 3.), (-3., 3.)))


def world(om, v, f):
    w = om.random_scene(0x5EED)
    w.add_triangles(v, f, om.Material.new_lambertian((0.3, 0.7, 0.3)))
    return w


def med(xs):
    return {"all": [round(x, 4) for x in xs], "median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def rates(om, L, fz, cam, rays, stream, a):
    sp = C.c_void_p(stream.cuda_stream)
    q = L.om_query_params(0.001, 100.0, 1024, 0)
    hits = torch.empty((rays.shape[0], 8), dtype=torch.float32, device=rays.device)
    hit = lambda: L.check(L.lib.om_hit_rays_device(fz.ctx, C.byref(q), C.c_void_p(rays.data_ptr()), rays.shape[0],
                                                   C.c_void_p(hits.data_ptr()), sp), fz.ctx)
    ms_h = timed(stream, hit, a.warmup, a.reps, a.groups)
    stats = torch.zeros(W * H * 40, dtype=torch.uint8, device=rays.device)
    # fixed spp, SPP samples per call: spp_total covers every call of the window, so that no call finds its pixels full
    calls = 1 + 2 * a.groups
    p = om.make_params(DEPTH, 0.001, 100.0, SPP * calls, W, H, sample_count=SPP, seed=7, adaptive=False)
    ren = lambda: L.check(L.lib.om_render_device(fz.ctx, C.byref(cam.raw), C.byref(p), C.c_void_p(stats.data_ptr()), sp), fz.ctx)
    ms_r = timed(stream, ren, 1, 2, a.groups)
    taken = int(stats.view(-1, 40)[:, 20:24].contiguous().view(torch.int32).min().item())
    assert taken == SPP * calls, f"a timed render call took no samples: Stats.n = {taken}, expected {SPP * calls}"
    stream.synchronize()
    return {"hit_ms": med(ms_h), "grays_per_s": round(rays.shape[0] / statistics.median(ms_h) / 1e6, 3),
            "render_ms": med(ms_r), "msamples_per_s": round(W * H * SPP / statistics.median(ms_r) / 1e3, 1)}, hits.clone()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,512")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--uploads", type=int, default=3)
    ap.add_argument("--steps", default="1,8,32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refit", "refit_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("refit_bench: no HIP device: nothing is measured without one")
    import raytracingoneweekend_amd as om
    from raytracingoneweekend_amd import _lib as L
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    cam = om.default_camera(W / H)
    res = {"frame": [W, H], "spp": SPP, "depth": DEPTH, "reps": a.reps, "groups": a.groups, "sizes": {}}
    with torch.cuda.stream(stream):
        rays = pinhole_rays(cam, dev)
        for n in [int(x) for x in a.sizes.split(",")]:
            v, f = field(om, n, 0.0)
            tf = torch.from_numpy(f.astype(np.int32)).to(dev)
            fz = world(om, v, f).freeze(cam)
            L.check(L.lib.om_set_counting(fz.ctx, 0), fz.ctx)
            row = {"triangles": int(len(f)), "tree": fz.tree_info()}
            v1, _ = field(om, n, 0.2)
            tv = [torch.from_numpy(v).to(dev), torch.from_numpy(v1).to(dev)]
            k = [0]

            def upd():
                k[0] ^= 1
                fz.update_triangles(tv[k[0]], tf, stream=stream.cuda_stream)
            row["update_ms"] = med(timed(stream, upd, a.warmup, a.reps, a.groups))
            w1 = world(om, v1, f)
            ups, frz = [], []
            ti = L.om_tree_info()
            for _ in range(a.uploads):
                stream.synchronize()
                t0 = time.perf_counter()
                L.check(L.lib.om_upload_world(fz.ctx, w1.handle), fz.ctx)
                ups.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                L.check(L.lib.om_world_tree_info(w1.handle, C.byref(ti)))
                frz.append((time.perf_counter() - t0) * 1e3)
            row["upload_ms"], row["freeze_ms"] = med(ups), med(frz)
            row["upload_over_update"] = round(row["upload_ms"]["median"] / row["update_ms"]["median"], 1)
            fz.close()
            # rates after K wave steps of refit against a fresh upload at the same vertices
            fz = world(om, v, f).freeze(cam)
            L.check(L.lib.om_set_counting(fz.ctx, 0), fz.ctx)
            row["steps"] = {}
            done = 0
            for K in [int(x) for x in a.steps.split(",")]:
                while done < K:
                    done += 1
                    vk, _ = field(om, n, 0.2 * done)
                    fz.update_triangles(torch.from_numpy(vk).to(dev), tf, stream=stream.cuda_stream)
                fresh = world(om, vk, f).freeze(cam)
                L.check(L.lib.om_set_counting(fresh.ctx, 0), fresh.ctx)
                r_refit, h_refit = rates(om, L, fz, cam, rays, stream, a)
                r_fresh, h_fresh = rates(om, L, fresh, cam, rays, stream, a)
                fresh.close()
                same = bool(torch.equal(h_refit.view(torch.int32), h_fresh.view(torch.int32)))
                row["steps"][str(K)] = {"refit": r_refit, "fresh": r_fresh, "hits_identical": same,
                                        "grays_ratio": round(r_refit["grays_per_s"] / r_fresh["grays_per_s"], 3),
                                        "msamples_ratio": round(r_refit["msamples_per_s"] / r_fresh["msamples_per_s"], 3)}
            fz.close()
            res["sizes"][str(n)] = row
            print(json.dumps({str(n): row}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
