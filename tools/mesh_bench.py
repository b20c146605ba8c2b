"""Ray-query and render rates on a triangle mesh: C1's world (S-traced
random_scene(0x5EED)) plus an icosphere of level 5 (20 480 triangles, radius 1, centre (0, 1, 0)),
1920x1080.

  pinhole    the frame's centre rays in pixel (row-major) order
  shuffled   the same rays in a random order
  secondary  one bounce: from every pinhole hit point, one random unit direction

Each set through om_hit_rays_device (closest hit) and om_occluded_rays_device (any hit), in Grays/s;
and one render figure: the same world at 16 spp, depth 50, fixed spp, in Msamples/s.

Each query figure is the time of one call, from HIP events around `--reps` calls on a dedicated
stream after `--warmup` calls, taken `--groups` times; the file keeps every group.  Counting is off.

The yardstick is the PARENT commit's build on the same rays in the same session, never a mode of the
build under test: `--root PARENT_TREE` measures that tree's package (it builds the same world with
one om_world_add_triangle call per face) and prints one JSON line; run it before and after, and
give the lines' file to --parent-json.  The parent tests one box per triangle and ray, so give it
fewer `--reps`.

    python tools/mesh_bench.py --root PARENT_TREE --reps 3 --groups 5 >> parent.jsonl
    python tools/mesh_bench.py --parent-json parent.jsonl        -> profiles/mesh/mesh_bench.json

`--heightfield N` replaces the icosphere by an N x N-cell heightfield (512: 524 288 triangles, a tree past
the BVH2's 15-bit child codes) and writes profiles/mesh/large_mesh_bench.json; the parent
runs OM_KERNEL_BVH's traversal there.  `--kernel K` and `OM_LIB=variant.so --lib-tag T` print one line each
for `--context-json` (this build's other kernels and build variants, same session):

    python tools/mesh_bench.py --heightfield 512 --root PARENT_TREE --reps 3 --groups 5 >> parent.jsonl
    python tools/mesh_bench.py --heightfield 512 --kernel bvh --reps 3 --groups 5 >> context.jsonl
    python tools/mesh_bench.py --heightfield 512 --reps 20 --parent-json parent.jsonl --context-json context.jsonl

The crossover that OM_BARY_TREE_MIN stands in for is not measured by this tool.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from query_bench import pinhole_rays, summary, timed  # noqa: E402

W, H = 1920, 1080
LEVEL, SPP, DEPTH = 5, 16, 50


def icosphere(level, center, radius):
    """scenes.icosphere, restated here so that a tree without it (the parent) gets the same mesh"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    verts = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
             (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    verts = [np.asarray(v, dtype=np.float64) / np.linalg.norm(v) for v in verts]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
             (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
             (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, split = {}, []
        for a, b, c in faces:
            m = []
            for p, q in ((a, b), (b, c), (c, a)):
                key = (min(p, q), max(p, q))
                if key not in mid:
                    s = verts[p] + verts[q]
                    verts.append(s / np.linalg.norm(s))
                    mid[key] = len(verts) - 1
                m.append(mid[key])
            split += [(a, m[0], m[2]), (b, m[1], m[0]), (c, m[2], m[1]), (m[0], m[1], m[2])]
        faces = split
    v = np.asarray(verts, dtype=np.float64) * radius + np.asarray(center, dtype=np.float64)
    return np.ascontiguousarray(v, dtype=np.float32), np.asarray(faces, dtype=np.uint32)


def heightfield(n):
    """scenes.heightfield(n, n, y = 0.3 sin(2.1 x) cos(1.7 z) + 1) over [-3, 3]^2, restated like the
    icosphere: 2 n^2 triangles, float32"""
    x = (-3.0 + 6.0 * np.arange(n + 1, dtype=np.float64) / n).astype(np.float32)
    gx, gz = np.meshgrid(x, x, indexing="ij")
    f32 = np.float32
    gy = (f32(0.3) * np.sin(f32(2.1) * gx, dtype=f32) * np.cos(f32(1.7) * gz, dtype=f32) + f32(1.0)).astype(f32)
    v = np.stack([gx, gy, gz], axis=-1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a = (i * (n + 1) + j).ravel()
    b, c, d = a + 1, a + (n + 1), a + (n + 2)
    f = np.stack([np.stack([a, b, c], axis=1), np.stack([c, b, d], axis=1)], axis=1).reshape(-1, 3)
    return np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.uint32)


def mesh_world(om, hf=0):
    w = om.random_scene(0x5EED)
    v, f = heightfield(hf) if hf else icosphere(LEVEL, (0., 1., 0.), 1.0)
    mat = om.Material.new_metal_fuzz((0.8, 0.7, 0.5), 0.05)
    t0 = time.perf_counter()
    if hasattr(w, "add_triangles"):
        w.add_triangles(v, f, mat)
        how = "add_triangles"
    else:
        for a, b, c in f:
            w += om.Triangle.new3points(v[a], v[b], v[c], mat)
        how = "om_world_add_triangle per face"
    return w, len(f), how, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--root", default=ROOT, help="tree whose raytracingoneweekend_amd is measured")
    ap.add_argument("--parent-json", help="the lines of the parent commit's build (--root PARENT), same session")
    ap.add_argument("--no-render", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--heightfield", type=int, default=0, metavar="N",
                    help="instead of the icosphere: an N x N-cell heightfield of 2 N^2 triangles (512: 524 288, a tree "
                         "past the 15-bit child codes, DESIGN.md §5.18) -> profiles/mesh/large_mesh_bench.json")
    ap.add_argument("--kernel", default="auto", help="kernel choice of the build under test; other than auto: one JSON "
                                                     "line for --context-json, no file")
    ap.add_argument("--context-json", help="lines of this build under other kernels (--kernel bvh / sbvh), same session")
    ap.add_argument("--lib-tag", default=None, help="a label for an OM_LIB build variant (one JSON line, no file)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "mesh", "large_mesh_bench.json" if args.heightfield else "mesh_bench.json")
    if not torch.cuda.is_available():
        sys.exit("mesh_bench: no HIP device; rates are only measured on the GPU")
    sys.path.insert(0, os.path.abspath(args.root))
    import raytracingoneweekend_amd as om
    from raytracingoneweekend_amd import _lib as L

    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    sp = stream.cuda_stream
    cam = om.default_camera(W / H)
    world, n_tri, how, t_add = mesh_world(om, args.heightfield)
    t0 = time.perf_counter()
    fz = world.freeze(cam, kernel=args.kernel)
    t_freeze = time.perf_counter() - t0
    L.check(L.lib.om_set_counting(fz.ctx, 0), fz.ctx)
    what = (f"{args.heightfield} x {args.heightfield}-cell heightfield over [-3, 3]^2, y = 0.3 sin(2.1 x) cos(1.7 z) + 1"
            if args.heightfield else f"icosphere level {LEVEL} at (0, 1, 0), radius 1")
    out = {"build_id": L.build_id(), "device": torch.cuda.get_device_name(0), "kernel": args.kernel,
           "tree_info": fz.tree_info() if hasattr(fz, "tree_info") else None, "lib_tag": args.lib_tag,
           "world": f"C1 (S-traced random_scene(0x5EED)) + {what}",
           "triangles": n_tri, "mesh_added_by": how, "add_s": round(t_add, 4), "freeze_upload_s": round(t_freeze, 4),
           "frame": f"{W}x{H}", "warmup": args.warmup, "reps": args.reps, "groups": args.groups, "counting": False, "sets": {}}
    g = torch.Generator(device="cuda").manual_seed(7)
    rays = pinhole_rays(cam, "cuda")
    shuffled = rays[torch.randperm(W * H, device="cuda", generator=g)].contiguous()
    hits = fz.hit_rays(rays, stream=sp)
    stream.synchronize()
    on = hits[:, 7].view(torch.int32) != 0
    d = torch.randn((int(on.sum()), 3), device="cuda", generator=g)
    secondary = torch.cat([hits[on][:, 1:4], d / d.norm(dim=1, keepdim=True)], dim=1).contiguous()
    hbuf = torch.empty((W * H, 8), dtype=torch.float32, device="cuda")
    obuf = torch.empty((W * H,), dtype=torch.uint8, device="cuda")
    stream.synchronize()
    for name, r in (("pinhole", rays), ("shuffled", shuffled), ("secondary", secondary)):
        n = r.shape[0]
        h, o = hbuf[:n], obuf[:n]
        row = {"rays": n}
        row["closest_hit"] = summary(timed(stream, lambda: fz.hit_rays(r, out=h, stream=sp), args.warmup, args.reps, args.groups), n)
        row["any_hit"] = summary(timed(stream, lambda: fz.occluded(r, out=o, stream=sp), args.warmup, args.reps, args.groups), n)
        for k in ("closest_hit", "any_hit"):
            row[k]["grays_per_s"] = round(row[k]["mrays_per_s"] / 1e3, 4)
        ids = h[:, 7].view(torch.int32)
        row["hit_share"] = round(float((ids != 0).float().mean()), 4)
        row["occluded_share"] = round(float(o.float().mean()), 4)
        out["sets"][name] = row
    if not args.no_render:
        stats = torch.zeros(W * H * 40, dtype=torch.uint8, device="cuda")
        p = om.make_params(DEPTH, 0.001, 100.0, SPP, W, H, seed=1, adaptive=False)
        ms = []
        for k in range(3):                                  # the first call warms up (buffers, tile lists)
            stats.zero_()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            L.check(L.lib.om_render_device(fz.ctx, C.byref(cam.raw), C.byref(p), C.c_void_p(stats.data_ptr()), C.c_void_p(sp)), fz.ctx)
            b.record(stream)
            b.synchronize()
            if k:
                ms.append(a.elapsed_time(b))
        out["render"] = {"spp": SPP, "max_depth": DEPTH, "ms": [round(x, 3) for x in ms],
                         "msamples_per_s": round(W * H * SPP / statistics.median(ms) / 1e3, 1)}
    fz.close()
    if args.parent_json:
        with open(args.parent_json) as f:
            runs = [json.loads(ln) for ln in f.read().splitlines() if ln.startswith("{")]
        out["parent_build"] = {"build_id": runs[0]["build_id"], "runs": len(runs), "mesh_added_by": runs[0]["mesh_added_by"],
                               "reps": runs[0]["reps"], "groups": runs[0]["groups"]}
        for name, row in out["sets"].items():
            for k in ("closest_hit", "any_hit"):
                ms = [x for run in runs for x in run["sets"][name][k]["ms"]]
                med = statistics.median(ms)
                row[k]["parent"] = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                                    "grays_per_s": round(row["rays"] / med / 1e6, 5)}
                row[k]["speedup_over_parent"] = round(med / row[k]["ms_median"], 2 if args.heightfield else 1)
                # no slower than the parent, the margin being the parent's own min-max spread
                row[k]["within_or_better_than_parent_spread"] = bool(row[k]["ms_median"] <= max(ms))
        if "render" in out and all("render" in run for run in runs):
            ms = [x for run in runs for x in run["render"]["ms"]]
            out["render"]["parent"] = {"ms": [round(x, 3) for x in ms],
                                       "msamples_per_s": round(W * H * SPP / statistics.median(ms) / 1e3, 1)}
            out["render"]["speedup_over_parent"] = round(statistics.median(ms) / statistics.median(out["render"]["ms"]),
                                                         2 if args.heightfield else 1)
            out["render"]["faster_than_parent_beyond_its_spread"] = bool(max(out["render"]["ms"]) < min(ms))
    if args.context_json:
        with open(args.context_json) as f:
            ctx = [json.loads(ln) for ln in f.read().splitlines() if ln.startswith("{")]
        out["context"] = [{"kernel": r["kernel"], "lib_tag": r.get("lib_tag"), "tree_info": r.get("tree_info"),
                           "render_ms": r.get("render", {}).get("ms"),
                           "sets": {n: {k: {"ms_median": s[k]["ms_median"], "grays_per_s": s[k]["grays_per_s"]}
                                        for k in ("closest_hit", "any_hit")} for n, s in r["sets"].items()}} for r in ctx]
    print(json.dumps(out))
    if args.root == ROOT and args.kernel == "auto" and not args.lib_tag:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
