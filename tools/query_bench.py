"""Ray-query rate (om_hit_rays_device) on the C1 world (S-traced, 1920x1080):

  pinhole    the frame's centre rays in pixel (row-major) order
  shuffled   the same rays in a random order
  secondary  one bounce: from every pinhole hit point, one random unit direction

  marched    the pinhole rays of C2's world (om.marched_scene, 256 march steps): the marched variant
             of the kernel, which spills

against the yardstick: bounce 0 of one sample per pixel of the same frame with primary lists off
(om_set_primary_lists(OFF), om_set_timing mode 1, OM_KT_BOUNCE0) -- the same number of coherent
rays through the same traversal, which also generates, shades and compacts them.

Each figure is the time of one call, from HIP events around `--reps` calls on a dedicated stream
after `--warmup` calls; it is taken `--groups` times and the file keeps every group, so the
spread is on record beside the medians.  Work counting is off (the production kernels).

    python tools/query_bench.py                  (GPU box)  -> profiles/query/query_bench.json
    python tools/query_bench.py --yardstick-only --root OTHER_TREE > parent.json    another build's yardstick
    python tools/query_bench.py --parent-json parent.json             ... recorded in the same file

--occlusion: the any-hit rate (om_occluded_rays_device) beside the closest-hit rate
(om_hit_rays_device, no windows) on the same rays: the four sets above with the call's window, and

  ao         from every pinhole hit point, one random unit direction in the normal's hemisphere with a
             per-ray window [0.001, 0.5] (closest-hit row: the same rays in [0.001, 100])

The yardstick of an any-hit row is the PARENT build's closest-hit time on the same rays, taken in
the same session: `--closest-only --root PARENT_TREE` prints one JSON line with the closest-hit rows
alone (it needs nothing the parent lacks); run it before and after, and give both lines' file to
--parent-json.  A set passes when the any-hit median is at most the parent's closest-hit median plus
the parent's own min-max spread over every group of every parent run.

    python tools/query_bench.py --closest-only --root PARENT_TREE >> parent.jsonl
    python tools/query_bench.py --occlusion --parent-json parent.jsonl   -> profiles/query/occlusion_bench.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080


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
    return {"rays": n, "ms": [round(x, 4) for x in ms], "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
            "ms_max": round(max(ms), 4), "mrays_per_s": round(n / med / 1e3, 1)}


def yardstick(om, L, fz, cam, stream, warmup, reps, groups):
    """Bounce 0 of one sample per pixel, primary lists off: OM_KT_BOUNCE0 ms per launch."""
    sp = C.c_void_p(stream.cuda_stream)
    L.check(L.lib.om_set_primary_lists(fz.ctx, 0), fz.ctx)
    stats = torch.zeros(W * H * 40, dtype=torch.uint8, device="cuda")
    spp = warmup + reps * groups
    p = om.make_params(50, 0.001, 100.0, spp, W, H, sample_count=1, seed=1)
    render = lambda: L.check(L.lib.om_render_device(fz.ctx, C.byref(cam.raw), C.byref(p), C.c_void_p(stats.data_ptr()), sp), fz.ctx)
    for _ in range(warmup):
        render()
    stream.synchronize()
    out = []
    for _ in range(groups):
        L.check(L.lib.om_set_timing(fz.ctx, 1), fz.ctx)
        for _ in range(reps):
            render()
        kt = L.om_kernel_times()
        L.check(L.lib.om_get_kernel_times(fz.ctx, C.byref(kt)), fz.ctx)
        k = L.KT_CLASSES.index("bounce0")
        assert kt.launches[k] == reps, kt.launches[k]
        out.append(kt.ms[k] / reps)
    L.check(L.lib.om_set_timing(fz.ctx, 0), fz.ctx)
    L.check(L.lib.om_set_primary_lists(fz.ctx, 1), fz.ctx)
    return out


def occlusion_sets(om, L, fz, cam, stream):
    """The ray sets of the --occlusion rows on the C1 world: {name: (rays, windows or None)}."""
    g = torch.Generator(device="cuda").manual_seed(7)
    rays = pinhole_rays(cam, "cuda")
    shuffled = rays[torch.randperm(W * H, device="cuda", generator=g)].contiguous()
    hits = fz.hit_rays(rays, stream=stream.cuda_stream)
    stream.synchronize()
    on = hits[:, 7].view(torch.int32) != 0
    k = int(on.sum())
    d = torch.randn((k, 3), device="cuda", generator=g)
    secondary = torch.cat([hits[on][:, 1:4], d / d.norm(dim=1, keepdim=True)], dim=1).contiguous()
    d = torch.randn((k, 3), device="cuda", generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    d = torch.where((d * hits[on][:, 4:7]).sum(dim=1, keepdim=True) < 0, -d, d)      # into the normal's hemisphere
    ao = torch.cat([hits[on][:, 1:4], d], dim=1).contiguous()
    ao_win = torch.tensor([0.001, 0.5], dtype=torch.float32, device="cuda").repeat(k, 1).contiguous()
    return {"pinhole": (rays, None), "shuffled": (shuffled, None), "secondary": (secondary, None), "ao": (ao, ao_win)}


def occlusion_bench(om, L, args, stream, cam):
    """--occlusion / --closest-only: closest-hit and (not --closest-only) any-hit rows per ray set."""
    sp = stream.cuda_stream
    fz = om.random_scene(0x5EED).freeze(cam)
    L.check(L.lib.om_set_counting(fz.ctx, 0), fz.ctx)
    out = {"build_id": L.build_id(), "device": torch.cuda.get_device_name(0), "world": "C1: S-traced random_scene(0x5EED)",
           "frame": f"{W}x{H}", "warmup": args.warmup, "reps": args.reps, "groups": args.groups, "counting": False,
           "closest_only": bool(args.closest_only), "sets": {}}
    sets = occlusion_sets(om, L, fz, cam, stream)
    mz = om.marched_scene().freeze(cam)
    L.check(L.lib.om_set_counting(mz.ctx, 0), mz.ctx)
    hbuf = torch.empty((W * H, 8), dtype=torch.float32, device="cuda")
    obuf = torch.empty((W * H,), dtype=torch.uint8, device="cuda")
    stream.synchronize()
    jobs = [(name, fz, r, win, {}, args.reps) for name, (r, win) in sets.items()]
    jobs.append(("marched_pinhole", mz, sets["pinhole"][0], None, {"march_steps": 256}, max(1, args.reps // 4)))
    for name, z, r, win, kw, reps in jobs:
        n = r.shape[0]
        h, o = hbuf[:n], obuf[:n]
        row = {"rays": n, "reps": reps, "window": "per ray [0.001, 0.5]" if win is not None else "call [0.001, 100]"}
        ms = timed(stream, lambda: z.hit_rays(r, out=h, stream=sp, **kw), args.warmup, reps, args.groups)
        row["closest_hit"] = summary(ms, n)
        row["hit_share"] = round(float((h[:, 7].view(torch.int32) != 0).float().mean()), 4)
        if not args.closest_only:
            ms = timed(stream, lambda: z.occluded(r, windows=win, out=o, stream=sp, **kw), args.warmup, reps, args.groups)
            row["any_hit"] = summary(ms, n)
            row["occluded_share"] = round(float(o.float().mean()), 4)
            ms = timed(stream, lambda: z.hit_rays(r, out=h, stream=sp, **kw), args.warmup, reps, args.groups)
            row["closest_hit_again"] = summary(ms, n)
        out["sets"][name] = row
    mz.close()
    fz.close()
    if args.parent_json and not args.closest_only:
        with open(args.parent_json) as f:
            runs = [json.loads(ln) for ln in f.read().splitlines() if ln.startswith("{")]
        out["parent_build"] = {"build_id": runs[0]["build_id"], "runs": len(runs)}
        for name, row in out["sets"].items():
            ms = [x for run in runs for x in run["sets"][name]["closest_hit"]["ms"]]
            med, spread = statistics.median(ms), max(ms) - min(ms)
            here = row["closest_hit"]["ms"] + row["closest_hit_again"]["ms"]
            row["parent_closest_hit"] = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
            row["any_hit_within_parent_spread"] = bool(row["any_hit"]["ms_median"] <= med + spread)
            row["closest_hit_vs_parent"] = {"ms_median": round(statistics.median(here), 4),
                                            "within_parent_spread": bool(abs(statistics.median(here) - med) <= spread)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--root", default=ROOT, help="tree whose raytracingoneweekend_amd is measured")
    ap.add_argument("--yardstick-only", action="store_true")
    ap.add_argument("--parent-json", help="the --yardstick-only line of the parent commit's build, same session")
    ap.add_argument("--occlusion", action="store_true", help="any-hit rows beside closest-hit ones (occlusion_bench.json)")
    ap.add_argument("--closest-only", action="store_true", help="the closest-hit rows of --occlusion alone, one JSON line")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "query", "occlusion_bench.json" if args.occlusion else "query_bench.json")
    if not torch.cuda.is_available():
        sys.exit("query_bench: no HIP device; rates are only measured on the GPU")
    sys.path.insert(0, os.path.abspath(args.root))
    import raytracingoneweekend_amd as om
    from raytracingoneweekend_amd import _lib as L

    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    cam = om.default_camera(W / H)
    if args.occlusion or args.closest_only:
        out = occlusion_bench(om, L, args, stream, cam)
        print(json.dumps(out))
        if not args.closest_only:
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")
        return
    fz = om.random_scene(0x5EED).freeze(cam)
    L.check(L.lib.om_set_counting(fz.ctx, 0), fz.ctx)
    out = {"build_id": L.build_id(), "device": torch.cuda.get_device_name(0), "world": "C1: S-traced random_scene(0x5EED)",
           "frame": f"{W}x{H}", "warmup": args.warmup, "reps": args.reps, "groups": args.groups, "counting": False}
    yd = yardstick(om, L, fz, cam, stream, args.warmup, args.reps, args.groups)
    out["yardstick_bounce0_lists_off"] = summary(yd, W * H)
    if not args.yardstick_only:
        out["query_max_grid"] = fz.query_max_grid()
        g = torch.Generator(device="cuda").manual_seed(7)
        rays = pinhole_rays(cam, "cuda")
        shuffled = rays[torch.randperm(W * H, device="cuda", generator=g)].contiguous()
        hits = fz.hit_rays(rays, stream=stream.cuda_stream)
        stream.synchronize()
        on = hits[:, 7].view(torch.int32) != 0
        d = torch.randn((int(on.sum()), 3), device="cuda", generator=g)
        secondary = torch.cat([hits[on][:, 1:4], d / d.norm(dim=1, keepdim=True)], dim=1).contiguous()
        sets = {"pinhole": rays, "shuffled": shuffled, "secondary": secondary}
        buf = torch.empty((W * H, 8), dtype=torch.float32, device="cuda")
        stream.synchronize()
        for name, r in sets.items():
            o = buf[:r.shape[0]]
            ms = timed(stream, lambda: fz.hit_rays(r, out=o, stream=stream.cuda_stream), args.warmup, args.reps, args.groups)
            out[name] = summary(ms, r.shape[0])
            out[name]["hit_share"] = round(float((o[:, 7].view(torch.int32) != 0).float().mean()), 4)
        # the yardstick once more after the queries: its spread over the session
        yd2 = yardstick(om, L, fz, cam, stream, args.warmup, args.reps, args.groups)
        out["yardstick_bounce0_lists_off_again"] = summary(yd2, W * H)
        every = yd + yd2
        out["pinhole_vs_yardstick"] = {
            "yardstick_ms_min": round(min(every), 4), "yardstick_ms_max": round(max(every), 4),
            "pinhole_ms_median": out["pinhole"]["ms_median"],
            "pinhole_not_slower_than_yardstick": bool(out["pinhole"]["ms_median"] <= max(every))}
        if args.parent_json:
            with open(args.parent_json) as f:
                par = json.loads([ln for ln in f.read().splitlines() if ln.startswith("{")][-1])
            out["yardstick_parent_build"] = {"build_id": par["build_id"], **par["yardstick_bounce0_lists_off"]}
        # C2's world: the marched kernel variant
        mz = om.marched_scene().freeze(cam)
        L.check(L.lib.om_set_counting(mz.ctx, 0), mz.ctx)
        o = buf[:rays.shape[0]]
        ms = timed(stream, lambda: mz.hit_rays(rays, march_steps=256, out=o, stream=stream.cuda_stream),
                   args.warmup, max(1, args.reps // 4), args.groups)
        out["marched_pinhole"] = summary(ms, rays.shape[0])
        out["marched_pinhole"].update(world="C2: marched_scene, 256 march steps", reps=max(1, args.reps // 4),
                                      hit_share=round(float((o[:, 7].view(torch.int32) != 0).float().mean()), 4))
        mz.close()
    fz.close()
    line = json.dumps(out)
    print(line)
    if not args.yardstick_only:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
