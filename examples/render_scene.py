"""Headless counterpart of the reference front-end (main.rs:123-214 + draw_to_sdl):
compose random_scene through the Camera/Material/HittableList API, render it
progressively on the GPU like the reference's render threads (adaptive retirement
by default, --fixed-spp to take every sample), then save every display view (keys 0-6 of main.rs:360-367) as BMP/PPM —
the F12 save of main.rs:473-476.

    python examples/render_scene.py --width 1000 --height 666 --spp 200 --out out/
    python examples/render_scene.py --width 1000 --height 666 --pick 500 400      # what is under a pixel
    python examples/render_scene.py --width 1000 --height 666 --ao 16 0.5         # ambient occlusion, out/ao.bmp
    python examples/render_scene.py --mesh model.obj --spp 64                     # a triangle mesh over the ground
    python examples/render_scene.py --camera fisheye --spp 32                     # another camera model, out/fisheye.bmp
    python examples/render_scene.py --camera pano --spp 64                        # a 360 degree frame with every view saved
    python examples/render_scene.py --wave 8 --spp 32                             # a moving heightfield, refitted in place per frame
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import raytracingoneweekend_amd as om  # noqa: E402
from raytracingoneweekend_amd import _lib as L  # noqa: E402


def pick(world, frozen, cam, W, H, x, y):
    """The object under pixel (x, y): its centre ray from a pinhole at the camera origin (no lens
    offset), built here on the host in f32, through FrozenHittableList.hit."""
    F = np.float32
    r = cam.raw
    org, hor, ver, llc = (np.array(list(v), dtype=F) for v in (r.origin, r.horizontal, r.vertical, r.lower_left_corner))
    u, v = (F(x) + F(0.5)) / F(W), F(1.0) - (F(y) + F(0.5)) / F(H)
    d = llc + u * hor + v * ver - org
    d = (d / np.sqrt((d * d).sum(dtype=F), dtype=F)).astype(F)
    h = frozen.hit(org, d)
    if h is None:
        print(f"pixel ({x}, {y}): sky")
        return
    print(f"pixel ({x}, {y}): obj {h.obj}, t {h.t:.6g}, point {tuple(float(c) for c in h.point)}, {world.material_of(h.obj)}")


def pinhole_rays(cam, W, H):
    """(W*H, 6) float32 centre rays of the frame, row-major, from a pinhole at the camera origin."""
    F = np.float32
    r = cam.raw
    org, hor, ver, llc = (np.array(list(v), dtype=F) for v in (r.origin, r.horizontal, r.vertical, r.lower_left_corner))
    j, i = np.meshgrid(np.arange(H, dtype=F), np.arange(W, dtype=F), indexing="ij")
    u = ((i.reshape(-1) + F(0.5)) / F(W)).astype(F)
    v = (F(1.0) - (j.reshape(-1) + F(0.5)) / F(H)).astype(F)
    d = (llc[None, :] + u[:, None] * hor[None, :] + v[:, None] * ver[None, :] - org[None, :]).astype(F)
    d = (d / np.sqrt((d * d).sum(axis=1, dtype=F), dtype=F)[:, None]).astype(F)
    return np.ascontiguousarray(np.concatenate([np.broadcast_to(org, d.shape), d], axis=1), dtype=F)


def ambient_occlusion(frozen, cam, W, H, samples, radius, seed):
    """Grey (H, W, 3) u8 image: per pixel, the share of `samples` seeded hemisphere rays of length
    `radius` from its primary hit point that reach nothing (sky pixels stay white).  Primary hits
    through hit_rays; the AO rays through occluded() with the per-ray window [0.001, radius]."""
    F = np.float32
    hits = frozen.hit_rays(pinhole_rays(cam, W, H))
    on = np.nonzero(hits["obj"])[0]
    n = hits["normal"][on]
    n = (n / np.sqrt((n * n).sum(axis=1, dtype=F), dtype=F)[:, None]).astype(F)      # cube normals are not unit
    rng = np.random.default_rng(seed)
    win = np.zeros(len(on), dtype=om.WINDOW_DTYPE)
    win["tmin"], win["tmax"] = F(0.001), F(radius)
    open_count = np.zeros(len(on), dtype=np.uint32)
    for _ in range(samples):
        d = rng.standard_normal((len(on), 3)).astype(F)
        d = (d / np.sqrt((d * d).sum(axis=1, dtype=F), dtype=F)[:, None]).astype(F)
        d = np.where((d * n).sum(axis=1, dtype=F)[:, None] < 0, -d, d).astype(F)
        rays = np.ascontiguousarray(np.concatenate([hits["point"][on], d], axis=1), dtype=F)
        open_count += ~frozen.occluded(rays, windows=win)
    grey = np.full(W * H, 255, dtype=np.uint8)
    grey[on] = np.round(255.0 * open_count / max(1, samples)).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(grey.reshape(H, W, 1), 3, axis=2))


def camera_rays(model, cam, W, H, device):
    """(W*H, 6) float32 centre rays of another camera model, built on the device with torch, row-major:
    fisheye (equidistant, 180 degrees across the frame's width), ortho (parallel rays over a 12-wide window) or
    equirect (a 360 x 180 degree panorama), all at the camera's origin, looking along -w."""
    import torch
    r = cam.raw
    t = lambda v: torch.tensor(list(v), dtype=torch.float32, device=device)
    org, cu, cv, cw = t(r.origin), t(r.u_of_plane), t(r.v_of_plane), t(r.w_of_plane)
    j, i = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=device),
                          torch.arange(W, dtype=torch.float32, device=device), indexing="ij")
    x = ((i.reshape(-1) + 0.5) / W * 2.0 - 1.0)                    # -1 .. 1 left to right
    y = (1.0 - (j.reshape(-1) + 0.5) / H * 2.0) * (H / W)          # up, same scale
    o = org.expand(W * H, 3)
    if model == "fisheye":
        rad = torch.sqrt(x * x + y * y).clamp_min(1e-12)
        theta = rad * (np.pi / 2.0)
        s = torch.sin(theta) / rad
        d = (x * s)[:, None] * cu + (y * s)[:, None] * cv - torch.cos(theta)[:, None] * cw
    elif model == "ortho":
        o = org + (6.0 * x)[:, None] * cu + (6.0 * y)[:, None] * cv
        d = (-cw).expand(W * H, 3)
    else:                                                           # equirect
        lon, lat = x * np.pi, (1.0 - (j.reshape(-1) + 0.5) / H * 2.0) * (np.pi / 2.0)
        d = (torch.cos(lat) * torch.sin(lon))[:, None] * cu + torch.sin(lat)[:, None] * cv \
            - (torch.cos(lat) * torch.cos(lon))[:, None] * cw
    d = d / torch.linalg.vector_norm(d, dim=1, keepdim=True)       # the unit-direction precondition
    return torch.cat([o, d], dim=1).contiguous()


def render_camera_model(frozen, cam, W, H, model, spp, max_depth, seed):
    """Mean of spp ray_color calls (sample = 0 .. spp-1, stream = the pixel index) -> (H, W, 3) u8 with
    the renderer's gamma (sqrt) and clamp."""
    import torch
    device = torch.device("cuda", int(frozen.device))
    rays = camera_rays(model, cam, W, H, device)
    acc = torch.zeros((W * H, 3), dtype=torch.float32, device=device)
    out = torch.empty((W * H, 5), dtype=torch.float32, device=device)
    for s in range(spp):
        frozen.ray_color(rays, max_depth=max_depth, seed=seed, sample=s, out=out)
        acc += out[:, :3]
    rgb = (acc / spp).clamp_min(0.0).sqrt().clamp(0.0, 0.999) * 256.0
    return np.ascontiguousarray(rgb.to(torch.uint8).reshape(H, W, 3).cpu().numpy())


def frame_rays(model, cam, W, H, samples, rng):
    """(samples, W*H, 6) float32 unit rays of a camera the renderer does not have, made on the host with
    numpy in float32, sample-major as render_rays reads them, every sample with a sub-pixel jitter of
    this example's own from `rng`:
      ortho  parallel rays along the view direction through a 12-wide view rectangle centred on lookfrom;
      pano   equirectangular, 360 x 180 degrees around lookfrom, the view direction in the middle."""
    F = np.float32
    r = cam.raw
    org, cu, cv, cw = (np.array(list(v), dtype=F) for v in (r.origin, r.u_of_plane, r.v_of_plane, r.w_of_plane))
    j, i = np.meshgrid(np.arange(H, dtype=F), np.arange(W, dtype=F), indexing="ij")
    i, j = i.reshape(1, -1), j.reshape(1, -1)
    jx, jy = rng.random((samples, W * H), dtype=F), rng.random((samples, W * H), dtype=F)
    x = ((i + jx) / F(W) * F(2.0) - F(1.0)).astype(F)              # -1 .. 1 left to right
    yv = (F(1.0) - (j + jy) / F(H) * F(2.0)).astype(F)             # 1 .. -1 top to bottom
    if model == "ortho":
        y = yv * F(H / W)
        o = org + (F(6.0) * x)[..., None] * cu + (F(6.0) * y)[..., None] * cv
        d = np.broadcast_to(-cw, o.shape)
    else:
        lon, lat = x * F(np.pi), yv * F(np.pi / 2.0)
        d = (np.cos(lat) * np.sin(lon))[..., None] * cu + np.sin(lat)[..., None] * cv - (np.cos(lat) * np.cos(lon))[..., None] * cw
        o = np.broadcast_to(org, d.shape)
    d = d.astype(F)
    d = (d / np.sqrt((d * d).sum(axis=2, dtype=F), dtype=F)[..., None]).astype(F)   # the unit-direction precondition
    return np.ascontiguousarray(np.concatenate([o.astype(F), d], axis=2), dtype=F)


def render_frame_camera(frozen, cam, W, H, model, args, pixels):
    """The progressive loop of main() with the model's rays in the place of the thin lens: per call
    `--per-call` samples through render_rays into the same Stats, adaptive retirement and credit as
    render() has them, default RNG streams (seed, pixel, Stats.n).  Returns the credited samples."""
    rng = np.random.default_rng(args.seed)
    credited = 0
    for done in range(0, args.spp, args.per_call):
        rays = frame_rays(model, cam, W, H, min(args.per_call, args.spp - done), rng)
        c = frozen.render_rays(pixels, rays, W, H, args.spp, max_depth=args.max_depth, adaptive=args.adaptive, seed=args.seed)
        credited += c["credited"]
        print(f"\r{100.0 * credited / (W * H * args.spp):5.1f}%", end="", flush=True)
        if credited >= W * H * args.spp:                            # every pixel is full or retired
            break
    return credited


def mesh_scene(path):
    """random_scene's ground sphere with the OBJ mesh standing on it: scaled to height 2, centred in x
    and z, one material, added with one add_triangles call."""
    v, f = om.load_obj(path)
    if len(f) == 0:
        raise SystemExit(f"{path}: no faces")
    lo, hi = v.min(axis=0), v.max(axis=0)
    scale = np.float32(2.0) / max(np.float32(1e-6), (hi - lo).max())
    mid = (lo + hi) * np.float32(0.5)
    v = ((v - np.array([mid[0], lo[1], mid[2]], dtype=np.float32)) * scale).astype(np.float32)
    world = om.HittableList.new()
    world += om.Sphere.new_with_radius((0., -1000., 0.), 1000.0, om.Material.new_lambertian((0.5, 0.5, 0.5)))
    world.add_triangles(v, f, om.Material.new_metal_fuzz((0.8, 0.7, 0.5), 0.05))
    print(f"{path}: {len(v)} vertices, {len(f)} triangles")
    return world


def wave_field(phase, cells=96):
    """a heightfield over [-4, 4]^2 whose sine's phase is `phase`"""
    f32 = np.float32
    fn = lambda x, z: (f32(0.35) * np.sin(f32(1.6) * x.astype(f32) + f32(phase), dtype=f32) * np.cos(f32(1.2) * z.astype(f32), dtype=f32)
                       + f32(0.45)).astype(f32)
    return om.heightfield(cells, cells, fn, extent=((-4.0, 4.0), (-4.0, 4.0)))


def render_wave(args, W, H):
    """--wave FRAMES: a short sequence of a heightfield whose phase advances per frame.  The world is
    frozen once; every later frame moves the mesh in place with FrozenHittableList.update_triangles
    (no re-upload, no rebuild) and renders it."""
    v, f = wave_field(0.0)
    world = om.HittableList.new()
    world += om.Sphere.new_with_radius((0.0, -1000.0, 0.0), 1000.0, om.Material.new_lambertian((0.5, 0.5, 0.5)))
    world += om.Sphere.new_with_radius((0.0, 1.6, 0.0), 0.7, om.Material.new_metal((0.8, 0.8, 0.9)))
    world.add_triangles(v, f, om.Material.new_lambertian((0.2, 0.5, 0.8)))
    cam = om.Camera.new((7.0, 4.5, 8.0), (0.0, 0.4, 0.0), (0.0, 1.0, 0.0), 35.0, W / H, 0.05, 11.0)
    frozen = world.freeze(cam)
    os.makedirs(args.out, exist_ok=True)
    for k in range(args.wave):
        t0 = time.perf_counter()
        if k:
            frozen.update_triangles(wave_field(0.35 * k)[0], f)
        t1 = time.perf_counter()
        pixels = om.PixelsBox.new(W * H)
        om.render(cam, frozen, args.max_depth, 0.001, 100.0, args.spp, W, H, pixels, seed=args.seed, adaptive=args.adaptive)
        path = os.path.join(args.out, f"wave_{k:03d}.{'ppm' if args.ppm else 'bmp'}")
        (om.write_ppm if args.ppm else om.write_bmp)(path, om.display(frozen, pixels, W, H, "normal"))
        print(f"frame {k}: update {1e3 * (t1 - t0):.2f} ms (host form, copies included), render {time.perf_counter() - t1:.3f} s, wrote {path}")
    print("updates:", frozen.update_info())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1000)           # main.rs:125-127
    ap.add_argument("--height", type=int, default=666)
    ap.add_argument("--spp", type=int, default=200)              # main.rs:145
    ap.add_argument("--max-depth", type=int, default=50)         # main.rs:146
    ap.add_argument("--per-call", type=int, default=8, help="samples per render call (progressive passes)")
    ap.add_argument("--fixed-spp", dest="adaptive", action="store_false",
                    help="take every sample of every pixel (default: retire converged pixels like the "
                         "reference's render threads, render_thread.rs:31-38,97-101)")
    ap.add_argument("--torus", action="store_true", help="include the marched torus block of main.rs:73-81")
    ap.add_argument("--mesh", metavar="FILE.obj",
                    help="render this Wavefront OBJ mesh (v / f lines) over the ground sphere instead of random_scene, "
                         "scaled to height 2 and centred on the origin; --pick and --ao work on it")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="out")
    ap.add_argument("--ppm", action="store_true", help="write PPM instead of BMP")
    ap.add_argument("--pick", type=int, nargs=2, metavar=("X", "Y"),
                    help="print the object id, t and material under the centre of pixel (X, Y) and exit (no render)")
    ap.add_argument("--ao", nargs=2, metavar=("SAMPLES", "RADIUS"),
                    help="write ao.bmp/ppm: ambient occlusion from SAMPLES any-hit rays of length RADIUS per primary hit "
                         "(FrozenHittableList.occluded), and exit (no render)")
    ap.add_argument("--camera", choices=("thinlens", "ortho", "pano", "fisheye", "equirect"), default="thinlens",
                    help="thinlens: the reference's camera through render().  ortho / pano: another camera's jittered rays, "
                         "made with numpy, rendered progressively into the same Stats through FrozenHittableList.render_rays "
                         "(adaptive retirement, every view saved).  fisheye / equirect: centre rays built on the device with "
                         "torch and averaged from FrozenHittableList.ray_color, --spp calls of one sample each; writes "
                         "MODEL.bmp/ppm and exits")
    ap.add_argument("--wave", type=int, metavar="FRAMES",
                    help="render FRAMES frames of a heightfield whose phase advances per frame, moved in place between "
                         "frames with FrozenHittableList.update_triangles (wave_000.bmp ...), and exit")
    args = ap.parse_args()

    W, H = args.width, args.height
    if args.wave:
        render_wave(args, W, H)
        return
    if args.mesh:
        world = mesh_scene(args.mesh)
        cam = om.Camera.new((5.0, 2.5, 6.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 30.0, W / H, 0.05, 8.0)
    else:
        world = om.random_scene_api(0x5EED, with_torus=args.torus)   # main.rs:37-100 through the API
        cam = om.Camera.new((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 20.0, W / H, 0.1, 10.0)  # main.rs:136-142
    frozen = world.freeze(cam)
    if args.mesh:
        ti = frozen.tree_info()      # which BVH2 regime the mesh landed in
        print(f"tree: {ti['records']} records, {ti['b2_nodes']} nodes, depth {ti['b2_depth']}, regime {ti['regime']}, "
              f"{ti['lds_bytes']} B of LDS per workgroup")
    if args.pick:
        if not (0 <= args.pick[0] < W and 0 <= args.pick[1] < H):
            ap.error("--pick: the pixel is outside the frame")
        pick(world, frozen, cam, W, H, *args.pick)
        return
    if args.ao:
        samples, radius = int(args.ao[0]), float(args.ao[1])
        if samples < 1 or not radius > 0.001:
            ap.error("--ao: need SAMPLES >= 1 and RADIUS > 0.001")
        t0 = time.perf_counter()
        rgb = ambient_occlusion(frozen, cam, W, H, samples, radius, args.seed)
        print(f"{W}x{H} ambient occlusion, {samples} rays of length {radius} per hit point, in {time.perf_counter() - t0:.3f} s")
        os.makedirs(args.out, exist_ok=True)
        path = os.path.join(args.out, f"ao.{'ppm' if args.ppm else 'bmp'}")
        (om.write_ppm if args.ppm else om.write_bmp)(path, rgb)
        print("wrote", path)
        return
    if args.camera in ("fisheye", "equirect"):
        t0 = time.perf_counter()
        rgb = render_camera_model(frozen, cam, W, H, args.camera, args.spp, args.max_depth, args.seed)
        dt = time.perf_counter() - t0
        print(f"{W}x{H}x{args.spp} {args.camera} in {dt:.3f} s ({W * H * args.spp / dt / 1e6:.0f} Mpaths/s)")
        os.makedirs(args.out, exist_ok=True)
        path = os.path.join(args.out, f"{args.camera}.{'ppm' if args.ppm else 'bmp'}")
        (om.write_ppm if args.ppm else om.write_bmp)(path, rgb)
        print("wrote", path)
        return
    pixels = om.PixelsBox.new(W * H)
    t0, credited = time.perf_counter(), 0
    if args.camera != "thinlens":
        credited = render_frame_camera(frozen, cam, W, H, args.camera, args, pixels)
    else:
        for done in range(0, args.spp, args.per_call):
            c = om.render(cam, frozen, args.max_depth, 0.001, 100.0, args.spp, W, H, pixels, seed=args.seed,
                          adaptive=args.adaptive, sample_count=min(args.per_call, args.spp - done))
            credited += c["credited"]
            print(f"\r{100.0 * credited / (W * H * args.spp):5.1f}%", end="", flush=True)   # main.rs:151-168 log
    dt = time.perf_counter() - t0
    print(f"\n{W}x{H}x{args.spp} {args.camera} in {dt:.3f} s ({W * H * args.spp / dt / 1e6:.0f} Msamples/s credited)")
    os.makedirs(args.out, exist_ok=True)
    for view in L.VIEWS:
        rgb = om.display(frozen, pixels, W, H, view)
        path = os.path.join(args.out, f"{view}.{'ppm' if args.ppm else 'bmp'}")
        (om.write_ppm if args.ppm else om.write_bmp)(path, rgb)
        print("wrote", path)


if __name__ == "__main__":
    main()
