"""Any-hit queries (om_occluded_rays*, FrozenHittableList.occluded) and per-ray windows
(om_hit_rays_windows*, hit_rays(windows=...)) against the CPU oracle, ray by ray.

occluded(ray, tmin, tmax) must equal `oracle.World.hit(ray, tmin, tmax) is not None` for every ray,
and hit_rays(windows=...) must give oracle.World.hit's record for every ray's own window: every
comparison is exact and no ray is left out.  The ray sets are those of tests/test_gpu_query.py
((a) 48x32 pinhole rays, (b) one random direction from every hit point, (c) rays from random points
of the scene's bounds).

Per-ray windows (test_per_ray_windows): ray k gets class k mod 8, built in float32 from the oracle's
closest root t* of that ray in [0.001, 100] (1.0 for a miss):
  0 [.001, t*]   1 [.001, nextafter(t*, 0)]   2 [nextafter(t*, inf), 100]   3 [t*, 100]
  4 [.001, inf]  5 [.001, t* / 2]             6 [-1, 100]                   7 [.001, NaN]
These are where an early-exit kernel can go wrong: the traced tests accept root == tmax and a NaN
tmax, the march does neither; tmin < 0 and NaN bounds are windows the tree culls are not conservative
for.  test_windows_cut_both_ways shows from the oracle alone that the classes discriminate on these
rays (it prints the per-class counts and asserts only the qualitative conditions, no numeric floor
other than "more than half" for class 0 on the traced worlds).
"""
import ctypes as C

import numpy as np
import pytest

from scenes_common import kitchen_sink, tie_scene
from test_gpu_query import (F, H, KERNELS, REGIMES, SBVH_WORLDS, W, _Cache, _grid_bounds, compare_hits, edge, ray_sets,  # noqa: F401
                            zoo)                                 # (edge, zoo: module-scoped fixtures, shared by name)

pytestmark = pytest.mark.gpu

WINDOW_KERNELS = ["bvh2", "bvh4", "brute"]
WINDOW_WORLDS = ["kitchen", "sfull", "marched"]


@pytest.fixture(scope="module")
def cache(om, oracle):
    return _Cache(om, oracle)


def _occluded(w, rays, kernel="auto", **kw):
    fz = w.freeze(kernel=kernel)
    try:
        return fz.occluded(rays, **kw)
    finally:
        fz.close()


def check_occluded(got, exp, label):
    """got: the bool vector of occluded(); exp: the oracle's records of the same rays."""
    assert got.dtype == np.bool_ and got.shape == (len(exp),)
    assert set(got.view(np.uint8).tolist()) <= {0, 1}, f"{label}: a byte is neither 0 nor 1"
    want = exp["obj"] != 0
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{label}: {len(bad)}/{len(exp)} rays differ, first {bad[:8].tolist()} (oracle obj {exp['obj'][bad[:8]].tolist()})"


# ------------------------------------------------------------------ worlds x kernels, the call's window
@pytest.mark.parametrize("kernel", KERNELS)
def test_kitchen_sink_every_kernel(om, cache, kernel):
    w, rays, exp = cache.kitchen()
    assert (exp["obj"] != 0).any() and (exp["obj"] == 0).any()
    check_occluded(_occluded(w, rays, kernel), exp, f"kitchen_sink/{kernel}")


@pytest.mark.parametrize("kernel", ["bvh2", "bvh4"])
@pytest.mark.parametrize("name", REGIMES)
def test_tree_regimes(om, cache, name, kernel):
    w, rays, exp = cache.regime(name)
    check_occluded(_occluded(w, rays, kernel), exp, f"{name}/{kernel}")


@pytest.mark.parametrize("name", SBVH_WORLDS)
def test_sbvh_staging_cut(om, cache, name):
    w, rays, exp = cache.regime(name)
    check_occluded(_occluded(w, rays, "sbvh"), exp, f"{name}/sbvh")


# ------------------------------------------------------------------ marched worlds
class _Worlds:
    """marched_scene and S-full (random_scene with the torus: traced and marched objects together)
    with their ray sets and oracle answers, built once per module."""

    def __init__(self, om, oracle, cache):
        self.om, self.oracle, self.cache, self.d = om, oracle, cache, {}

    def get(self, name):
        """-> (world, oracle world, rays, oracle records in [0.001, 100])"""
        if name not in self.d:
            om, O = self.om, self.oracle
            if name == "kitchen":
                w, rays, exp = self.cache.kitchen()
                self.d[name] = (w, kitchen_sink(om, O)[1], rays, exp)
            elif name == "marched":
                w, ow = om.marched_scene(), O.marched_scene()
                self.d[name] = (w, ow) + ray_sets(om, ow, om.default_camera(W / H), (-4., -0.3, -4.), (4., 2.5, 4.))
            else:
                w, ow = om.random_scene(0x5EED, with_torus=True), O.random_scene(0x5EED, with_torus=True)
                lo, hi = _grid_bounds("g11")
                self.d[name] = (w, ow) + ray_sets(om, ow, om.default_camera(W / H), lo, hi)
        return self.d[name]


@pytest.fixture(scope="module")
def worlds(om, oracle, cache):
    return _Worlds(om, oracle, cache)


def test_marched_scene(om, worlds):
    w, _, rays, exp = worlds.get("marched")
    assert len(set(int(x) for x in exp["obj"])) >= 4
    check_occluded(_occluded(w, rays), exp, "marched_scene")


@pytest.mark.parametrize("steps", [512, 7])
def test_marched_zoo_with_sdf_program(om, zoo, steps):
    w, sets = zoo
    rays, exp = sets[steps]
    assert int(exp["obj"].max()) == 9                            # the program object (last id) is hit
    check_occluded(_occluded(w, rays, march_steps=steps), exp, f"marched zoo/{steps} steps")


@pytest.mark.parametrize("kernel", ["auto", "bvh4", "brute"])
def test_s_full_traced_and_marched_together(om, worlds, kernel):
    w, _, rays, exp = worlds.get("sfull")
    torus = int(exp["obj"].max())
    assert (exp["obj"] == torus).sum() > 10 and len(set(exp["obj"].tolist())) > 100   # the torus (last id) and the field
    check_occluded(_occluded(w, rays, kernel), exp, f"S-full/{kernel}")


# ------------------------------------------------------------------ per-ray windows
def class_windows(om, exp):
    """The window of ray k: class k mod 8 of the module docstring, in float32."""
    n = len(exp)
    t = exp["t"].astype(F).copy()
    t[exp["obj"] == 0] = F(1.0)
    k = np.arange(n) % 8
    tmin, tmax = np.full(n, F(0.001), F), np.full(n, F(100.0), F)
    tmax[k == 0] = t[k == 0]
    tmax[k == 1] = np.nextafter(t[k == 1], F(0.0))
    tmin[k == 2] = np.nextafter(t[k == 2], F(np.inf))
    tmin[k == 3] = t[k == 3]
    tmax[k == 4] = F(np.inf)
    tmax[k == 5] = (t[k == 5] / F(2.0)).astype(F)
    tmin[k == 6] = F(-1.0)
    tmax[k == 7] = F(np.nan)
    win = np.zeros(n, dtype=om.WINDOW_DTYPE)
    win["tmin"], win["tmax"] = tmin, tmax
    return win


def oracle_hits_windows(om, ow, rays, win):
    out = np.zeros(len(rays), dtype=om.HIT_DTYPE)
    out["t"] = np.inf
    for k, r in enumerate(rays):
        h = ow.hit(r[:3], r[3:], win["tmin"][k], win["tmax"][k])
        if h is not None:
            out[k] = (h[0][0], h[0][1:4], h[0][4:7], h[1])
    return out


@pytest.fixture(scope="module")
def windowed(om, worlds):
    """Per world: (world, rays, base records, windows, oracle records of every ray's own window)."""
    d = {}

    def get(name):
        if name not in d:
            w, ow, rays, exp = worlds.get(name)
            win = class_windows(om, exp)
            d[name] = (w, rays, exp, win, oracle_hits_windows(om, ow, rays, win))
        return d[name]
    return get


@pytest.mark.parametrize("kernel", WINDOW_KERNELS)
@pytest.mark.parametrize("name", WINDOW_WORLDS)
def test_per_ray_windows(om, windowed, name, kernel):
    """occluded(windows=) and hit_rays(windows=) == the oracle with every ray's own window; the
    windows both as an n-vector of WINDOW_DTYPE and as an (n, 2) float32 array."""
    w, rays, _, win, wexp = windowed(name)
    fz = w.freeze(kernel=kernel)
    try:
        check_occluded(fz.occluded(rays, windows=win), wexp, f"{name}/{kernel} occluded(windows)")
        got = fz.hit_rays(rays, windows=np.ascontiguousarray(win.view(F).reshape(-1, 2)))
        assert np.array_equal(got["obj"], wexp["obj"]), f"{name}/{kernel}: obj differs on {int((got['obj'] != wexp['obj']).sum())} rays"
        compare_hits(got, wexp, f"{name}/{kernel} hit_rays(windows)", nan_payload=True)
    finally:
        fz.close()


@pytest.mark.parametrize("name", WINDOW_WORLDS)
def test_windows_cut_both_ways(windowed, name):
    """From the oracle alone: the window classes decide rays.  Among the rays that hit in
    [0.001, 100]: classes 0 and 2 (traced worlds) and 2 and 3 (marched_scene) hold occluded and
    unoccluded rays; class 3 ([t*, 100]) is all occluded in the traced worlds, where the closest
    root is a traced one and the traced tests accept root == tmin (the reference alone gives 281 of
    281 and 347 of 347 here, so "both ways" cannot be asked of it; marched_scene's march restarts
    from tmin and gives 63 of 271); classes 1 and 5 are all unoccluded (nothing is closer than the
    closest root);
    class 0 is all unoccluded in marched_scene (the march's t < tmax) and mostly occluded in the
    traced worlds (the traced tests' root <= tmax); class 6 (tmin = -1) turns misses into hits."""
    _, rays, exp, win, wexp = windowed(name)
    k = np.arange(len(rays)) % 8
    hit, occ = exp["obj"] != 0, wexp["obj"] != 0
    counts = {c: (int((occ & hit & (k == c)).sum()), int((hit & (k == c)).sum())) for c in range(8)}
    miss_to_hit = int((occ & ~hit & (k == 6)).sum())
    print(f"{name}: occluded / hit rays per class {counts}; class 6 misses that became hits: {miss_to_hit} "
          f"of {int((~hit & (k == 6)).sum())}")
    both = (0, 2) if name != "marched" else (2, 3)
    for c in both:
        assert 0 < counts[c][0] < counts[c][1], f"class {c}: {counts[c]}"
    if name != "marched":                                       # root == tmin is accepted by every traced test
        assert counts[3][0] == counts[3][1] > 0, f"class 3: {counts[3]}"
    for c in (1, 5):
        assert counts[c][0] == 0 and counts[c][1] > 0, f"class {c}: {counts[c]}"
    assert miss_to_hit >= 1
    if name == "marched":                                       # the march: t < tmax, and no start under a NaN tmax
        assert counts[0][0] == 0 and counts[0][1] > 0 and counts[7][0] == 0 and counts[7][1] > 0
    else:                                                       # the traced tests: root <= tmax, NaN tmax accepted
        assert 2 * counts[0][0] > counts[0][1] and 2 * counts[7][0] > counts[7][1]
    assert (~np.isfinite(win["tmax"])).sum() >= len(rays) // 8 * 2      # the inf and NaN classes are present


@pytest.mark.parametrize("kernel", WINDOW_KERNELS)
def test_equal_windows_are_the_call_form(om, worlds, kernel):
    w, _, rays, _ = worlds.get("sfull")
    fz = w.freeze(kernel=kernel)
    try:
        for tmin, tmax in ((0.001, 100.0), (0.001, 2.5)):
            win = np.zeros(len(rays), dtype=om.WINDOW_DTYPE)
            win["tmin"], win["tmax"] = F(tmin), F(tmax)
            a, b = fz.occluded(rays, tmin, tmax), fz.occluded(rays, 5.0, 6.0, windows=win)
            assert a.tobytes() == b.tobytes(), f"{kernel} [{tmin}, {tmax}]: occluded differs from the call form"
            ha, hb = fz.hit_rays(rays, tmin, tmax), fz.hit_rays(rays, 5.0, 6.0, windows=win)
            assert ha.tobytes() == hb.tobytes(), f"{kernel} [{tmin}, {tmax}]: hit_rays differs from the call form"
            assert np.array_equal(a, ha["obj"] != 0)
        assert 0 < int(a.sum()) < int(fz.occluded(rays).sum())      # [0.001, 2.5] cuts hits off
    finally:
        fz.close()


# ------------------------------------------------------------------ ray counts, output bounds
def test_ray_counts_partial_waves_blocks_and_looping_workgroups(om, cache):
    from raytracingoneweekend_amd import _lib
    w, rays, exp = cache.regime("g11")
    fz = w.freeze(kernel="bvh2")
    grid = fz.query_max_grid()
    assert grid > 0 and grid % 4 == 0
    big_n = 4 * _lib.OM_QUERY_BLOCK * grid + 3
    big_rays = np.ascontiguousarray(np.resize(rays, (big_n, 6)))
    big = fz.occluded(big_rays)
    check_occluded(big[:len(rays)], exp, "g11/large call head")
    want = np.resize(exp["obj"] != 0, big_n)
    assert np.array_equal(big, want), "repeated rays of the large call gave different answers"
    for n in (1, 63, 64, 65, 511, 512, 513):
        got = fz.occluded(big_rays[:n])
        assert got.tobytes() == big[:n].tobytes(), f"n = {n} differs from the head of the large call"
    fz.close()


def test_output_bytes_stay_inside_the_array(om, cache):
    """The device form with the output at byte offsets 0..3 of a 0xAA-filled buffer with 64 guard
    bytes on each side: the guards stay, every byte of [0, n) is 0 or 1 and equals the oracle.  Run
    with the rays and the windows 8-byte aligned, and with both at a 4-byte-only alignment."""
    import torch
    from raytracingoneweekend_amd import _lib as L
    w, rays, exp = cache.regime("g11")
    want = (exp["obj"] != 0).astype(np.uint8)
    n_all = len(rays)
    fz = w.freeze(kernel="bvh2")
    s = torch.cuda.Stream()
    q = L.om_query_params(5.0, 6.0, 1024, 0)                     # the per-ray windows replace it
    d_rays = torch.from_numpy(rays).cuda()
    d_win = torch.tensor([0.001, 100.0], dtype=torch.float32, device="cuda").repeat(n_all, 1).contiguous()
    pad_r = torch.zeros(n_all * 6 + 1, dtype=torch.float32, device="cuda")
    pad_w = torch.zeros(n_all * 2 + 1, dtype=torch.float32, device="cuda")
    pad_r[1:] = d_rays.reshape(-1)
    pad_w[1:] = d_win.reshape(-1)
    torch.cuda.synchronize()
    assert d_rays.data_ptr() % 8 == 0 and d_win.data_ptr() % 8 == 0 and pad_r.data_ptr() % 8 == 0 and pad_w.data_ptr() % 8 == 0
    for rp, wp, label in ((d_rays.data_ptr(), d_win.data_ptr(), "aligned"), (pad_r.data_ptr() + 4, pad_w.data_ptr() + 4, "4-byte")):
        for n in (1, 63, 64, 65, 511, 512, 513, n_all):
            for off in range(4):
                buf = torch.full((64 + off + n + 64,), 0xAA, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                L.check(L.lib.om_occluded_rays_device(fz.ctx, C.byref(q), C.c_void_p(rp), C.c_void_p(wp), n,
                                                      C.c_void_p(buf.data_ptr() + 64 + off), C.c_void_p(s.cuda_stream)), fz.ctx)
                s.synchronize()
                b = buf.cpu().numpy()
                assert (b[:64 + off] == 0xAA).all() and (b[64 + off + n:] == 0xAA).all(), f"{label} n {n} offset {off}: guard bytes written"
                assert len(b[64 + off + n:]) == 64
                assert np.array_equal(b[64 + off:64 + off + n], want[:n]), f"{label} n {n} offset {off}: differs from the oracle"
    fz.close()


# ------------------------------------------------------------------ edge rays, ties
@pytest.mark.parametrize("kernel", WINDOW_KERNELS)
def test_edge_rays(om, cache, edge, kernel):
    """Rays with NaN / inf components under EDGE_WINDOWS (tmin > tmax, tmax = inf, tmin = 0), as the
    call's window and as per-ray windows: only obj != 0 is compared."""
    w = cache.kitchen()[0]
    both, answers = edge
    fz = w.freeze(kernel=kernel)
    for (tmin, tmax), exp in answers.items():
        check_occluded(fz.occluded(both, tmin, tmax), exp, f"edge/{kernel} [{tmin}, {tmax}]")
        win = np.zeros(len(both), dtype=om.WINDOW_DTYPE)
        win["tmin"], win["tmax"] = F(tmin), F(tmax)
        check_occluded(fz.occluded(both, windows=win), exp, f"edge/{kernel} windows [{tmin}, {tmax}]")
    fz.close()


def test_tie_scene(om, oracle):
    w, ow = tie_scene(om, oracle)
    rays, exp = ray_sets(om, ow, om.default_camera(W / H), (-6., -0.3, -6.), (6., 2.5, 6.))
    assert 131 in set(int(x) for x in exp["obj"])
    for kernel in WINDOW_KERNELS:
        check_occluded(_occluded(w, rays, kernel), exp, f"ties/{kernel}")


# ------------------------------------------------------------------ entry points
def _params(L, tmin=0.001, tmax=100.0, steps=1024, reserved=0):
    return L.om_query_params(tmin, tmax, steps, reserved)


def test_status_codes(om, cache):
    from raytracingoneweekend_amd import _lib as L
    w, rays, exp = cache.regime("g11")
    some = np.concatenate([np.nonzero(exp["obj"])[0][:5], np.nonzero(exp["obj"] == 0)[0][:3]])
    r = np.ascontiguousarray(rays[some])
    win = np.zeros(8, dtype=om.WINDOW_DTYPE)
    win["tmin"], win["tmax"] = F(0.001), F(100.0)
    occ = np.full(8, 0xAA, dtype=np.uint8)
    hits = np.full(8 * 32, 0xAA, dtype=np.uint8)
    rp, wp = r.ctypes.data_as(C.c_void_p), win.ctypes.data_as(C.c_void_p)
    op, hp = occ.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p)
    ctx = C.c_void_p()
    L.check(L.lib.om_create(0, C.byref(ctx)))
    q = _params(L)
    lib = L.lib
    for wins in (wp, None):                                                        # before om_upload_world
        assert lib.om_occluded_rays(ctx, C.byref(q), rp, wins, 8, op) == L.OM_ERR_STATE
        assert lib.om_occluded_rays_device(ctx, C.byref(q), rp, wins, 8, op, None) == L.OM_ERR_STATE
        assert lib.om_hit_rays_windows(ctx, C.byref(q), rp, wins, 8, hp) == L.OM_ERR_STATE
        assert lib.om_hit_rays_windows_device(ctx, C.byref(q), rp, wins, 8, hp, None) == L.OM_ERR_STATE
    L.check(lib.om_upload_world(ctx, w.handle), ctx)
    assert lib.om_occluded_rays(ctx, C.byref(q), rp, wp, 0, op) == L.OM_OK
    assert lib.om_occluded_rays(ctx, C.byref(q), None, None, 0, None) == L.OM_OK     # n == 0 launches nothing
    assert lib.om_occluded_rays_device(ctx, C.byref(q), None, None, 0, None, None) == L.OM_OK
    assert lib.om_hit_rays_windows(ctx, C.byref(q), None, None, 0, None) == L.OM_OK
    assert lib.om_hit_rays_windows_device(ctx, C.byref(q), None, None, 0, None, None) == L.OM_OK
    for wins in (wp, None):
        assert lib.om_occluded_rays(ctx, None, rp, wins, 8, op) == L.OM_ERR_INVALID
        assert lib.om_occluded_rays(ctx, C.byref(q), None, wins, 8, op) == L.OM_ERR_INVALID
        assert lib.om_occluded_rays(ctx, C.byref(q), rp, wins, 8, None) == L.OM_ERR_INVALID
        assert lib.om_occluded_rays_device(ctx, C.byref(q), None, wins, 8, None, None) == L.OM_ERR_INVALID
        assert lib.om_hit_rays_windows(ctx, None, rp, wins, 8, hp) == L.OM_ERR_INVALID
        assert lib.om_hit_rays_windows(ctx, C.byref(q), None, wins, 8, hp) == L.OM_ERR_INVALID
        assert lib.om_hit_rays_windows(ctx, C.byref(q), rp, wins, 8, None) == L.OM_ERR_INVALID
        for bad in (_params(L, reserved=1), _params(L, tmin=float("nan")), _params(L, tmax=float("nan"))):
            assert lib.om_occluded_rays(ctx, C.byref(bad), rp, wins, 8, op) == L.OM_ERR_INVALID   # q is validated with windows too
            assert lib.om_occluded_rays_device(ctx, C.byref(bad), rp, wins, 8, op, None) == L.OM_ERR_INVALID
            assert lib.om_hit_rays_windows(ctx, C.byref(bad), rp, wins, 8, hp) == L.OM_ERR_INVALID
            assert lib.om_hit_rays_windows_device(ctx, C.byref(bad), rp, wins, 8, hp, None) == L.OM_ERR_INVALID
    assert (occ == 0xAA).all() and (hits == 0xAA).all()                             # no failed call wrote anything
    assert lib.om_occluded_rays(ctx, C.byref(q), rp, wp, 8, op) == L.OM_OK
    assert occ.tolist() == [1, 1, 1, 1, 1, 0, 0, 0]
    occ[:] = 0xAA
    assert lib.om_occluded_rays(ctx, C.byref(q), rp, None, 8, op) == L.OM_OK
    assert occ.tolist() == [1, 1, 1, 1, 1, 0, 0, 0]
    assert lib.om_hit_rays_windows(ctx, C.byref(q), rp, wp, 8, hp) == L.OM_OK
    assert hits.tobytes() == exp[some].tobytes()
    lib.om_destroy(ctx)


def test_python_argument_errors(om, cache):
    import torch
    w, rays, _ = cache.regime("g11")
    fz = w.freeze()
    n = len(rays)
    good = np.zeros((n, 2), dtype=F)
    for bad in (good[:-1], good.astype(np.float64), np.zeros((n, 3), dtype=F), np.zeros(n, dtype=F),
                torch.zeros((n, 2), dtype=torch.float32)):
        with pytest.raises(ValueError):
            fz.occluded(rays, windows=bad)
        with pytest.raises(ValueError):
            fz.hit_rays(rays, windows=bad)
    d_rays = torch.from_numpy(rays).cuda()
    for bad in (good, torch.zeros((n, 2), dtype=torch.float32), torch.zeros((n, 2), dtype=torch.float64, device="cuda"),
                torch.zeros((n - 1, 2), dtype=torch.float32, device="cuda")):
        with pytest.raises(ValueError):
            fz.occluded(d_rays, windows=bad)
        with pytest.raises(ValueError):
            fz.hit_rays(d_rays, windows=bad)
    with pytest.raises(ValueError):
        fz.occluded(d_rays, out=torch.zeros(n, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        fz.occluded(d_rays, stream=0)
    with pytest.raises(ValueError):
        fz.occluded(np.zeros((4, 5), dtype=F))
    fz.close()


def test_device_entry_point_streams_counters_and_progress(om, cache):
    """Torch tensors through om_occluded_rays_device == the host form; two occlusion queries queued
    between two om_render_device calls on one stream leave the frame equal to the renders alone;
    counters: segments == n, samples == credited == 0; the om_progress word untouched."""
    import torch
    from raytracingoneweekend_amd import _lib as L
    w, rays, exp = cache.regime("g11")
    cam = om.default_camera(W / H)
    n = len(rays)
    p = om.make_params(50, 0.001, 100.0, 4, W, H, sample_count=2, seed=11)

    def render_pair(fz, frame, st, between=None):
        L.check(L.lib.om_render_device(fz.ctx, C.byref(cam.raw), C.byref(p), C.c_void_p(frame.data_ptr()), C.c_void_p(st)), fz.ctx)
        out = between() if between else None
        L.check(L.lib.om_render_device(fz.ctx, C.byref(cam.raw), C.byref(p), C.c_void_p(frame.data_ptr()), C.c_void_p(st)), fz.ctx)
        return out

    s = torch.cuda.Stream()
    fz = w.freeze()
    ref_frame = torch.zeros(W * H * 40, dtype=torch.uint8, device="cuda")
    render_pair(fz, ref_frame, s.cuda_stream)
    s.synchronize()
    host = fz.occluded(rays)
    check_occluded(host, exp, "g11/host entry point")
    win_np = np.zeros((n, 2), dtype=F)
    win_np[:, 0], win_np[:, 1] = F(0.001), F(3.0)
    host_win = fz.occluded(rays, windows=win_np)
    assert 0 < int(host_win.sum()) < int(host.sum())
    fz.close()

    fz = w.freeze()
    prog = L.lib.om_progress(fz.ctx)
    assert prog and prog[0] == 0
    d_rays = torch.from_numpy(rays).cuda()
    d_win = torch.from_numpy(win_np).cuda()
    frame = torch.zeros(W * H * 40, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L.check(L.lib.om_reset_counters(fz.ctx, C.c_void_p(s.cuda_stream)), fz.ctx)
    o1 = fz.occluded(d_rays, stream=s.cuda_stream)                 # alone: segments == n, samples == 0
    s.synchronize()
    assert o1.dtype == torch.uint8 and tuple(o1.shape) == (n,) and o1.device == d_rays.device
    ctr = fz.counters()
    assert ctr["segments"] == n and ctr["samples"] == 0 and ctr["credited"] == 0
    assert ctr["prim_tests"] > 0 and ctr["pre_tests"] > 0 and ctr["march_steps"] == 0
    assert prog[0] == 0

    def two_queries():
        return fz.occluded(d_rays, stream=s.cuda_stream), fz.occluded(d_rays, windows=d_win, stream=s.cuda_stream)

    before = prog[0]
    q1, q2 = render_pair(fz, frame, s.cuda_stream, two_queries)
    s.synchronize()
    assert torch.equal(frame, ref_frame), "renders around the queries differ from the renders alone"
    credited = fz.counters()["credited"]
    assert prog[0] - before == credited == 4 * W * H                # the renders' credit only
    for got, want, label in ((o1, host, "device"), (q1, host, "queued 1"), (q2, host_win, "queued 2")):
        assert got.cpu().numpy().tobytes() == want.view(np.uint8).tobytes(), f"{label}: differs from the host entry point"
    hw = fz.hit_rays(d_rays, windows=d_win, stream=s.cuda_stream)   # the windowed closest-hit device form
    s.synchronize()
    assert np.array_equal(hw.cpu().numpy().view(om.HIT_DTYPE).reshape(-1)["obj"] != 0, host_win)
    fz.close()


def test_torch_default_stream_is_ordered_with_the_query(om, cache):
    """occluded(tensor) with no stream= while torch is on its null stream: rays made by torch ops
    queued just before, the result read by torch right after, no synchronise in between."""
    import torch
    w, rays, exp = cache.regime("g11")
    fz = w.freeze()
    host = fz.occluded(rays)
    check_occluded(host, exp, "g11/host entry point")
    assert torch.cuda.current_stream().cuda_stream == 0
    src = torch.from_numpy(rays).cuda()
    torch.cuda.synchronize()
    for _ in range(3):
        big = torch.ones((1 << 24,), dtype=torch.float32, device="cuda")
        for _ in range(20):                                       # work queued ahead of the rays' producer
            big = big * 1.0
        d_rays = (src * big[:1]).contiguous()                     # src * 1.0: the same bits, made on the device
        got = fz.occluded(d_rays)                                 # no stream=, no synchronise
        flat = got.clone()                                        # a torch reader on the null stream
        assert flat.cpu().numpy().tobytes() == host.view(np.uint8).tobytes()
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):                                # a non-null current stream is used as it is
        got = fz.occluded(src.clone())
        assert got.cpu().numpy().tobytes() == host.view(np.uint8).tobytes()
    fz.close()


# ------------------------------------------------------------------ early exit
def _counted(fz, fn):
    from raytracingoneweekend_amd import _lib as L
    L.check(L.lib.om_reset_counters(fz.ctx, None), fz.ctx)
    fn()
    return fz.counters()


def test_early_exit_is_real(om, worlds):
    """Counting on, kernel brute, S-full: the any-hit loop is a strict prefix of the reference loop
    for every ray that hits before the last object, so occluded() runs strictly fewer exact tests
    than hit_rays(); rays a traced object answered never march, so it takes strictly fewer march
    steps.  The tree kernels' counts are only printed."""
    from raytracingoneweekend_amd import _lib as L
    w, _, rays, exp = worlds.get("sfull")
    n = len(rays)
    for kernel in ("brute", "bvh2", "bvh4"):
        fz = w.freeze(kernel=kernel)
        L.check(L.lib.om_set_counting(fz.ctx, 1), fz.ctx)
        any_hit = _counted(fz, lambda: fz.occluded(rays))
        closest = _counted(fz, lambda: fz.hit_rays(rays))
        fz.close()
        print(f"S-full/{kernel}: prim_tests {any_hit['prim_tests']} vs {closest['prim_tests']}, pre_tests "
              f"{any_hit['pre_tests']} vs {closest['pre_tests']}, march_steps {any_hit['march_steps']} vs {closest['march_steps']}")
        assert any_hit["segments"] == closest["segments"] == n
        assert any_hit["samples"] == any_hit["credited"] == 0
        if kernel == "brute":
            assert 0 < any_hit["prim_tests"] < closest["prim_tests"]
            assert 0 < any_hit["march_steps"] < closest["march_steps"]
