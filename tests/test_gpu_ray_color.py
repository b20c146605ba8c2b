"""Radiance queries (om_ray_color*, FrozenHittableList.ray_color) against the CPU oracle, ray by ray.

The reference of every ray is the oracle's own one-sample render: one pixel, one sample of
oracle.render is ray_color of one ray (paths_common.py derives that ray and the RNG state with which
the sample enters ray_color).  A record must equal the oracle's Stats of that sample as bits:
color + 0.0 == sum, depth == avg_depth, obj == the id of oracle.World.hit(ray).

Set 1: the 1536 samples of a 48x32 frame of the world's camera, seed 7.
Set 2: 512 rays from first-hit points of set 1, each through an aperture-0 camera of its own (2x2
frame, pixel 0, seed 1000 + k), and, in a call of their own with tmax 2e4, four rays from about 1e4 away.

Witness thresholds, measured with the oracle alone on the CPU (80 % of the smallest value of each row):
  set 1, share that hits at segment 0:       g11 0.7845, g50x 0.8477, kitchen_sink 0.7389 -> asserted >= 0.591
  set 1, share that misses at segment 0:     g11 0.2155, g50x 0.1523, kitchen_sink 0.2611 -> asserted >= 0.121
  set 1 at depth 2, share exhausted (colour 0, finite depth):
                                             g11 0.3268, g50x 0.3366, kitchen_sink 0.2279 -> asserted >= 0.182
  set 1, paths with 2 or more disc tries:    352 of 1536 in all three (the streams are the frame's: 1184 / 284 /
                                             53 / 11 / 3 / 0 / 1 paths with 1 .. 7 tries)        -> asserted >= 281
  set 2, rays that hit / miss at segment 0:  g11 295 / 217, kitchen_sink 120 / 392        -> asserted >= 96 / 173
  (all four far rays hit in both worlds, at t = 1.00e4 .. 1.12e4)
"""
import ctypes as C

import numpy as np
import pytest

from paths_common import camera_path, camera_paths, compare_records, expected_records, first_ids
from scenes_common import REGIME_WORLDS, _unit, kitchen_sink

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SEED = 48, 32, 7
WORLDS = ["g11", "g50x", "kitchen_sink"]
FAR_TMAX = 2.0e4
MIN_HIT, MIN_MISS, MIN_EXHAUSTED, MIN_RETRIED = 0.591, 0.121, 0.182, 281
MIN_SURFACE_HIT, MIN_SURFACE_MISS = 96, 173


class _Cache:
    """Worlds, ray sets and oracle answers, each built once per module and never changed."""

    def __init__(self, om, O):
        self.om, self.O, self.d = om, O, {}

    def world(self, name):
        if name not in self.d:
            om, O = self.om, self.O
            if name == "kitchen_sink":
                w, ow, cam, ocam = kitchen_sink(om, O)
            else:
                wb, cb = REGIME_WORLDS[name]
                w, ow = wb(om, O)
                cam, ocam = cb(om, O, W / H)
            rays, states, tries = camera_paths(O, ocam, W, H, SEED)
            self.d[name] = dict(w=w, ow=ow, cam=cam, ocam=ocam, rays=rays, states=states, tries=tries,
                                ids=first_ids(ow, rays), exp={})
        return self.d[name]

    def expected(self, name, depth=50):
        """(the expected records of set 1, the oracle's segment count) at max_depth `depth`"""
        d = self.world(name)
        if depth not in d["exp"]:
            stats, ctr = self.O.render(d["ow"], d["ocam"], self.O.params(W, H, 1, seed=SEED, max_depth=depth))
            d["exp"][depth] = (expected_records(self.om, self.O, stats, d["ids"]), int(ctr["segments"]))
        return d["exp"][depth]

    def surface(self, name):
        """Set 2: rays, states and expected records."""
        d = self.world(name)
        if "surface" not in d:
            om, O, ow = self.om, self.O, d["ow"]
            rng = np.random.default_rng(20261021)
            pts = []
            for r in d["rays"]:
                h = ow.hit(r[:3], r[3:])
                if h is not None:
                    pts.append(h[0][1:4])
            pts = np.array(pts, dtype=F)
            pts = pts[rng.permutation(len(pts))[:512]]
            assert len(pts) == 512
            dirs = _unit(rng.standard_normal((4 * len(pts), 3)))
            dirs = dirs[np.abs(dirs[:, 1]) < 0.99][:len(pts)]
            cams = [(tuple(map(float, p)), tuple(map(float, p + q)), 40.0, 1000 + k) for k, (p, q) in enumerate(zip(pts, dirs))]
            d["surface"] = self._own_cameras(ow, cams, 100.0)
        return d["surface"]

    def far(self, name):
        """Four finite origins about 1e4 from the world, looking at it, with a window that reaches it."""
        d = self.world(name)
        if "far" not in d:
            cams = [(o, (0.3 * k, 0.4, -0.5), 0.02, 2000 + k)
                    for k, o in enumerate([(1e4, 2e3, 3e3), (-9e3, 4e3, -2e3), (3e3, 1e4, 1e3), (-2e3, 5e2, 1.1e4)])]
            d["far"] = self._own_cameras(d["ow"], cams, FAR_TMAX)
        return d["far"]

    def _own_cameras(self, ow, cams, tmax):
        """Pixel 0 of a 2x2 frame of an aperture-0 camera per ray -> rays, states, expected records."""
        om, O = self.om, self.O
        rays, states, exp_stats = [], [], []
        for lookfrom, lookat, vfov, seed in cams:
            oc = O.camera(lookfrom, lookat, (0., 1., 0.), vfov, 1.0, 0.0, 1.0)
            ray, st, _ = camera_path(O, oc, 2, 2, seed, 0, O.jitter_table(seed, 1))
            rays.append(ray)
            states.append(st)
            exp_stats.append(O.render_pixels(ow, oc, O.params(2, 2, 1, seed=seed, tmax=tmax), [0])[0])
        rays = np.ascontiguousarray(np.stack(rays).astype(F))
        stats = np.array(exp_stats, dtype=O.PIXEL_STATS_DTYPE)
        return rays, np.array(states, dtype=np.uint64), expected_records(om, O, stats, first_ids(ow, rays, tmax=tmax))


@pytest.fixture(scope="module")
def cache(om, oracle):
    return _Cache(om, oracle)


def _run(d, rays, states, kernel="auto", **kw):
    fz = d["w"].freeze(kernel=kernel)
    try:
        return fz.ray_color(rays, rng=states, **kw)
    finally:
        fz.close()


# ------------------------------------------------------------------ 1. camera rays
@pytest.mark.parametrize("name", WORLDS)
def test_witness(cache, name):
    """The expected set itself, from the oracle's data alone: it holds misses, hits, exhausted paths
    and streams that needed more than one lens-disc try."""
    d = cache.world(name)
    exp, _ = cache.expected(name)
    n = len(exp)
    hit = exp["obj"] != 0
    print(f"{name}: hit share {hit.mean():.3f}, miss share {(~hit).mean():.3f}, retried {(d['tries'] >= 2).sum()}")
    assert hit.mean() >= MIN_HIT and (~hit).mean() >= MIN_MISS
    assert np.isinf(exp["depth"][~hit]).all() and np.isfinite(exp["depth"][hit]).all()
    assert (d["tries"] >= 2).sum() >= MIN_RETRIED
    e2, _ = cache.expected(name, 2)
    exhausted = (e2["color"] == 0).all(axis=1) & np.isfinite(e2["depth"])
    print(f"{name}: depth 2 exhausted share {exhausted.mean():.3f}")
    assert exhausted.sum() >= MIN_EXHAUSTED * n


@pytest.mark.parametrize("name,kernel", [(w, "auto") for w in WORLDS] + [("g11", k) for k in ("brute", "bvh", "sbvh", "bvh4", "bvh2w")])
def test_camera_rays(cache, name, kernel):
    d = cache.world(name)
    exp, _ = cache.expected(name)
    compare_records(_run(d, d["rays"], d["states"], kernel), exp, f"{name}/{kernel}")


@pytest.mark.parametrize("depth", [0, 1, 2])
def test_depth_cap(cache, depth):
    d = cache.world("g11")
    exp, _ = cache.expected("g11", depth)
    got = _run(d, d["rays"], d["states"], max_depth=depth)
    compare_records(got, exp, f"g11/depth {depth}")
    done = exp["obj"] != 0 if depth < 2 else (exp["color"] == 0).all(axis=1) & np.isfinite(exp["depth"])
    assert np.signbit(got["color"][done]).all()                    # -Color::ZERO on an exhausted depth


# ------------------------------------------------------------------ 2. rays no camera of the frame makes
@pytest.mark.parametrize("name", ["g11", "kitchen_sink"])
def test_surface_and_far_rays(cache, name):
    d = cache.world(name)
    rays, states, exp = cache.surface(name)
    assert (exp["obj"] != 0).sum() >= MIN_SURFACE_HIT and (exp["obj"] == 0).sum() >= MIN_SURFACE_MISS
    compare_records(_run(d, rays, states), exp, f"{name}/surface")
    rays, states, exp = cache.far(name)
    assert (np.abs(rays[:, :3]).max(axis=1) >= 9e3).all() and (exp["obj"] != 0).all()
    compare_records(_run(d, rays, states, tmax=FAR_TMAX), exp, f"{name}/far")


# ------------------------------------------------------------------ 3. implicit streams
@pytest.mark.parametrize("base", [0, 2 ** 32 - 3])
def test_implicit_streams(om, cache, base):
    d = cache.world("g11")
    rays = np.ascontiguousarray(d["rays"][::5])                   # 308 rays from all over the frame (its first rows are sky)
    fz = d["w"].freeze()
    try:
        states = np.array([om.path_rng_state(SEED, (base + i) % 2 ** 32, 3, 0) for i in range(len(rays))], dtype=np.uint64)
        a = fz.ray_color(rays, seed=SEED, stream_base=base, sample=3)
        b = fz.ray_color(rays, rng=states, seed=99, stream_base=5, sample=8)
        assert a.tobytes() == b.tobytes()
        c = fz.ray_color(rays, seed=SEED, stream_base=base, sample=4)
        hit = a["obj"] != 0
        assert hit.any() and np.array_equal(a["obj"], c["obj"]) and np.array_equal(a["depth"], c["depth"])
        assert (a["color"][hit] != c["color"][hit]).any()
    finally:
        fz.close()


# ------------------------------------------------------------------ 4. scheduling invariance
def _set(fz, what, value):
    from raytracingoneweekend_amd import _lib
    _lib.check(getattr(_lib.lib, what)(fz.ctx, value), fz.ctx)


@pytest.mark.parametrize("name", ["g11", "kitchen_sink"])
def test_scheduling_invariance(om, cache, name):
    import torch
    d = cache.world(name)
    exp, _ = cache.expected(name)
    n = 1573
    idx = np.arange(n) % len(d["rays"])
    rays, states, exp = np.ascontiguousarray(d["rays"][idx]), np.ascontiguousarray(d["states"][idx]), exp[idx]
    fz = d["w"].freeze()
    try:
        base = fz.ray_color(rays, rng=states)
        compare_records(base, exp, f"{name}/base")
        for m in (1, 63, 64, 65, 513):
            assert fz.ray_color(rays[:m], rng=states[:m]).tobytes() == base[:m].tobytes(), m
        fz.set_path_batch(6)                                        # 25 batches of 64 paths, the last one partial
        assert fz.ray_color(rays, rng=states).tobytes() == base.tobytes()
        fz.set_path_batch(0)
        for t in (1, 3, 100):
            _set(fz, "om_set_tail_bounce", t)
            assert fz.ray_color(rays, rng=states).tobytes() == base.tobytes(), t
        _set(fz, "om_set_tail_bounce", 0)
        _set(fz, "om_set_counting", 0)
        assert fz.ray_color(rays, rng=states).tobytes() == base.tobytes()
        _set(fz, "om_set_counting", 1)
        fz.set_pipeline("megakernel")                               # the query runs the wavefront whatever this says
        assert fz.ray_color(rays, rng=states).tobytes() == base.tobytes()
        fz.set_pipeline("auto")
        # device buffers 4 bytes off a 16-byte boundary
        dev = torch.device("cuda", 0)
        rbuf = torch.zeros(n * 6 + 1, dtype=torch.float32, device=dev)
        obuf = torch.zeros(n * 5 + 2, dtype=torch.float32, device=dev)
        rt = rbuf[1:].view(n, 6)
        rt.copy_(torch.from_numpy(rays).to(dev))
        st = torch.from_numpy(states.view(np.int64)).to(dev)
        ot = obuf[1:1 + n * 5].view(n, 5)
        assert rt.data_ptr() % 16 == 4 and ot.data_ptr() % 16 == 4
        fz.ray_color(rt, rng=st, out=ot)
        torch.cuda.synchronize()
        assert ot.cpu().numpy().tobytes() == base.tobytes()
        assert obuf[0].item() == 0.0 and obuf[-1].item() == 0.0    # nothing outside the n records
    finally:
        fz.close()


# ------------------------------------------------------------------ 5. neighbours undisturbed
def test_neighbours_undisturbed(om, oracle, cache):
    from raytracingoneweekend_amd import _lib
    d = cache.world("g11")
    exp, segments = cache.expected("g11")
    fz = d["w"].freeze()
    try:
        pix = om.PixelsBox.new(W * H)
        h0 = fz.hit_rays(d["rays"])
        om.render(d["cam"], fz, 50, 0.001, 100.0, 4, W, H, pix, seed=SEED, adaptive=False, sample_count=2)
        word = _lib.lib.om_progress(fz.ctx)
        _lib.check(_lib.lib.om_reset_counters(fz.ctx, None), fz.ctx)
        before = int(word[0])
        compare_records(fz.ray_color(d["rays"], rng=d["states"]), exp, "g11/between renders")
        ctr = fz.counters()
        assert ctr["segments"] == segments and ctr["samples"] == 0 and ctr["credited"] == 0
        assert ctr["prim_tests"] > 0 and int(word[0]) == before
        om.render(d["cam"], fz, 50, 0.001, 100.0, 4, W, H, pix, seed=SEED, adaptive=False, sample_count=2)
        ref, _ = oracle.render(d["ow"], d["ocam"], oracle.params(W, H, 4, seed=SEED))
        assert pix.pixels.tobytes() == ref.tobytes()
        assert fz.hit_rays(d["rays"]).tobytes() == h0.tobytes()
    finally:
        fz.close()


# ------------------------------------------------------------------ 6. non-finite rays
@pytest.mark.parametrize("name", ["g11", "kitchen_sink"])
def test_non_finite_rays_leave_the_others_alone(cache, name):
    """A ray with a NaN or infinite component is not traced: its record is (NaN colour, depth +inf, obj 0),
    it counts no segment, and the other records are those of the run without it."""
    d = cache.world(name)
    rays, states = d["rays"][:256].copy(), d["states"][:256]
    good = _run(d, rays, states)
    bad = [(3, 0, np.nan), (40, 1, np.inf), (63, 2, -np.inf), (64, 3, np.nan), (100, 4, np.inf), (129, 5, -np.inf),
           (200, 0, np.inf), (255, 5, np.nan)]
    for i, c, v in bad:
        rays[i, c] = v
    got = _run(d, rays, states)                                     # OM_OK: a failure raises
    keep = np.ones(256, dtype=bool)
    keep[[i for i, _, _ in bad]] = False
    assert got[keep].tobytes() == good[keep].tobytes()
    assert np.isnan(got["color"][~keep]).all() and np.isposinf(got["depth"][~keep]).all() and (got["obj"][~keep] == 0).all()
