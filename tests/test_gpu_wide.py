"""The wide BVH2 (OM_KERNEL_BVH2W: 32-bit child codes, u32 lane stack) against the
CPU oracle, bit for bit.

1. Forced "bvh2w" on small worlds, which run it in milliseconds: the mesh worlds of
   tests/mesh_common.py (ico2; ico2x2, whose duplicate triangles tie; hf48; degen), S-traced (g11),
   the one-leaf tree g0 and ico2 beside a marched torus.  Closest hit, any hit, one [0.001, 0.5]
   window per ray, the edge windows of tests/test_gpu_occlusion.py (tmin < 0, NaN and inf bounds),
   non-finite rays, and wavefront renders with the primary lists off and on and one adaptive one.
   The ray sets are those of tests/test_gpu_mesh.py and tests/test_gpu_query.py.
2. The worlds of tests/wide_common.py past the 15-bit codes, under kernel "auto" (and "bvh4", which
   becomes the same variant): tree_info() says wide, queries and an 8x8 render window equal the
   oracle, the counters show that a tree was walked, and in W16P some winners are records above 65 535.

The oracle is brute force: 2.6 ms per ray at 104 k triangles, so the large worlds get 1024 and 512 rays.
"""
import numpy as np
import pytest

import mesh_common as MC
import wide_common as WC
from scenes_common import REGIME_WORLDS, compare_stats
from test_gpu_mesh import BOUNDS, DEPTH, H, SEED, SPP, VIEW, W, WINDOW, _cameras, _check_queries
from test_gpu_occlusion import class_windows, oracle_hits_windows
from test_gpu_query import RAY_SEED, _grid_bounds, compare_hits, oracle_hits, pinhole_rays, ray_sets

pytestmark = pytest.mark.gpu

F = np.float32
SMALL = ["ico2", "ico2x2", "hf48", "degen", "g11", "g0", "ico2+torus"]
MESH_VIEW = {"degen": "ico2", "ico2+torus": "ico2"}          # camera and bounds of another mesh world


def _unit(d):
    d = np.asarray(d, dtype=F)
    n = np.sqrt((d * d).sum(axis=1, dtype=F), dtype=F)
    return (d / n[:, None]).astype(F)


class _Small:
    """name -> (world, oracle world, camera, oracle camera, rays, oracle records for the call window and
    for WINDOW), built once per module and never changed."""

    def __init__(self, om, O):
        self.om, self.O, self.d, self.frames = om, O, {}, {}

    def get(self, name):
        if name not in self.d:
            om, O = self.om, self.O
            if name in ("g11", "g0"):
                wb, cb = REGIME_WORLDS[name]
                w, ow = wb(om, O)
                cam, ocam = cb(om, O, W / H)
                lo, hi = _grid_bounds("g11")
            else:
                w, ow = MC.build(om, O, MC.spec(om, name.split("+")[0]))
                if name == "ico2+torus":
                    tor = om.m4x4("TR", -1.9, 0.6, 1.3) ^ om.m4x4("RX", 0.5) ^ om.m4x4("SC", 1.0, 1.0, 1.0)
                    w += om.MarchedTorus.new(tor, (0.45, 0.12, 0.12), om.Material.new_metal((0.7, 0.7, 0.2)))
                    ow.add_marched_torus(tor.to_numpy(), (0.45, 0.12, 0.12), O.material("metal", (0.7, 0.7, 0.2)))
                view = MESH_VIEW.get(name, name)
                cam, ocam = _cameras(om, O, view)
                lo, hi = BOUNDS[view]
            rays, exp = ray_sets(om, ow, cam, lo, hi)
            self.d[name] = (w, ow, cam, ocam, rays, exp, oracle_hits(om, ow, rays, *WINDOW))
        return self.d[name]

    def frame(self, name, adaptive):
        if (name, adaptive) not in self.frames:
            _, ow, _, ocam = self.get(name)[:4]
            p = self.O.params(W, H, SPP, max_depth=DEPTH, seed=SEED, adaptive=adaptive)
            self.frames[(name, adaptive)] = self.O.render(ow, ocam, p)[0]
        return self.frames[(name, adaptive)]


@pytest.fixture(scope="module")
def small(om, oracle):
    s = _Small(om, oracle)
    yield s
    s.d.clear()
    s.frames.clear()


# ------------------------------------------------------------------ 1. forced bvh2w, small worlds
@pytest.mark.parametrize("name", SMALL)
def test_forced_wide_queries_equal_the_oracle(om, small, name):
    w, _, _, _, rays, exp, exp_win = small.get(name)
    fz = w.freeze(kernel="bvh2w")
    try:
        ti = fz.tree_info()
    finally:
        fz.close()
    assert ti["regime"] == "wide" and ti["lds_bytes"] >= 512 * 4 * ti["b2_depth"], ti
    assert (exp["obj"] != 0).any() and (exp["obj"] == 0).any()
    _check_queries(om, w, "bvh2w", rays, exp, exp_win, f"{name}/bvh2w")


@pytest.mark.parametrize("name,regime", [("ico2", "lds"), ("hf48", "l2"), ("g11", "lds"), ("g0", "lds")])
def test_host_plan_and_ctx_report_the_same_lds(small, name, regime):
    """om_world_tree_info restates the wavefront's LDS request on the host (om_world.h); under AUTO the
    ctx, which asks the wavefront itself (trace_lds), must report the same, in every regime (the wide
    one: test_w15p_auto_is_wide)."""
    w = small.get(name)[0]
    host = w.tree_info()
    fz = w.freeze()
    try:
        assert fz.tree_info() == host and host["regime"] == regime and host["lds_bytes"] > 0, (host, fz.tree_info())
    finally:
        fz.close()


def test_forced_wide_on_an_empty_tree_takes_the_fallbacks(om, oracle):
    """g0x (the ground only: no BVH2) under "bvh2w" answers like "bvh2" does there."""
    wb, cb = REGIME_WORLDS["g0x"]
    w, ow = wb(om, oracle)
    rays = np.ascontiguousarray(pinhole_rays(cb(om, oracle, W / H)[0])[::7])
    fz = w.freeze(kernel="bvh2w")
    try:
        assert fz.tree_info()["regime"] == "none"
        compare_hits(fz.hit_rays(rays), oracle_hits(om, ow, rays), "g0x/bvh2w")
    finally:
        fz.close()


@pytest.mark.parametrize("name", SMALL)
def test_forced_wide_edge_windows(om, small, name):
    """One window per ray from the eight classes of test_gpu_occlusion.class_windows: root == tmax,
    just below it, tmin just above the root, tmax = inf, tmin = -1, tmax = NaN, ..."""
    w, ow, _, _, rays, exp, _ = small.get(name)
    rays, exp = rays[::3], exp[::3]
    win = class_windows(om, exp)
    wexp = oracle_hits_windows(om, ow, rays, win)
    fz = w.freeze(kernel="bvh2w")
    try:
        occ = fz.occluded(rays, windows=win)
        assert np.array_equal(occ, wexp["obj"] != 0), f"{name}: {int((occ != (wexp['obj'] != 0)).sum())} rays differ"
        got = fz.hit_rays(rays, windows=win)
        assert np.array_equal(got["obj"], wexp["obj"])
        compare_hits(got, wexp, f"{name}/bvh2w edge windows", nan_payload=True)
    finally:
        fz.close()


@pytest.mark.parametrize("name", SMALL)
def test_forced_wide_non_finite_rays(om, small, name):
    """NaN and infinite ray components beside ordinary rays (test_gpu_query's edge set, on these worlds)."""
    w, ow, _, _, rays, _, _ = small.get(name)
    nan, inf = F("nan"), F("inf")
    odd = np.repeat(rays[[5, 700, 1400, 1600, 2200, len(rays) - 10]], 2, axis=0).copy()
    odd[0, 0] = nan; odd[1, 4] = nan; odd[2, 1] = inf; odd[3, 3] = -inf; odd[4, 5] = inf; odd[5, 2] = -inf
    odd[6, 0] = nan; odd[6, 4] = inf; odd[7, 3] = nan; odd[7, 5] = nan; odd[8, :3] = inf; odd[9, 4] = nan; odd[10, 2] = nan; odd[11, 3] = inf
    both = np.ascontiguousarray(np.concatenate([odd, rays[::97]]))
    fz = w.freeze(kernel="bvh2w")
    try:
        for tmin, tmax in [(0.001, 100.0), (0.0, float("inf")), (5.0, 1.0)]:
            exp = oracle_hits(om, ow, both, tmin, tmax)
            got = fz.hit_rays(both, tmin, tmax)
            assert np.array_equal(got["obj"], exp["obj"]), f"{name} [{tmin}, {tmax}]: obj differs"
            compare_hits(got, exp, f"{name}/bvh2w non-finite [{tmin}, {tmax}]", nan_payload=True)
            assert np.array_equal(fz.occluded(both, tmin, tmax), exp["obj"] != 0)
    finally:
        fz.close()


RENDERS = [(0, False), (2, False), (None, True)]


@pytest.mark.parametrize("lists,adaptive", RENDERS, ids=["lists0", "lists2", "adaptive"])
@pytest.mark.parametrize("name", SMALL)
def test_forced_wide_renders_equal_the_oracle(om, small, name, lists, adaptive):
    from raytracingoneweekend_amd import _lib as L
    w, _, cam, _ = small.get(name)[:4]
    fz = w.freeze(cam, kernel="bvh2w", pipeline="wavefront")
    try:
        if lists is not None:
            L.check(L.lib.om_set_primary_lists(fz.ctx, lists), fz.ctx)
        pix = om.PixelsBox.new(W * H)
        om.render(cam, fz, DEPTH, 0.001, 100.0, SPP, W, H, pix, seed=SEED, adaptive=adaptive)
    finally:
        fz.close()
    nb, msg = compare_stats(pix.pixels, small.frame(name, adaptive), f"{name}/bvh2w/lists={lists}/adaptive={adaptive}")
    assert nb == 0, msg
    if not adaptive:
        assert (pix.pixels["n"] == SPP).all()


# ------------------------------------------------------------------ 2. past the 15-bit codes
VIEW_W = ((0.5, 6.0, 7.0), (0., 1., 0.), 40.)                 # above the field, looking down at it
RW, RH = 64, 48


def _wide_cameras(om, O):
    frm, at, fov = VIEW_W
    dist = float(np.linalg.norm(np.subtract(frm, at)))
    return (om.Camera.new(frm, at, (0., 1., 0.), fov, RW / RH, 0.05, dist), O.camera(frm, at, (0., 1., 0.), fov, RW / RH, 0.05, dist))


def _wide_rays(om, ow, cam, n):
    """n rays: a third a pinhole subset, a third straight down or with one zero direction component
    at random points of the field, a third one bounce from the pinhole hit points; with the oracle's records."""
    rng = np.random.default_rng(RAY_SEED)
    k = n // 3
    allp = pinhole_rays(cam, RW, RH)
    a = allp[rng.choice(len(allp), k, replace=False)]
    xz = (rng.random((k, 2), dtype=F) * F(5.6) - F(2.8)).astype(F)
    org = np.stack([xz[:, 0], np.full(k, F(3.0)), xz[:, 1]], axis=1)
    d = np.tile(np.array([0., -1., 0.], dtype=F), (k, 1))
    d[1::3] = _unit(np.stack([np.zeros(len(d[1::3]), F), np.full(len(d[1::3]), F(-1.0)), rng.standard_normal(len(d[1::3])).astype(F)], axis=1))
    d[2::3] = _unit(np.stack([rng.standard_normal(len(d[2::3])).astype(F), np.full(len(d[2::3]), F(-1.0)), np.zeros(len(d[2::3]), F)], axis=1))
    b = np.concatenate([org, d], axis=1).astype(F)
    ea = oracle_hits(om, ow, a)
    on = np.nonzero(ea["obj"] != 0)[0]
    pick = on[np.arange(n - 2 * k) % len(on)]
    c = np.concatenate([ea["point"][pick], _unit(rng.standard_normal((len(pick), 3)))], axis=1).astype(F)
    rays = np.ascontiguousarray(np.concatenate([a, b, c]))
    return rays, np.concatenate([ea, oracle_hits(om, ow, b), oracle_hits(om, ow, c)])


@pytest.fixture(scope="module")
def w15p(om, oracle):
    items = WC.spec(om, "W15P")
    w, ow = MC.build(om, oracle, items)
    cam, ocam = _wide_cameras(om, oracle)
    rays, exp = _wide_rays(om, ow, cam, 1024)
    return items, w, ow, cam, ocam, rays, exp


def test_w15p_auto_is_wide(w15p):
    _, w, _, cam, _, _, _ = w15p
    host = w.tree_info()
    fz = w.freeze(cam)
    try:
        ti = fz.tree_info()
        assert ti == host, "the ctx under AUTO reports what the host-only plan does"
        assert ti["regime"] == "wide" and ti["b2_leaves"] >= 32768 and ti["records"] == 2 * WC.N["W15P"] ** 2 + 3   # (2 ellipsoids + cube: the small ellipsoid is a thin sphere, outside the trees)
        assert ti["lds_bytes"] == 512 * 4 * ti["b2_depth"], "the u32 lane stack alone (no node prefix, DESIGN.md §5.18)"
        fz.set_kernel("bvh")
        assert fz.tree_info()["regime"] == "none" and fz.tree_info()["lds_bytes"] == 0
    finally:
        fz.close()


@pytest.mark.parametrize("kernel", ["auto", "bvh4", "bvh2w"])
def test_w15p_queries_equal_the_oracle(om, w15p, kernel):
    """closest hit, any hit and windows; "bvh4" has no BVH4 here and runs the wide variant too"""
    items, w, ow, _, _, rays, exp = w15p
    tri = set(int(x) for x in exp["obj"]) & set(MC.mesh_ids(items))
    assert len(tri) >= 300 and (exp["obj"] == 0).any(), "the rays reach many triangles, and some miss"
    assert (rays[len(rays) // 3: 2 * (len(rays) // 3), 3:] == 0).any(axis=1).all(), "set two has a zero direction component"
    fz = w.freeze(kernel=kernel)
    try:
        assert fz.tree_info()["regime"] == "wide"
        compare_hits(fz.hit_rays(rays), exp, f"W15P/{kernel}/hit_rays")
        assert np.array_equal(fz.occluded(rays), exp["obj"] != 0)
        if kernel == "auto":
            win = np.ascontiguousarray(np.tile(np.array(WINDOW, dtype=F), (len(rays), 1)))
            exp_win = oracle_hits(om, ow, rays, *WINDOW)
            assert (exp_win["obj"] != 0).any()
            compare_hits(fz.hit_rays(rays, windows=win), exp_win, "W15P/auto/hit_rays windows")
            assert np.array_equal(fz.occluded(rays, windows=win), exp_win["obj"] != 0)
    finally:
        fz.close()


def test_w15p_a_tree_is_walked(om, w15p):
    """Counting on: pre_tests per ray below records / 100 (brute force or always2 would cost one
    test per record and ray).  A condition, not a tuning target."""
    from raytracingoneweekend_amd import _lib as L
    _, w, _, _, _, rays, exp = w15p
    fz = w.freeze()
    try:
        L.check(L.lib.om_set_counting(fz.ctx, 1), fz.ctx)
        L.check(L.lib.om_reset_counters(fz.ctx, None), fz.ctx)
        got = fz.hit_rays(rays)
        ctr = fz.counters()
        records = fz.tree_info()["records"]
    finally:
        fz.close()
    compare_hits(got, exp, "W15P/auto counting")
    per_ray = ctr["pre_tests"] / ctr["segments"]
    print(f"W15P: {records} records, {per_ray:.1f} box tests and {ctr['prim_tests'] / ctr['segments']:.1f} exact tests per ray")
    assert ctr["segments"] == len(rays) and 0 < per_ray < records / 100


def test_w15p_render_window_equals_the_oracle(om, oracle, w15p):
    """an 8x8 window of a 64x48 frame at 2 spp, depth 8 (the device renders the whole frame)"""
    _, w, ow, cam, ocam, _, _ = w15p
    pixels = oracle.window_pixels(RW, RH, 28, 22, 8)
    exp = oracle.render_pixels(ow, ocam, oracle.params(RW, RH, 2, max_depth=8, seed=SEED), pixels, nthreads=0)
    fz = w.freeze(cam, pipeline="wavefront")
    try:
        pix = om.PixelsBox.new(RW * RH)
        om.render(cam, fz, 8, 0.001, 100.0, 2, RW, RH, pix, seed=SEED, adaptive=False)
    finally:
        fz.close()
    got = pix.pixels[pixels]
    assert (exp["bloom"] != 0).any(), "the window sees the field"
    nb, msg = compare_stats(np.ascontiguousarray(got), exp, "W15P/auto/wavefront window")
    assert nb == 0, msg


def test_w16p_winners_above_65535(om, oracle):
    """More than 65 536 nodes and records: 512 rays, straight down over the whole field, so winners
    lie all over the record array; closest and any hit."""
    items = WC.spec(om, "W16P")
    w, ow = MC.build(om, oracle, items)
    rng = np.random.default_rng(RAY_SEED + 1)
    n = 512
    xz = (rng.random((n, 2), dtype=F) * F(5.8) - F(2.9)).astype(F)
    d = np.tile(np.array([0., -1., 0.], dtype=F), (n, 1))
    d[n // 2:] = _unit(np.stack([rng.standard_normal(n - n // 2).astype(F) * F(0.3), np.full(n - n // 2, F(-1.0)),
                                 rng.standard_normal(n - n // 2).astype(F) * F(0.3)], axis=1))
    rays = np.ascontiguousarray(np.concatenate([np.stack([xz[:, 0], np.full(n, F(3.0)), xz[:, 1]], axis=1), d], axis=1).astype(F))
    exp = oracle_hits(om, ow, rays)
    fz = w.freeze()
    try:
        ti = fz.tree_info()
        assert ti["regime"] == "wide" and ti["b2_nodes"] > 65536 and ti["records"] > 65536
        got = fz.hit_rays(rays)
        occ = fz.occluded(rays)
    finally:
        fz.close()
    compare_hits(got, exp, "W16P/auto/hit_rays")
    assert np.array_equal(occ, exp["obj"] != 0)
    # obj = gi + 1.  Winners with ids above 65 536 show that no 16-bit gi survives anywhere.  The
    # record index itself is not visible from here: the records are the primitives in leaf order,
    # which follows the tree's split of space, the field's triangles are numbered row by row, and
    # the rays fall uniformly over the field -- so winners spread over the whole id range (every
    # quarter of it is asserted) are spread over the whole record array, of which the first 65 536
    # records are 30 %.  tests/test_wide_regimes.py checks on the host that every record of this
    # world lies in exactly one leaf of the wide tree.
    ids = np.unique(got["obj"][got["obj"] != 0])
    n_tri = 2 * WC.N["W16P"] ** 2
    quarters = np.histogram(ids[ids > 5], bins=4, range=(5, 5 + n_tri))[0]
    print(f"W16P: {len(ids)} distinct winners, per quarter of the triangle ids {quarters.tolist()}")
    assert (ids > 65536 + 5).sum() >= 100 and len(ids) >= 400 and (quarters >= 50).all(), f"{len(ids)} distinct winners"
