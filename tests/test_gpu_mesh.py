"""Triangle meshes in the SBVH / BVH2 / BVH4 leaves against the CPU oracle: ray
queries record for record, occlusion, mesh cracks and duplicate-triangle ties, zero-thickness boxes
under axis rays, renders pixel for pixel, and the O(log n) work count.

Worlds: tests/mesh_common.py (numpy float32 geometry, the same arrays to add_triangles and, face by
face in the same order, to the oracle); tests/test_mesh_regimes.py pins the regime of each.

Ray sets (a), (b), (c) are those of tests/test_gpu_query.py (its ray_sets, 48x32), the camera aimed
at the mesh.  Witnesses measured with the oracle alone on the CPU, seed RAY_SEED:
  ico2    distinct triangles that are the answer of some ray: 285 of 320       (asserted: >= 160)
  ico2x2  the same rays: 285 distinct triangles, every one of the later copy
  hf48    distinct triangles answered: 943 of 4608                              (asserted: >= 200)
  cracks  of the 642 vertex / edge-midpoint rays at ico2, 119 pass through the near surface (39 of
          the 162 vertex rays); the others miss the edge by a float32 rounding and hit a triangle
  flat    of the 320 straight-down rays at hf48's flat region 159 hit a flat triangle (the others
          meet a shared vertex or edge and go on to the ground); the 640 in-plane rays get 118
          different answers
  ico3    set (a) is answered by 265 distinct triangles of 1280
"""
import numpy as np
import pytest

import mesh_common as MC
from scenes_common import compare_stats
from test_gpu_query import RAY_SEED, compare_hits, oracle_hits, ray_sets

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SPP, DEPTH, SEED = 48, 32, 8, 8, 5
KERNELS = ["brute", "culled", "bvh", "sbvh", "bvh2", "bvh4"]
WORLDS = ["ico2", "ico2x2", "hf48"]
WINDOW = (0.001, 0.5)
# camera (lookfrom, lookat, vfov) and the box set (c)'s origins are drawn from
VIEW = {"ico2": ((3.2, 2.0, 4.0), (0., 1., 0.), 35.), "ico2x2": ((3.2, 2.0, 4.0), (0., 1., 0.), 35.),
        "hf48": ((0.5, 6.0, 7.0), (0., 0., 0.), 40.)}
BOUNDS = {"ico2": ((-1.6, -0.3, -1.6), (1.6, 2.3, 1.6)), "ico2x2": ((-1.6, -0.3, -1.6), (1.6, 2.3, 1.6)),
          "hf48": ((-3.2, -0.3, -3.2), (3.2, 1.0, 3.2))}


def _unit(d):
    d = np.asarray(d, dtype=F)
    n = np.sqrt((d * d).sum(axis=1, dtype=F), dtype=F)
    return (d / n[:, None]).astype(F)


def _cameras(om, O, name):
    frm, at, fov = VIEW[name]
    return (om.Camera.new(frm, at, (0., 1., 0.), fov, W / H, 0.05, float(np.linalg.norm(np.subtract(frm, at)))),
            O.camera(frm, at, (0., 1., 0.), fov, W / H, 0.05, float(np.linalg.norm(np.subtract(frm, at)))))


class _Cache:
    """Worlds, ray sets and oracle answers, each built once per module and never changed."""

    def __init__(self, om, oracle):
        self.om, self.O, self.d, self.frames = om, oracle, {}, {}

    def world(self, name):
        key = ("world", name)
        if key not in self.d:
            items = MC.spec(self.om, name)
            self.d[key] = (items,) + MC.build(self.om, self.O, items)
        return self.d[key]

    def rays(self, name):
        """-> rays of sets (a) + (b) + (c), the oracle's records for the call window and for WINDOW"""
        key = ("rays", name)
        if key not in self.d:
            _, _, ow = self.world(name)
            cam, _ = _cameras(self.om, self.O, name)
            rays, exp = ray_sets(self.om, ow, cam, *BOUNDS[name])
            self.d[key] = (rays, exp, oracle_hits(self.om, ow, rays, *WINDOW))
        return self.d[key]

    def frame(self, name, adaptive=False):
        key = (name, adaptive)
        if key not in self.frames:
            _, _, ow = self.world(name)
            _, ocam = _cameras(self.om, self.O, name)
            p = self.O.params(W, H, SPP, max_depth=DEPTH, seed=SEED, adaptive=adaptive)
            self.frames[key] = self.O.render(ow, ocam, p)[0]
        return self.frames[key]

    def render(self, name, kernel, pipeline, adaptive=False, setup=None):
        from raytracingoneweekend_amd import _lib as L
        _, w, _ = self.world(name)
        cam, _ = _cameras(self.om, self.O, name)
        fz = w.freeze(cam, kernel=kernel, pipeline=pipeline)
        try:
            if setup:
                setup(L, fz)
            pix = self.om.PixelsBox.new(W * H)
            self.om.render(cam, fz, DEPTH, 0.001, 100.0, SPP, W, H, pix, seed=SEED, adaptive=adaptive)
        finally:
            fz.close()
        return pix.pixels


@pytest.fixture(scope="module")
def cache(om, oracle):
    c = _Cache(om, oracle)
    yield c
    c.d.clear()
    c.frames.clear()


def _check_queries(om, w, kernel, rays, exp, exp_win, label):
    """hit_rays and occluded, with the call's window and with one [0.001, 0.5] window per ray."""
    win = np.ascontiguousarray(np.tile(np.array(WINDOW, dtype=F), (len(rays), 1)))
    fz = w.freeze(kernel=kernel)
    try:
        compare_hits(fz.hit_rays(rays), exp, f"{label}/hit_rays")
        occ = fz.occluded(rays)
        assert np.array_equal(occ, exp["obj"] != 0), f"{label}/occluded: {int((occ != (exp['obj'] != 0)).sum())} rays differ"
        compare_hits(fz.hit_rays(rays, windows=win), exp_win, f"{label}/hit_rays windows")
        occ = fz.occluded(rays, windows=win)
        assert np.array_equal(occ, exp_win["obj"] != 0), f"{label}/occluded windows: {int((occ != (exp_win['obj'] != 0)).sum())} rays differ"
    finally:
        fz.close()


# ------------------------------------------------------------------ 1. queries, all six kernels
@pytest.mark.parametrize("name", WORLDS)
def test_ray_sets_reach_the_mesh(cache, name):
    """From the oracle alone: many different triangles are the answer of some ray."""
    items, _, _ = cache.world(name)
    rays, exp, exp_win = cache.rays(name)
    ids = set()
    for k in range(sum(1 for it in items if it[0] == "mesh")):
        ids |= set(MC.mesh_ids(items, k))
    tri = set(int(x) for x in exp["obj"]) & ids
    n_tri = len(MC.mesh_ids(items, -1))
    print(f"{name}: {len(rays)} rays, {len(tri)} distinct triangles of {len(ids)} answered; "
          f"{int((exp_win['obj'] != 0).sum())} rays hit within {WINDOW}")
    if name == "hf48":
        assert len(tri) >= 200
    else:
        assert len(tri) >= n_tri // 2, "at least half of the world's triangles"
    assert (exp["obj"] == 0).any() and (exp_win["obj"] != 0).any()
    if name == "ico2x2":                                         # every duplicate pair resolves to the later copy
        assert not set(int(x) for x in exp["obj"]) & set(MC.mesh_ids(items, 0))


@pytest.mark.parametrize("kernel", KERNELS + ["auto"])
@pytest.mark.parametrize("name", WORLDS)
def test_queries_equal_the_oracle(om, cache, name, kernel):
    _, w, _ = cache.world(name)
    rays, exp, exp_win = cache.rays(name)
    _check_queries(om, w, kernel, rays, exp, exp_win, f"{name}/{kernel}")


# ------------------------------------------------------------------ 2. cracks and ties
@pytest.fixture(scope="module")
def crack_rays():
    """From outside, at every vertex of ico2 and at every edge midpoint (float32): 162 + 480 rays."""
    v, f = MC.icosphere(2, (0., 1., 0.), 1.0)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64)
    e = np.unique(np.sort(e, axis=1), axis=0)
    mid = ((v[e[:, 0]] + v[e[:, 1]]) * F(0.5)).astype(F)
    targets = np.concatenate([v, mid]).astype(F)
    assert len(v) == 162 and len(e) == 480
    c = np.array([0., 1., 0.], dtype=F)
    org = (c + (targets - c) * F(3.0)).astype(F)
    return np.ascontiguousarray(np.concatenate([org, _unit(targets - org)], axis=1).astype(F))


@pytest.mark.parametrize("name", ["ico2", "ico2x2"])
def test_cracks_and_ties(om, cache, crack_rays, name):
    items, w, ow = cache.world(name)
    exp = oracle_hits(om, ow, crack_rays)
    exp_win = oracle_hits(om, ow, crack_rays, *WINDOW)
    # the near surface is 2 away (|origin - target|, a little less at an edge midpoint): a ray the
    # oracle answers from beyond 2.5 (the far side, the ground, another object, the sky) went through a crack
    through = int(((exp["t"] > 2.5) | (exp["obj"] == 0)).sum())
    print(f"{name}: {through} of {len(crack_rays)} vertex / edge rays pass the near surface")
    assert through >= 1, "no ray met a crack: check_inside's strict inequalities are not exercised"
    if name == "ico2x2":
        assert not set(int(x) for x in exp["obj"]) & set(MC.mesh_ids(items, 0)), "a hit reports the first copy"
        assert set(int(x) for x in exp["obj"]) & set(MC.mesh_ids(items, 1))
    for kernel in KERNELS:
        _check_queries(om, w, kernel, crack_rays, exp, exp_win, f"{name}/cracks/{kernel}")


# ------------------------------------------------------------------ 3. flat boxes and axis rays
@pytest.fixture(scope="module")
def flat_rays():
    """Rays at hf48's flat region (triangles lying exactly in y = 0: zero-thickness boxes, rounded
    outward to half precision in the L2 tree): straight down, with one zero direction component, and
    lying in the plane y = 0."""
    v, f = MC.heightfield48()
    flat = f[(v[f][:, :, 1] == 0).all(axis=1)]
    assert len(flat) >= 500, "the height function lost its flat region"
    rng = np.random.default_rng(RAY_SEED)
    pick = flat[rng.choice(len(flat), 160, replace=False)]
    cen = ((v[pick[:, 0]] + v[pick[:, 1]] + v[pick[:, 2]]) / F(3.0)).astype(F)      # inside a flat triangle
    vert = v[pick[:, 0]]                                                              # a shared vertex of flat triangles
    targets = np.concatenate([cen, vert]).astype(F)
    n = len(targets)
    down = np.concatenate([targets + np.array([0., 2., 0.], dtype=F), np.tile(np.array([0., -1., 0.], dtype=F), (n, 1))], axis=1)
    # one zero component: from above, in a plane x = const or z = const through the target
    off = np.zeros((n, 3), dtype=F)
    off[:, 1] = F(1.5)
    off[::2, 0] = F(1.0)
    off[1::2, 2] = F(-1.25)
    slant = np.concatenate([targets + off, _unit(-off)], axis=1)
    # in the plane y = 0: origins on the flat region and outside the field, d.y = 0 exactly
    ang = rng.random(n, dtype=F) * F(6.2831855)
    dirs = np.stack([np.cos(ang, dtype=F), np.zeros(n, dtype=F), np.sin(ang, dtype=F)], axis=1)
    dirs[:8] = np.array([[1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 0, -1]] * 2, dtype=F)   # and along the axes
    inplane = np.concatenate([targets, _unit(dirs)], axis=1)
    outside = inplane.copy()
    outside[:, :3] = (targets - _unit(dirs) * F(8.0)).astype(F)
    outside[:, 1] = F(0.0)
    rays = np.ascontiguousarray(np.concatenate([down, slant, inplane, outside]).astype(F))
    assert (rays[:n, 3] == 0).all() and (rays[:n, 5] == 0).all() and (rays[2 * n:, 4] == 0).all() and (rays[2 * n:, 1] == 0).all()
    return rays


@pytest.mark.parametrize("kernel", KERNELS)
def test_flat_boxes_and_axis_rays(om, cache, flat_rays, kernel):
    items, w, ow = cache.world("hf48")
    key = ("flat", "hf48")
    if key not in cache.d:
        cache.d[key] = (oracle_hits(om, ow, flat_rays), oracle_hits(om, ow, flat_rays, *WINDOW))
    exp, exp_win = cache.d[key]
    n = len(flat_rays) // 4
    tri = set(MC.mesh_ids(items))
    down_tri = sum(1 for x in exp["obj"][:n] if int(x) in tri)
    assert down_tri >= n // 4, "the straight-down rays do not reach the flat triangles"
    assert len(set(int(x) for x in exp["obj"][2 * n:])) >= 3, "the in-plane rays all give one answer"
    _check_queries(om, w, kernel, flat_rays, exp, exp_win, f"hf48/flat/{kernel}")


# ------------------------------------------------------------------ 4. renders
RENDERS = [("auto", "wavefront", False, None), ("auto", "megakernel", False, None)] + \
          [(k, "wavefront", False, None) for k in KERNELS] + \
          [("bvh2", "wavefront", False, 0), ("bvh2", "wavefront", False, 2), ("auto", "wavefront", True, None)]


@pytest.mark.parametrize("kernel,pipeline,adaptive,lists", RENDERS,
                         ids=[f"{k}-{p}{'-adaptive' if a else ''}{'' if l is None else f'-lists{l}'}" for k, p, a, l in RENDERS])
@pytest.mark.parametrize("name", WORLDS)
def test_renders_equal_the_oracle(cache, name, kernel, pipeline, adaptive, lists):
    setup = None if lists is None else (lambda L, fz: L.check(L.lib.om_set_primary_lists(fz.ctx, lists), fz.ctx))
    got = cache.render(name, kernel, pipeline, adaptive=adaptive, setup=setup)
    exp = cache.frame(name, adaptive)
    nb, msg = compare_stats(got, exp, f"{name}/{kernel}/{pipeline}/adaptive={adaptive}/lists={lists}")
    assert nb == 0, msg
    if not adaptive:
        assert (got["n"] == SPP).all()


@pytest.mark.parametrize("name", WORLDS)
def test_frames_show_the_mesh(cache, name):
    """From the oracle alone: many first hits of the frame are mesh triangles, and paths go deep
    (the dielectric copy of ico2x2 keeps them bouncing inside)."""
    items, _, ow = cache.world(name)
    _, ocam = _cameras(cache.om, cache.O, name)
    one = cache.O.render(ow, ocam, cache.O.params(W, H, 1, max_depth=DEPTH, seed=SEED))[0]
    blooms = {cache.O.bloom_hash(i) for k in range(sum(1 for it in items if it[0] == "mesh")) for i in MC.mesh_ids(items, k)}
    seen = len(set(one["bloom"].tolist()) & blooms)
    print(f"{name}: {seen} distinct mesh triangles are first hits of the 1-spp frame")
    assert seen >= 50


# ------------------------------------------------------------------ 5. O(log n), not O(n)
def test_a_mesh_ray_costs_far_fewer_box_tests_than_triangles(om, oracle, cache):
    """ico3 (1280 triangles), AUTO kernel, counting on, set (a): with the triangles in always2 every
    ray pays one box test per triangle (pre_tests / segments >= 1280); in the tree a few tens.  The
    bound n_tri / 2 = 640 separates the two with a wide margin on both sides."""
    from raytracingoneweekend_amd import _lib as L
    items = MC.spec(om, "ico3")
    w, ow = MC.build(om, oracle, items)
    assert w.counts()["triangles"] == 1280
    cam, _ = _cameras(om, oracle, "ico2")
    from test_gpu_query import pinhole_rays
    rays = np.ascontiguousarray(pinhole_rays(cam))
    exp = oracle_hits(om, ow, rays)
    fz = w.freeze()
    try:
        L.check(L.lib.om_set_counting(fz.ctx, 1), fz.ctx)
        L.check(L.lib.om_reset_counters(fz.ctx, None), fz.ctx)
        got = fz.hit_rays(rays)
        ctr = fz.counters()
    finally:
        fz.close()
    compare_hits(got, exp, "ico3/auto")
    assert len(set(int(x) for x in exp["obj"]) & set(MC.mesh_ids(items))) >= 100
    ratio = ctr["pre_tests"] / ctr["segments"]
    print(f"ico3: segments {ctr['segments']}, pre_tests {ctr['pre_tests']}, prim_tests {ctr['prim_tests']}: "
          f"{ratio:.1f} box tests and {ctr['prim_tests'] / ctr['segments']:.1f} exact tests per ray")
    assert ctr["segments"] == len(rays)
    assert ratio < 640
