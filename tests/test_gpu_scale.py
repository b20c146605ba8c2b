"""The tree culls against the exact tests across scale and distance, on the device.

Every other GPU test runs at one scale: coordinates within +-15, radii >= 0.2, ray origins inside the
world or 13 away.  Here the worlds and ray sets of tests/scale_common.py leave it: primitives of
1e-3, ray origins up to 1e5 away, worlds 3.6e4 and 1.4e5 from the origin (half-precision planes with
ulp 16, or beyond the half range), near-singular transforms, and the far sets again at g17, whose
BVH2 is read through L2 with half planes.  tests/test_scale_conservative.py shows on the CPU that
these sets hold rays whose float32 winner lies beyond its inflated box.

Every record of every kernel must equal the oracle's (all 32 bytes), every occlusion bit the
oracle's obj != 0, every frame the oracle's frame.  `brute` does everywhere.  The culling kernels do at
the scene scale, in the tiny and the sliver world (a sphere or ellipsoid whose margin cannot cover its
test's worst rounding from 16 away stays outside the trees and has no `culled` bound) and from
D = 1e4 on (a query ray beyond the slab test's reach, OM_SLAB_REACH, takes the reference loop).  They still differ at the sets of
scale_common.NOT_CONSERVATIVE, spheres of radius 0.14 .. 1 from 1e3 away (`culled`: from 1e2; measured before these
fixes, AUTO: cluster 9 of 2688 records at D = 1e2, 293 at 1e3; now 0 and 105).  The far renders all
equal the oracle's: a camera beyond the slab test's reach renders with the reference loop.  Those cases are strict expected failures with the failure pinned: every
differing record lost the oracle's winner, a bounded sphere, to a cull, and shows a farther hit or none;
anything else fails outright.
"""
import numpy as np
import pytest

import scale_common as SC
from scenes_common import compare_stats
from test_gpu_query import compare_hits

pytestmark = pytest.mark.gpu

F = np.float32
KERNELS = ["brute", "culled", "bvh", "sbvh", "bvh2", "bvh4", "bvh2w", "auto"]
ALL = SC.WORLDS + [SC.L2_WORLD]
W, H, SPP, DEPTH, SEED = 32, 20, 2, 8, 9
MW, MH = 16, 12


class _Cache:
    """worlds, ray sets, oracle answers and oracle frames: built once per module and never changed"""

    def __init__(self, om, O):
        self.om, self.O, self.d, self.frames, self.fz = om, O, {}, {}, None

    def world(self, name):
        if name not in self.d:
            items, w, ow = SC.world(self.om, self.O, name) if name != "marched" else \
                ((SC.spec(self.om, "marched"),) + SC.build(self.om, self.O, SC.spec(self.om, "marched")))
            sets = SC.ray_sets(self.om, self.O, name, items) if name != "marched" else {}
            self.d[name] = (items, w, ow, sets)
        return self.d[name]

    def answers(self, name, D, win):
        _, _, ow, sets = self.world(name)
        return SC.oracle_answers(self.om, self.O, name, D, ow, sets[D][0], *win)


@pytest.fixture(scope="module")
def cache(om, oracle):
    c = _Cache(om, oracle)
    yield c
    if c.fz is not None:
        c.fz[1].close()
    c.d.clear()
    c.frames.clear()


def _frozen(cache, name, kernel):
    """the world frozen under `kernel`; one at a time stays open (the cases of a world and kernel follow each other)"""
    if cache.fz is None or cache.fz[0] != (name, kernel):
        if cache.fz is not None:
            cache.fz[1].close()
        cache.fz = ((name, kernel), cache.world(name)[1].freeze(kernel=kernel))
    return cache.fz[1]


# ------------------------------------------------------------------ closest-hit and any-hit queries
# `brute` is the reference loop itself and passes everywhere; every other kernel culls, and fails
# at exactly the sets where tests/test_scale_conservative.py finds winners past their boxes
# (`culled` pre-tests spheres only: in the sphere-free world it is the reference loop too)
QUERY_CASES = [pytest.param(n, k, D, id=f"{n}-{k}-{D:g}",
                            marks=SC.xfail_known(k != "brute" and (n, D) in (SC.NOT_CONSERVATIVE_CULLED if k == "culled" else SC.NOT_CONSERVATIVE)))
               for n in ALL for k in KERNELS for D in SC.sets_of(n)]


@pytest.mark.parametrize("name,kernel,D", QUERY_CASES)
def test_queries_equal_the_oracle(cache, name, kernel, D):
    """hit_rays (all 32 bytes of every record) and occluded, in both windows of the set."""
    items, _, _, sets = cache.world(name)
    fz = _frozen(cache, name, kernel)
    rays = sets[D][0]
    prims = SC.prims(items)
    kinds = np.array([p.kind for p in prims] + ["marched"])
    skippable = np.array([p.kind == "sphere" and p.in_tree for p in prims] + [False])   # what a cull is known to skip
    bad = []
    for win in (SC.windows(name, D) if D else SC.windows(name, 13.0)[:1]):
        exp = cache.answers(name, D, win)
        got = fz.hit_rays(rays, *win)
        diff = (got.view(np.uint8).reshape(-1, 32) != exp.view(np.uint8).reshape(-1, 32)).any(axis=1)
        occ = fz.occluded(rays, *win)
        odiff = int((occ != (exp["obj"] != 0)).sum())
        lost = exp["obj"][diff & (exp["obj"] != 0)].astype(np.int64) - 1
        by_kind = {k: int((kinds[np.minimum(lost, len(kinds) - 1)] == k).sum()) for k in ("sphere", "cube", "tri", "para")}
        print(f"{name}/{kernel} D={D:g} window={win}: {int(diff.sum())} of {len(rays)} records differ "
              f"(the oracle's winner there: {by_kind}, none: {int((diff & (exp['obj'] == 0)).sum())}), {odiff} occlusion bits")
        if diff.any() or odiff:
            bad.append((win, int(diff.sum()), odiff))
            # the one known failure: the oracle's winner, a bounded sphere, was skipped; the device shows a
            # farther hit or none, and an occlusion bit can only be lost.  Anything else is a plain failure.
            assert (exp["obj"][diff] != 0).all() and skippable[np.minimum(lost, len(kinds) - 1)].all(), \
                f"{name}/{kernel} D={D:g} window={win}: a record differs where no cull is known to skip the winner"
            assert (got["t"][diff] >= exp["t"][diff]).all(), f"{name}/{kernel} D={D:g} window={win}: a nearer hit than the oracle's"
            assert not (occ & (exp["obj"] == 0)).any(), f"{name}/{kernel} D={D:g} window={win}: occluded where the oracle has no hit"
    if bad:
        raise SC.KnownDisagreement(f"{name}/{kernel} D={D:g}: (window, records, occlusion bits) {bad}")


WINDOW_CASES = [pytest.param(n, known, id=f"{n}-{'known' if known else 'control'}", marks=SC.xfail_known(known))
                for n in ALL for known in (False, True)
                if any(((n, D) in SC.NOT_CONSERVATIVE) == known for D in SC.WORLD_DISTANCES[n])]


@pytest.mark.parametrize("name,known", WINDOW_CASES)
def test_one_window_per_ray(cache, name, known):
    """The far sets of a world in one call, every ray with the second window of its own set
    ([0.001, 2 D]; the tiny world: the default window), closest hit and any hit, AUTO kernel: once
    the sets of scale_common.NOT_CONSERVATIVE (expected to fail), once the others."""
    _, w, _, sets = cache.world(name)
    rays, wins, exps = [], [], []
    for D in SC.WORLD_DISTANCES[name]:
        if ((name, D) in SC.NOT_CONSERVATIVE) != known:
            continue
        win = SC.windows(name, D)[-1]
        rays.append(sets[D][0])
        wins.append(np.tile(np.array(win, dtype=F), (len(sets[D][0]), 1)))
        exps.append(cache.answers(name, D, win))
    rays, wins, exp = (np.ascontiguousarray(np.concatenate(x)) for x in (rays, wins, exps))
    fz = _frozen(cache, name, "auto")
    got = fz.hit_rays(rays, windows=wins)
    occ = fz.occluded(rays, windows=wins)
    if not known:
        compare_hits(got, exp, f"{name}/windows per ray")
        assert np.array_equal(occ, exp["obj"] != 0), f"{name}: {int((occ != (exp['obj'] != 0)).sum())} occlusion bits differ"
        return
    diff = (got.view(np.uint8).reshape(-1, 32) != exp.view(np.uint8).reshape(-1, 32)).any(axis=1)
    odiff = occ != (exp["obj"] != 0)
    assert (exp["obj"][diff] != 0).all() and (got["t"][diff] >= exp["t"][diff]).all() and not (occ & (exp["obj"] == 0)).any(), \
        f"{name}: a difference other than a lost winner"
    if diff.any() or odiff.any():
        raise SC.KnownDisagreement(f"{name}/windows per ray: {int(diff.sum())} records, {int(odiff.sum())} occlusion bits differ")


def test_far_answers_go_both_ways(cache):
    """From the oracle alone: hits, misses and at least 3 distinct objects in each window of each world."""
    for name in ALL:
        for k in range(len(SC.windows(name, 13.0))):
            ids = set()
            for D in SC.WORLD_DISTANCES[name]:
                ids |= set(int(x) for x in cache.answers(name, D, SC.windows(name, D)[k])["obj"])
            assert 0 in ids and len(ids - {0}) >= 3, (name, k, len(ids))


# ------------------------------------------------------------------ renders from a far camera
# (pipeline, adaptive, primary lists, tail bounce)
CONFIGS = [("wavefront", False, None, None), ("megakernel", False, None, None), ("wavefront", False, 0, None),
           ("wavefront", False, 2, None), ("wavefront", True, None, None), ("wavefront", False, None, 1),
           ("wavefront", False, None, 0)]
VIEWS = [("cluster", 1e2), ("cluster", 1e3), ("cluster", 1e4), ("tiny", 0.0)]
# No far frame is a known failure: at D = 1e2 and 1e3 the frames are the oracle's (the flattened ellipsoids
# are outside the trees; the query sets at 1e3, aimed at the silhouettes, still find spheres to lose), and
# from D = 1e4, beyond the slab test's reach, om_render runs the call with the reference loop.
RENDER_KNOWN = lambda name, D, lists: False


def _view(cache, name, D, w=W, h=H):
    """-> cameras, tmax: a far camera with tmax = 4 D; D = 0: the default camera and window"""
    items = cache.world(name)[0]
    if D == 0.0:
        return cache.om.default_camera(w / h), cache.O.default_camera(w / h), 100.0
    cam, ocam = SC.far_camera(cache.om, cache.O, items, D, aspect=w / h, aperture=0.05)
    return cam, ocam, 4.0 * D


def _frame(cache, name, D, adaptive, w=W, h=H, tmax=None, steps=1024):
    key = (name, D, adaptive)
    if key not in cache.frames:
        _, ocam, t = _view(cache, name, D, w, h)
        p = cache.O.params(w, h, SPP, max_depth=DEPTH, tmin=0.001, tmax=tmax or t, march_steps=steps, seed=SEED, adaptive=adaptive)
        cache.frames[key] = cache.O.render(cache.world(name)[2], ocam, p)[0]
    return cache.frames[key]


def _render(cache, name, D, pipeline, adaptive, lists, tail, w=W, h=H, tmax=None, steps=1024):
    from raytracingoneweekend_amd import _lib as L
    cam, _, t = _view(cache, name, D, w, h)
    fz = cache.world(name)[1].freeze(cam, pipeline=pipeline)
    try:
        if lists is not None:
            L.check(L.lib.om_set_primary_lists(fz.ctx, lists), fz.ctx)
        if tail is not None:
            L.check(L.lib.om_set_tail_bounce(fz.ctx, tail), fz.ctx)
        pix = cache.om.PixelsBox.new(w * h)
        cache.om.render(cam, fz, DEPTH, 0.001, tmax or t, SPP, w, h, pix, seed=SEED, adaptive=adaptive, march_steps=steps)
    finally:
        fz.close()
    return pix.pixels


def _cfg_id(p, a, l, t):
    return f"{p}{'-adaptive' if a else ''}{'' if l is None else f'-lists{l}'}{'' if t is None else f'-tail{t}'}"


RENDER_CASES = [pytest.param(n, D, *c, id=f"{n}-{D:g}-{_cfg_id(*c)}", marks=SC.xfail_known(RENDER_KNOWN(n, D, c[2])))
                for n, D in VIEWS for c in CONFIGS]


@pytest.mark.parametrize("name,D,pipeline,adaptive,lists,tail", RENDER_CASES)
def test_far_renders_equal_the_oracle(cache, name, D, pipeline, adaptive, lists, tail):
    got = _render(cache, name, D, pipeline, adaptive, lists, tail)
    exp = _frame(cache, name, D, adaptive)
    nb, msg = compare_stats(got, exp, f"{name} D={D:g}/{pipeline}/adaptive={adaptive}/lists={lists}/tail={tail}")
    if nb and RENDER_KNOWN(name, D, lists):
        # the known failure is a frame of the right shape with other paths in it, nothing else
        assert got.dtype == exp.dtype and got.shape == exp.shape and int(got["n"].min()) >= 1, msg
        raise SC.KnownDisagreement(msg)
    assert nb == 0, msg


def test_far_frames_show_the_world(cache):
    """From the oracle alone: a far frame holds sky and paths that hit different objects of the cluster
    (measured: 11 %, 13 % and 86 % of the 640 pixels hit something at D = 1e2, 1e3, 1e4)."""
    for name, D in VIEWS[:3]:
        one = _frame(cache, name, D, False)
        seen = one["bloom"][one["bloom"] != 0]
        assert len(seen) >= 64 and len(set(seen.tolist())) >= 3 and (one["bloom"] == 0).any(), (name, D)


@pytest.mark.parametrize("pipeline", ["wavefront", "megakernel"])
def test_marched_from_afar(cache, pipeline):
    """The cluster plus a marched sphere, box and torus from 200 away (tmax 1000, 256 march steps):
    the wave-uniform march culls with every object far from the ray origin."""
    got = _render(cache, "marched", 200.0, pipeline, False, None, None, MW, MH, tmax=1000.0, steps=256)
    exp = _frame(cache, "marched", 200.0, False, MW, MH, tmax=1000.0, steps=256)
    nb, msg = compare_stats(got, exp, f"marched/{pipeline}")
    assert nb == 0, msg
