"""The ray-ordered LDS nodes of the BVH2 (OM_B2_PLANES) against the CPU oracle, byte
for byte, and against the work the library counted before them.

stage_scene<TR_BVH2_LDS> keeps every (child, axis) plane pair of a staged node as [lo, hi, lo] and a
lane reads (near, far) at the dword its ray's sign picks; tests/test_ordered_planes.py shows on the
host that every visit then decides what it decided.  Here the device runs it, under kernel "bvh2":

* closest hit and any hit on g0 (one leaf and an empty second child, staged as all of space),
  S-traced (g11), g16 (the LDS budget's edge), c7x18 (the leaf table behind the nodes) and the ico2
  mesh (the TR_BARY forms), on ray sets made for the sign-picked read: 128 rays in each of the 8 sign
  octants, rays with one zero direction component (every axis, both signs of the zero) and with two
  (every axis direction, all four sign pairs of the zeros), all from random points inside the
  scene's boxes, and rays leaving the surfaces the octant rays hit;
* the counters of those calls: the box tests and exact tests the parent commit counted for the same
  rays (tests/golden/ordered_planes_counters.json, recorded from it) -- the ordered read visits the
  same nodes in the same order;
* 64x40x4 renders of S-traced at depth 50 and 2 through the wavefront, kernels "bvh2" and "auto",
  counting on and off, tail threshold 2 and default, the counters of tests/golden/fused_counters.json,
  and the same frame through the megakernel, whose own staging is untouched.  (The first launch
  stages and reads the plain node, the later launches and the tail the ordered one: depth 2 ends
  inside the first launch, depth 50 runs both, and both must meet in one frame.)

The oracle's answers are computed once per module and shared read-only.
"""
import json
import os

import numpy as np
import pytest

import mesh_common as MC
from scenes_common import REGIME_WORLDS, _unit, compare_stats, oracle_hits
from test_gpu_fused_bounce import GOLDEN as FUSED_GOLDEN, SEED, _Frames
from test_gpu_mesh import BOUNDS
from test_gpu_query import _grid_bounds, compare_hits

pytestmark = pytest.mark.gpu

F = np.float32
RAY_SEED = 20261021
WORLDS = ["g0", "g11", "g16", "c7x18", "ico2"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ordered_planes_counters.json")
COUNTED = ("segments", "pre_tests", "prim_tests")


def sign_rays(lo, hi, seed=RAY_SEED):
    """The octant, one-zero and two-zero sets of the module docstring: origins uniform in [lo, hi]."""
    rng = np.random.default_rng(seed)
    d = []
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                a = np.abs(rng.standard_normal((128, 3))).astype(F) + F(1e-3)
                d.append(_unit(a * np.array([sx, sy, sz], dtype=F)))
    for axis in range(3):
        for zero in (F(0.0), F(-0.0)):
            a = rng.standard_normal((64, 3)).astype(F)
            a[:, axis] = 0
            a = _unit(a)
            a[:, axis] = zero
            d.append(a)
    for axis in range(3):
        for s in (F(1.0), F(-1.0)):
            for za in (F(0.0), F(-0.0)):
                for zb in (F(0.0), F(-0.0)):
                    a = np.empty((16, 3), dtype=F)
                    a[:, axis], a[:, (axis + 1) % 3], a[:, (axis + 2) % 3] = s, za, zb
                    d.append(a)
    d = np.concatenate(d).astype(F)
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    o = (lo + rng.random((len(d), 3), dtype=F) * (hi - lo)).astype(F)
    return np.ascontiguousarray(np.concatenate([o, d], axis=1).astype(F))


def build_world(om, O, name):
    if name == "ico2":
        w, ow = MC.build(om, O, MC.spec(om, name))
        return w, ow, BOUNDS[name]
    w, ow = REGIME_WORLDS[name][0](om, O)
    return w, ow, _grid_bounds(name)


def ray_set(om, O, name):
    """-> world, rays (the sign sets + 256 rays leaving the points the octant rays hit), oracle records"""
    w, ow, (lo, hi) = build_world(om, O, name)
    a = sign_rays(lo, hi)
    ea = oracle_hits(om, ow, a)
    on = np.nonzero(ea["obj"][:1024] != 0)[0]
    pick = on[np.arange(256) % len(on)]
    rng = np.random.default_rng(RAY_SEED + 1)
    b = np.concatenate([ea["point"][pick], _unit(rng.standard_normal((256, 3)))], axis=1).astype(F)
    rays = np.ascontiguousarray(np.concatenate([a, b]))
    exp = np.concatenate([ea, oracle_hits(om, ow, b)])
    exp.setflags(write=False)
    return w, rays, exp


def counted_queries(w, rays, counting=1):
    """hit_rays and occluded under "bvh2" -> records, flags, the counters of each call"""
    from raytracingoneweekend_amd import _lib as L
    fz = w.freeze(kernel="bvh2")
    try:
        assert fz.tree_info()["regime"] == "lds"
        L.check(L.lib.om_set_counting(fz.ctx, counting), fz.ctx)
        L.check(L.lib.om_reset_counters(fz.ctx, None), fz.ctx)
        got = fz.hit_rays(rays)
        c_hit = fz.counters()
        L.check(L.lib.om_reset_counters(fz.ctx, None), fz.ctx)
        occ = fz.occluded(rays)
        c_occ = fz.counters()
    finally:
        fz.close()
    return got, occ, {k: int(c_hit[k]) for k in COUNTED}, {k: int(c_occ[k]) for k in COUNTED}


@pytest.fixture(scope="module")
def sets(om, oracle):
    d = {}

    def get(name):
        if name not in d:
            d[name] = ray_set(om, oracle, name)
        return d[name]
    yield get
    d.clear()


def test_ray_sets_cover_the_signs():
    r = sign_rays((-1., -1., -1.), (1., 1., 1.))
    d = r[:, 3:]
    assert len(r) == 1024 + 384 + 384
    octants = {tuple(np.signbit(x)) for x in d[:1024]}
    assert len(octants) == 8 and (d[:1024] != 0).all()
    one, two = d[1024:1408], d[1408:]
    assert ((one == 0).sum(axis=1) == 1).all() and ((two == 0).sum(axis=1) == 2).all()
    for part in (one, two):
        z = part == 0
        assert (z & np.signbit(part)).any(axis=0).all() and (z & ~np.signbit(part)).any(axis=0).all(), "both signs of zero on every axis"


@pytest.mark.parametrize("name", WORLDS)
def test_queries_equal_the_oracle_and_the_recorded_work(sets, name):
    w, rays, exp = sets(name)
    hit_share = float((exp["obj"] != 0).mean())
    print(f"{name}: {len(rays)} rays, hit share {hit_share:.3f}, {len(np.unique(exp['obj']))} distinct answers")
    assert 0.05 < hit_share < 1.0, "the set has hits and misses"
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    for counting in (1, 0):
        got, occ, c_hit, c_occ = counted_queries(w, rays, counting)
        compare_hits(got, exp, f"{name}/bvh2/count{counting}/hit_rays")
        assert np.array_equal(occ, exp["obj"] != 0), f"{name}/occluded: {int((occ != (exp['obj'] != 0)).sum())} rays differ"
        if counting:
            print("hit_rays", c_hit, "occluded", c_occ, "recorded", want)
            assert c_hit == want["hit_rays"] and c_occ == want["occluded"]
            assert c_hit["segments"] == len(rays) and c_hit["pre_tests"] > 0


@pytest.fixture(scope="module")
def frames(om, oracle):
    f = _Frames(om, oracle)
    yield f
    f.frames.clear()


@pytest.mark.parametrize("kernel", ["bvh2", "auto"])
@pytest.mark.parametrize("depth", [50, 2])
def test_renders_equal_the_oracle(frames, depth, kernel):
    W, H, SPP = 64, 40, 4
    for counting in (1, 0):
        for tail in (2, 0):
            got, _ = frames.check(f"depth{depth}/{kernel}/count{counting}/tail{tail}", "S-traced", W, H, SPP, depth=depth,
                                  kernel=kernel, counting=counting, tail=tail)
            assert (got["n"] == SPP).all()


def test_render_counters_are_the_recorded_ones(frames):
    W, H, SPP = 64, 40, 4
    _, ctr = frames.check("counters", "S-traced", W, H, SPP, counting=1)
    with open(FUSED_GOLDEN) as f:
        want = json.load(f)["S-traced 64x40 4spp seed 17 bvh2 wavefront"]
    print({k: ctr[k] for k in COUNTED}, "recorded", want)
    assert ctr["pre_tests"] == want["pre_tests"] and ctr["prim_tests"] == want["prim_tests"] and ctr["segments"] == want["segments"]


def test_megakernel_render_is_untouched(om, frames):
    W, H, SPP = 64, 40, 4
    exp, _ = frames.expected("S-traced", W, H, SPP)
    w, _ = frames.worlds("S-traced")
    cam, _ = frames.cameras(None, W / H)
    fz = w.freeze(cam, kernel="bvh2", pipeline="megakernel")
    try:
        pix = om.PixelsBox.new(W * H)
        om.render(cam, fz, 50, 0.001, 100.0, SPP, W, H, pix, seed=SEED, adaptive=False)
    finally:
        fz.close()
    nb, msg = compare_stats(pix.pixels, exp, "S-traced/bvh2/megakernel")
    assert nb == 0, msg
