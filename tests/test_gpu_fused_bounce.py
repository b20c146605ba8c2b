"""Bounce 1 inside the bounce-0 launch (k_bounce's FUSE, OM_WF_FUSE_B1) against
the oracle, all 40 bytes of every pixel.

The first launch of a traced batch traces and shades bounce 1 on the lanes whose path goes on, before
it compacts them into bounce 2's queue; the per-bounce launches then start at bounce 2 and the tail
one bounce later.  Every case renders through the wavefront with kernel BVH2 on S-traced (tree in
LDS) unless it says otherwise, with the counting kernels and with the plain ones.  The shapes are the
smallest at which each part can go wrong:

* max_depth 1 / 2 / 3 / 50: no second segment at all; every second segment ends in the -0 exhaustion;
  the first queue written is the last; the normal case;
* survivor extremes: a sky-only view (every wave skips the second segment, every count is zero) and
  a view of the ground from above (no lane ends at bounce 0);
* ragged frames: 70x37 (partial tiles take the per-lane candidate lists, the batch's last block is
  partial) and 1x7 (non-finite rays);
* primary lists off / auto / on (bounce 0 through the tree, like the fused second segment, or the lists);
* tail thresholds 1, 2, 3 and the default on 1 and 2 streams (a tail asked for at a bounce the fused
  launch has already run starts on the first queue there is);
* one adaptive call on 1 stream (serial) and 2 streams;
* the L2 tree (g17) under BVH2 and BVH4, and S-traced under BVH4;
* the work counters: segments as the oracle counts them, exact and box tests as the library counted
  them before the fused launch (tests/golden/fused_counters.json, recorded from the parent commit);
* the launch counts of one 16-spp batch: bounce0 1, bounce 15, tail 1.

Oracle frames are rendered once per module and shared read-only.
"""
import ctypes as C
import json
import os

import pytest

from scenes_common import REGIME_WORLDS, compare_stats

pytestmark = pytest.mark.gpu

SEED = 17
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_counters.json")
VIEWS = {
    # straight up from above the ground: sky only
    "sky": ((0., 5., 0.), (0., 50., 0.1), (0., 0., 1.), 20., 0., 10.),
    # down on the middle of the sphere field from above it: ground and spheres, no sky
    "ground": ((0., 12., 0.1), (0., 0., 0.), (0., 1., 0.), 30., 0., 10.),
}


class _Frames:
    """Oracle frames keyed by their arguments, each rendered once."""

    def __init__(self, om, oracle):
        self.om, self.oracle, self.frames = om, oracle, {}

    def worlds(self, name):
        if name == "S-traced":
            return self.om.random_scene(0x5EED), self.oracle.random_scene(0x5EED)
        return REGIME_WORLDS[name][0](self.om, self.oracle)

    def cameras(self, view, aspect):
        if view is None:
            return self.om.default_camera(aspect), self.oracle.default_camera(aspect)
        a = VIEWS[view]
        args = (a[0], a[1], a[2], a[3], aspect, a[4], a[5])
        return self.om.Camera.new(*args), self.oracle.camera(*args)

    def expected(self, name, W, H, spp, depth=50, adaptive=False, view=None):
        key = (name, W, H, spp, depth, adaptive, view)
        if key not in self.frames:
            _, ow = self.worlds(name)
            _, ocam = self.cameras(view, W / H)
            exp, ctr = self.oracle.render(ow, ocam, self.oracle.params(W, H, spp, max_depth=depth, adaptive=adaptive, seed=SEED))
            exp.setflags(write=False)
            self.frames[key] = (exp, ctr)
        return self.frames[key]

    def render(self, name, W, H, spp, depth=50, adaptive=False, view=None, kernel="bvh2", tail=0, streams=0, lists=None,
               counting=1, timing=False):
        """-> (pixels, the call's counters, the kernel times when `timing`)"""
        from raytracingoneweekend_amd import _lib as L
        w, _ = self.worlds(name)
        cam, _ = self.cameras(view, W / H)
        fz = w.freeze(cam, kernel=kernel, pipeline="wavefront")
        try:
            L.check(L.lib.om_set_tail_bounce(fz.ctx, tail), fz.ctx)
            L.check(L.lib.om_set_counting(fz.ctx, counting), fz.ctx)
            if streams:
                L.check(L.lib.om_set_streams(fz.ctx, streams), fz.ctx)
            if lists is not None:
                L.check(L.lib.om_set_primary_lists(fz.ctx, lists), fz.ctx)
            if timing:
                L.check(L.lib.om_set_timing(fz.ctx, 1), fz.ctx)
            pix = self.om.PixelsBox.new(W * H)
            ctr = self.om.render(cam, fz, depth, 0.001, 100.0, spp, W, H, pix, seed=SEED, adaptive=adaptive)
            kt = None
            if timing:
                kt = L.om_kernel_times()
                L.check(L.lib.om_get_kernel_times(fz.ctx, C.byref(kt)), fz.ctx)
        finally:
            fz.close()
        return pix.pixels, ctr, kt

    def check(self, label, name, W, H, spp, **kw):
        okw = {k: kw[k] for k in ("depth", "adaptive", "view") if k in kw}
        exp, _ = self.expected(name, W, H, spp, **okw)
        got, ctr, _ = self.render(name, W, H, spp, **kw)
        nb, msg = compare_stats(got, exp, label)
        assert nb == 0, msg
        return got, ctr


@pytest.fixture(scope="module")
def frames(om, oracle):
    f = _Frames(om, oracle)
    yield f
    f.frames.clear()


@pytest.mark.parametrize("counting", [1, 0])
@pytest.mark.parametrize("depth", [1, 2, 3, 50])
def test_max_depth(frames, depth, counting):
    """Paths that end inside the fused second segment, the -0 exhaustion written from it."""
    W, H, SPP = 64, 40, 4
    got, _ = frames.check(f"depth{depth}/count{counting}", "S-traced", W, H, SPP, depth=depth, counting=counting)
    assert (got["n"] == SPP).all()


@pytest.mark.parametrize("counting", [1, 0])
@pytest.mark.parametrize("view", ["sky", "ground"])
def test_survivor_extremes(frames, view, counting):
    W, H, SPP = 64, 40, 4
    got, _ = frames.check(f"{view}/count{counting}", "S-traced", W, H, SPP, view=view, counting=counting)
    seen = int((got["bloom"] != 0).sum())
    assert seen == (0 if view == "sky" else W * H), f"{view}: {seen} of {W * H} pixels saw an object"


@pytest.mark.parametrize("counting", [1, 0])
@pytest.mark.parametrize("size", [(70, 37), (1, 7)])
def test_ragged_frames(frames, size, counting):
    W, H = size
    got, _ = frames.check(f"{W}x{H}/count{counting}", "S-traced", W, H, 4, counting=counting)
    assert (got["n"] == 4).all()


@pytest.mark.parametrize("lists", [0, 1, 2])
def test_primary_lists(frames, lists):
    for counting in (1, 0):
        frames.check(f"lists{lists}/count{counting}", "S-traced", 70, 37, 4, lists=lists, counting=counting)


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("tail", [1, 2, 3, 0])
def test_tail_threshold(frames, tail, streams):
    frames.check(f"tail{tail}/streams{streams}", "S-traced", 64, 40, 4, tail=tail, streams=streams, counting=streams - 1)


def test_adaptive(frames):
    """One adaptive call: the serial schedule, two streams and the oracle agree."""
    W, H, SPP = 64, 40, 24
    serial, _ = frames.check("adaptive/streams1", "S-traced", W, H, SPP, adaptive=True, streams=1)
    two, _ = frames.check("adaptive/streams2", "S-traced", W, H, SPP, adaptive=True, streams=2, counting=0)
    nb, msg = compare_stats(two, serial, "adaptive/2 vs 1")
    assert nb == 0, msg
    assert int(serial["n"].min()) < SPP


@pytest.mark.parametrize("name,kernel", [("g17", "bvh2"), ("g17", "bvh4"), ("S-traced", "bvh4")])
def test_other_trees(frames, name, kernel):
    """The tree read through L2 (g17) and the 4-wide tree."""
    for counting in (1, 0):
        frames.check(f"{name}/{kernel}/count{counting}", name, 64, 40, 4, kernel=kernel, counting=counting)


def test_counters(frames):
    """Both segments of the fused launch are counted: `segments` is the oracle's total, and the exact
    and box tests are what the library counted when bounce 1 was a launch of its own (the parent
    commit's totals for this render, tests/golden/fused_counters.json)."""
    W, H, SPP = 64, 40, 4
    _, octr = frames.expected("S-traced", W, H, SPP)
    _, ctr = frames.check("counters", "S-traced", W, H, SPP, counting=1)
    with open(GOLDEN) as f:
        want = json.load(f)["S-traced 64x40 4spp seed 17 bvh2 wavefront"]
    print({k: ctr[k] for k in ("samples", "segments", "prim_tests", "pre_tests")}, "recorded", want)
    assert ctr["samples"] == octr["samples"] == W * H * SPP
    assert ctr["segments"] == octr["segments"] == want["segments"]
    assert ctr["prim_tests"] == want["prim_tests"]
    assert ctr["pre_tests"] == want["pre_tests"]


def test_launch_counts(frames):
    """One 16-spp batch on one stream: the first launch, 15 per-bounce launches (bounces 2-16), the tail."""
    from raytracingoneweekend_amd import _lib as L
    W, H, SPP = 64, 40, 16
    exp, _ = frames.expected("S-traced", W, H, SPP)
    got, _, kt = frames.render("S-traced", W, H, SPP, kernel="auto", streams=1, timing=True)
    nb, msg = compare_stats(got, exp, "launch counts")
    assert nb == 0, msg
    n = {c: int(kt.launches[L.KT_CLASSES.index(c)]) for c in ("bounce0", "bounce", "tail", "accumulate")}
    assert n == {"bounce0": 1, "bounce": 15, "tail": 1, "accumulate": 1}, n
