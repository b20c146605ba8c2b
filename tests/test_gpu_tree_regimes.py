"""Bit-exact parity with the oracle in every tree regime of the BVH2 / BVH4 / SBVH traversals.

Which traversal code a world runs is decided by size thresholds (om::plan_trees in om_world.h,
the leaf and code limits of om_bvh.cpp), not by the workload: BVH2 staged whole in LDS (nodes 80 B
apart, child codes scaled by 5) or read through L2 behind a 512-node LDS prefix; direct leaf
codes (OM_LEAF | first << 4 | count, decoded with an 11-bit mask) or the leaf table (staged behind
the padded nodes when the tree is in LDS); the max-leaf fallback tree from 32768 primitives; the
BVH4's own LDS cut; the megakernel's staged SBVH.  scenes_common.REGIME_WORLDS holds one small
world per regime and per budget edge, tests/test_tree_regimes.py (CPU) pins that each world is in
its regime, and this module renders each of them at 48x32 against the oracle, all 40 bytes of
every pixel.

The oracle's frames are rendered once per module and shared; the witness test shows from the
oracle alone that each frame really is a test of the tree (>= 100 distinct first-hit objects),
not of the ground sphere.
"""
import pytest

from scenes_common import REGIME_WORLDS, compare_stats

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH, SEED = 48, 32, 2, 50, 3
TAIL_SPP = 6

WORLDS = list(REGIME_WORLDS)
TREE_WORLDS = [n for n in WORLDS if n != "g0x"]          # ground only has no tree: the tail test renders it
CLUSTERS = [n for n in WORLDS if n.startswith("c")]
PAIRS = [("bvh2", "wavefront"), ("bvh4", "wavefront"), ("bvh2", "megakernel"), ("bvh4", "megakernel"), ("auto", "auto")]
# the two worlds on either side of the megakernel's staging budget (kLdsBudget, 96 KiB)
STAGING_CUT = ["g15", "g16"]
# worlds whose record indices pass 2048 or whose leaves hold 4 records (srec_box is indexed by record)
LIST_WORLDS = ["c7x18", "c8x17", "g91x"]


class _Regimes:
    """The regime worlds and the oracle's frames of them, each built / rendered once per module."""

    def __init__(self, om, oracle):
        self.om, self.oracle = om, oracle
        self.scenes, self.frames = {}, {}

    def scene(self, name):
        """(world, oracle world, camera, oracle camera)"""
        if name not in self.scenes:
            world_of, cams_of = REGIME_WORLDS[name]
            w, ow = world_of(self.om, self.oracle)
            cam, ocam = cams_of(self.om, self.oracle, W / H)
            self.scenes[name] = (w, ow, cam, ocam)
        return self.scenes[name]

    def expected(self, name, spp=SPP, adaptive=False):
        """The oracle's frame (read-only: shared between the tests)."""
        key = (name, spp, adaptive)
        if key not in self.frames:
            _, ow, _, ocam = self.scene(name)
            p = self.oracle.params(W, H, spp, max_depth=DEPTH, adaptive=adaptive, seed=SEED)
            exp, _ = self.oracle.render(ow, ocam, p)
            exp.setflags(write=False)
            self.frames[key] = exp
        return self.frames[key]

    def render(self, name, kernel, pipeline, spp=SPP, adaptive=False, setup=None):
        from raytracingoneweekend_amd import _lib as L
        w, _, cam, _ = self.scene(name)
        fz = w.freeze(cam, kernel=kernel, pipeline=pipeline)
        try:
            if setup:
                setup(L, fz)
            pix = self.om.PixelsBox.new(W * H)
            self.om.render(cam, fz, DEPTH, 0.001, 100.0, spp, W, H, pix, seed=SEED, adaptive=adaptive)
        finally:
            fz.close()
        return pix.pixels


@pytest.fixture(scope="module")
def regimes(om, oracle):
    r = _Regimes(om, oracle)
    yield r
    r.scenes.clear()
    r.frames.clear()


@pytest.mark.parametrize("name", WORLDS)
def test_frames_exercise_the_tree(regimes, name):
    """From the oracle alone: the 1-spp frame holds >= 100 distinct `bloom` words, i.e. 100 distinct
    first-hit objects (measured 114-333), and the cluster camera sees no sky.  The two worlds of
    fewer than 100 objects (g0x: the ground; g0: ground + three spheres) show every object they have."""
    w, _, _, _ = regimes.scene(name)
    one = regimes.expected(name, spp=1)
    words = set(one["bloom"].tolist()) - {0}
    objects = sum(w.counts().values())
    assert len(words) >= min(100, objects), f"{name}: only {len(words)} distinct first-hit objects of {objects}"
    if name in CLUSTERS:
        assert int((one["bloom"] == 0).sum()) == 0, f"{name}: the cluster camera sees sky"


@pytest.mark.parametrize("kernel,pipeline", PAIRS)
@pytest.mark.parametrize("name", TREE_WORLDS)
def test_regime_bit_exact(regimes, name, kernel, pipeline):
    got = regimes.render(name, kernel, pipeline)
    nb, msg = compare_stats(got, regimes.expected(name), f"{name}/{kernel}/{pipeline}")
    assert nb == 0, msg
    assert (got["n"] == SPP).all()


@pytest.mark.parametrize("name", WORLDS)
def test_regime_tail_bit_exact(regimes, name):
    """The persistent tail from bounce 2 with adaptive sampling: most segments run through k_tail's
    own instantiation of the traversal (as test_ten_k_half_bvh4_adaptive_and_tail_bit_exact does
    for the BVH4 of S-10k)."""
    got = regimes.render(name, "bvh2", "wavefront", spp=TAIL_SPP, adaptive=True,
                  setup=lambda L, fz: L.check(L.lib.om_set_tail_bounce(fz.ctx, 2), fz.ctx))
    nb, msg = compare_stats(got, regimes.expected(name, spp=TAIL_SPP, adaptive=True), f"{name}/tail 2")
    assert nb == 0, msg


@pytest.mark.parametrize("kernel", ["sbvh", "culled"])
@pytest.mark.parametrize("name", STAGING_CUT)
def test_megakernel_staging_cut_bit_exact(regimes, name, kernel):
    """g15: the stackless BVH and its records staged in LDS at 92 % of the 96 KiB budget; g16: the
    first world past it, read from global memory."""
    got = regimes.render(name, kernel, "megakernel")
    nb, msg = compare_stats(got, regimes.expected(name), f"{name}/{kernel}/megakernel")
    assert nb == 0, msg


@pytest.mark.parametrize("lists", [0, 2])
@pytest.mark.parametrize("name", LIST_WORLDS)
def test_primary_tile_lists_bit_exact(regimes, name, lists):
    """Primary-ray tile lists forced off (0) and on (2): they index srec_box and the records by
    record number, here past 2048 and with 4- and 7-record leaves."""
    got = regimes.render(name, "bvh2", "wavefront",
                  setup=lambda L, fz: L.check(L.lib.om_set_primary_lists(fz.ctx, lists), fz.ctx))
    nb, msg = compare_stats(got, regimes.expected(name), f"{name}/primary lists {lists}")
    assert nb == 0, msg
