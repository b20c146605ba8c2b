"""The traced tail (k_tail) against the oracle, all 40 bytes of every pixel.

The tail numbers the paths of a whole queue through the prefix of its segment counts, deals them
in 64-path units over a resident grid and, when the queue is longer than the grid's lanes, lets
ended lanes claim the rest from one counter per queue set, which the batch's bounce 0 zeroes.
The shapes are the smallest at which each of those parts can go wrong:

* refill + stale counter: S-traced 400x225, tail from bounce 1, two 32-spp calls into one Stats
  (2.9M camera paths per call on one stream, 1.4M per batch on two): more paths enter the tail
  than the grid has lanes, and each queue set's second tail finds the counter its first one left;
* sparse deal: 64x48 at 4 spp: far fewer 64-path units than workgroups;
* empty tail: max_depth 1 / 2 and a sky-only view, then a normal call on the same context;
* zero-count segments between full ones: the S-traced frame (sky rows), a single-sphere and a
  single-plane world (scenes_common has no world named for this; these are the one-primitive
  worlds of test_gpu_parity.test_sparse_worlds_bit_exact);
* every tracer the tail is built for: an LDS tree and an L2 tree (g17) under bvh2 and bvh4;
* adaptive calls (tail 8) on 1 and 2 streams; a pixel list sharded over 3 logical ranks.

Oracle frames are rendered once per module and shared read-only.
"""
import ctypes as C

import numpy as np
import pytest

from scenes_common import REGIME_WORLDS, compare_stats

pytestmark = pytest.mark.gpu

SEED = 5


class _Frames:
    """Oracle frames keyed by (world, W, H, spp, depth, adaptive), each rendered once."""

    def __init__(self, om, oracle):
        self.om, self.oracle, self.frames = om, oracle, {}

    def worlds(self, name):
        om, O = self.om, self.oracle
        if name == "S-traced":
            return om.random_scene(0x5EED), O.random_scene(0x5EED)
        if name in REGIME_WORLDS:
            return REGIME_WORLDS[name][0](om, O)
        mats = (om.Material.new_lambertian((0.4, 0.5, 0.6)), O.material("lambertian", (0.4, 0.5, 0.6)))
        w, ow = om.HittableList.new(), O.World()
        if name == "sphere":
            w += om.Sphere.new_with_radius((0., 1., 0.), 1., mats[0]); ow.add_sphere_radius((0., 1., 0.), 1., mats[1])
        elif name == "plane":
            w += om.InfinitePlane.new((0., 0., 0.), (0., 1., 0.), mats[0]); ow.add_plane((0., 0., 0.), (0., 1., 0.), mats[1])
        else:
            raise KeyError(name)
        return w, ow

    def cameras(self, name, aspect):
        if name == "sky":                       # looks straight up from above the ground: sky only
            args = ((0., 5., 0.), (0., 50., 0.1), (0., 0., 1.), 20., aspect, 0., 10.)
            return self.om.Camera.new(*args), self.oracle.camera(*args)
        return self.om.default_camera(aspect), self.oracle.default_camera(aspect)

    def expected(self, name, W, H, spp, depth=50, adaptive=False, view=None):
        key = (name, W, H, spp, depth, adaptive, view)
        if key not in self.frames:
            _, ow = self.worlds(name)
            _, ocam = self.cameras(view or name, W / H)
            exp, _ = self.oracle.render(ow, ocam, self.oracle.params(W, H, spp, max_depth=depth, adaptive=adaptive, seed=SEED))
            exp.setflags(write=False)
            self.frames[key] = exp
        return self.frames[key]

    def render(self, name, W, H, spp, tail, depth=50, adaptive=False, kernel="auto", streams=0, calls=None, view=None,
               fz=None):
        """`calls` sample counts into one Stats on one context (default: one call of spp)."""
        from raytracingoneweekend_amd import _lib as L
        w, _ = self.worlds(name)
        cam, _ = self.cameras(view or name, W / H)
        own = fz is None
        if own:
            fz = w.freeze(cam, kernel=kernel, pipeline="wavefront")
        try:
            L.check(L.lib.om_set_tail_bounce(fz.ctx, tail), fz.ctx)
            if streams:
                L.check(L.lib.om_set_streams(fz.ctx, streams), fz.ctx)
            pix = self.om.PixelsBox.new(W * H)
            for c in calls or (spp,):
                self.om.render(cam, fz, depth, 0.001, 100.0, spp, W, H, pix, seed=SEED, adaptive=adaptive, sample_count=c)
        finally:
            if own:
                fz.close()
        return pix.pixels


@pytest.fixture(scope="module")
def frames(om, oracle):
    f = _Frames(om, oracle)
    yield f
    f.frames.clear()


@pytest.mark.parametrize("streams", [1, 2])
def test_refill_and_counter_reset(frames, streams):
    """More paths than the grid's lanes enter each tail, twice per queue set."""
    W, H, SPP = 400, 225, 64
    got = frames.render("S-traced", W, H, SPP, tail=1, streams=streams, calls=(32, 32))
    nb, msg = compare_stats(got, frames.expected("S-traced", W, H, SPP), f"refill/streams{streams}")
    assert nb == 0, msg
    assert (got["n"] == SPP).all()


@pytest.mark.parametrize("tail", [1, 0])
def test_sparse_deal(frames, tail):
    """Far fewer units than workgroups (tail 0: the library's default threshold)."""
    W, H, SPP = 64, 48, 4
    got = frames.render("S-traced", W, H, SPP, tail=tail)
    nb, msg = compare_stats(got, frames.expected("S-traced", W, H, SPP), f"sparse deal/tail{tail}")
    assert nb == 0, msg


@pytest.mark.parametrize("case", ["depth1", "depth2", "sky"])
def test_empty_tail_then_normal_call(frames, case):
    """A tail with nothing to do returns before staging; the next batch on the context is whole.
    (max_depth 1: no tail launch at all; max_depth 2: every path entering bounce 1 ends there;
    sky: every camera path ends at bounce 0, so the tail's queue is empty.)"""
    W, H, SPP = 64, 48, 4
    w, _ = frames.worlds("g0x" if case == "sky" else "S-traced")
    name = "g0x" if case == "sky" else "S-traced"
    view = "sky" if case == "sky" else None
    depth = {"depth1": 1, "depth2": 2, "sky": 50}[case]
    cam, _ = frames.cameras(view or name, W / H)
    fz = w.freeze(cam, pipeline="wavefront")
    try:
        got = frames.render(name, W, H, SPP, tail=1, depth=depth, view=view, fz=fz)
        nb, msg = compare_stats(got, frames.expected(name, W, H, SPP, depth=depth, view=view), f"empty tail/{case}")
        assert nb == 0, msg
        if case == "sky":
            assert int((got["bloom"] != 0).sum()) == 0, "the sky view must see nothing"
        # the same context, the same camera, a full-depth call
        got = frames.render(name, W, H, SPP, tail=1, view=view, fz=fz)
        nb, msg = compare_stats(got, frames.expected(name, W, H, SPP, view=view), f"after empty tail/{case}")
        assert nb == 0, msg
    finally:
        fz.close()


@pytest.mark.parametrize("name", ["sphere", "plane", "g0"])
def test_zero_count_segments(frames, name):
    """One-primitive worlds: most of the frame is sky, so most segments enter the tail empty."""
    W, H, SPP = 64, 48, 4
    got = frames.render(name, W, H, SPP, tail=1)
    nb, msg = compare_stats(got, frames.expected(name, W, H, SPP), f"zero segments/{name}")
    assert nb == 0, msg


@pytest.mark.parametrize("kernel", ["bvh2", "bvh4"])
@pytest.mark.parametrize("name", ["S-traced", "g17"])
def test_every_tracer(frames, name, kernel):
    """The tail's instantiations: trees staged in LDS (S-traced) and read through L2 (g17)."""
    W, H, SPP = 160, 90, 8
    got = frames.render(name, W, H, SPP, tail=1, kernel=kernel)
    nb, msg = compare_stats(got, frames.expected(name, W, H, SPP), f"tracer/{name}/{kernel}")
    assert nb == 0, msg


@pytest.mark.parametrize("streams", [1, 2])
def test_adaptive(frames, streams):
    W, H, SPP = 160, 90, 24
    got = frames.render("S-traced", W, H, SPP, tail=8, adaptive=True, streams=streams)
    nb, msg = compare_stats(got, frames.expected("S-traced", W, H, SPP, adaptive=True), f"adaptive/streams{streams}")
    assert nb == 0, msg
    assert int(got["n"].min()) < SPP


def test_sharded_pixel_list(frames):
    """om_shard_pixels' deal over 3 logical ranks, each rank's list rendered on its own, tail 1."""
    import torch
    from raytracingoneweekend_amd import _lib as L
    from raytracingoneweekend_amd import shard
    om = frames.om
    W, H, SPP = 160, 90, 4
    w, _ = frames.worlds("S-traced")
    cam = om.default_camera(W / H)
    fz = w.freeze(cam, pipeline="wavefront")
    try:
        L.check(L.lib.om_set_tail_bounce(fz.ctx, 1), fz.ctx)
        p = om.make_params(50, 0.001, 100.0, SPP, W, H, seed=SEED)
        shards = []
        for r in range(3):
            pix = shard.tile_pixels(W, H, r, 3)
            dpix = torch.from_numpy(pix.view(np.int32)).cuda()
            st = torch.zeros(pix.size * 40, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()       # torch's fill and copy are queued on its stream, the render on the ctx's own
            L.check(L.lib.om_render_device_pixels(fz.ctx, C.byref(cam.raw), C.byref(p), C.c_void_p(st.data_ptr()),
                                                  C.c_void_p(dpix.data_ptr()), pix.size, None), fz.ctx)
            torch.cuda.synchronize()
            shards.append(st.cpu().numpy())
    finally:
        fz.close()
    frame = shard.assemble(W, H, shards)
    nb, msg = compare_stats(frame, frames.expected("S-traced", W, H, SPP), "sharded")
    assert nb == 0, msg
