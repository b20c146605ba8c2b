"""Bounce 0's deal (csrc/om_deal.h) against the oracle, all 40 bytes of every pixel.

Bounce 0 (k_bounce's FIRST branch, k_raygen for marched worlds) numbers the batch's camera samples in
blocks of 64 and deals the blocks round-robin over the workgroups, OM_WF_DEAL_BLOCKS at a time; the
survivors of workgroup g go into queue segment g.  Results are keyed by the sample's batch index and
the RNG by (pixel, sample), so no bit may change.  The shapes are the smallest at which the deal can
go wrong:

* 8x8 at 1 spp: one block, two workgroups: every other workgroup is empty (and still writes its count);
* 50x37 at 3 spp: ragged tiles; two batches on the default two streams, 3700 samples in 58 blocks
  over 8 workgroups and 1850 in 29 over 4 (no multiples): each batch's last block is partial, and at
  the shipped OM_WF_DEAL_BLOCKS = 8 its last group is short;
* 96x64 at 4 spp: 384 blocks over 48 workgroups on one stream, 192 over 24 per batch on two, as
  1-spp calls 96 over 12: 8 blocks per workgroup, one round of the shipped OM_WF_DEAL_BLOCKS = 8
  (several rounds of a smaller one);
* 400x225 at 8 spp on one stream: 720 000 samples, more than the 1024 workgroups of a 256-CU device
  take 512 each, so the grid is capped and the 1407 groups of 8 blocks go round the workgroups
  more than once, the last round reaching only some of them (the shapes above give a workgroup per
  512 samples, which is one group);
* the 96x64 frame as the pixel lists of 3 logical ranks, each through om_render_device_pixels with
  its shard as the Stats (what om_render_shard calls for its rank; by_pixel = 0): 32 blocks per
  sample of a list that is every third tile of the frame;
* the 96x64 frame adaptive on 1 and 2 streams: the batches' path counts (live pixels x planned
  samples) are known only on the device, which evaluates the deal from them.  Half of S-traced's
  pixels never retire at this size, so the same frame of a single-sphere world follows: its last
  16-spp call starts with 61 live pixels, less than one block (the oracle frame is asserted to);
* a marched world at 40x24, 2 spp: k_raygen's deal;
* S-traced 160x90 at 16 spp with the tail forced to bounce 2 and at the default threshold.

Every fixed-spp case is also rendered as 1-spp calls into one Stats, which must give the same bytes.
Oracle frames are rendered once per module and shared read-only.
"""
import ctypes as C

import numpy as np
import pytest

from scenes_common import compare_stats

pytestmark = pytest.mark.gpu

SEED = 9
MARCH_STEPS = 256


class _Frames:
    def __init__(self, om, oracle):
        self.om, self.oracle, self.frames = om, oracle, {}

    def worlds(self, name):
        om, O = self.om, self.oracle
        if name == "S-marched":
            return om.marched_scene(), O.marched_scene()
        if name == "sphere":
            mats = (om.Material.new_lambertian((0.4, 0.5, 0.6)), O.material("lambertian", (0.4, 0.5, 0.6)))
            w, ow = om.HittableList.new(), O.World()
            w += om.Sphere.new_with_radius((0., 1., 0.), 1., mats[0]); ow.add_sphere_radius((0., 1., 0.), 1., mats[1])
            return w, ow
        return om.random_scene(0x5EED), O.random_scene(0x5EED)

    def expected(self, name, W, H, spp, adaptive=False):
        key = (name, W, H, spp, adaptive)
        if key not in self.frames:
            _, ow = self.worlds(name)
            exp, _ = self.oracle.render(ow, self.oracle.default_camera(W / H),
                                        self.oracle.params(W, H, spp, adaptive=adaptive, seed=SEED, march_steps=MARCH_STEPS))
            exp.setflags(write=False)
            self.frames[key] = exp
        return self.frames[key]

    def render(self, name, W, H, spp, calls=None, tail=0, streams=0, adaptive=False):
        """`calls` sample counts into one Stats on one context (default: one call of spp)."""
        from raytracingoneweekend_amd import _lib as L
        w, _ = self.worlds(name)
        cam = self.om.default_camera(W / H)
        fz = w.freeze(cam, pipeline="wavefront")
        try:
            L.check(L.lib.om_set_tail_bounce(fz.ctx, tail), fz.ctx)
            if streams:
                L.check(L.lib.om_set_streams(fz.ctx, streams), fz.ctx)
            pix = self.om.PixelsBox.new(W * H)
            for c in calls or (spp,):
                self.om.render(cam, fz, 50, 0.001, 100.0, spp, W, H, pix, seed=SEED, march_steps=MARCH_STEPS,
                               adaptive=adaptive, sample_count=c)
        finally:
            fz.close()
        return pix.pixels


@pytest.fixture(scope="module")
def frames(om, oracle):
    f = _Frames(om, oracle)
    yield f
    f.frames.clear()


def _fixed(frames, name, W, H, spp, label, **kw):
    """One call of spp == spp one-sample calls == the oracle."""
    exp = frames.expected(name, W, H, spp)
    got = frames.render(name, W, H, spp, **kw)
    nb, msg = compare_stats(got, exp, label)
    assert nb == 0, msg
    assert (got["n"] == spp).all()
    one = frames.render(name, W, H, spp, calls=(1,) * spp, **kw)
    nb, msg = compare_stats(one, exp, label + " as 1-spp calls")
    assert nb == 0, msg
    assert got.tobytes() == one.tobytes()


def test_one_block_and_an_empty_workgroup(frames):
    _fixed(frames, "S-traced", 8, 8, 1, "8x8x1")


def test_partial_last_block_ragged_tiles(frames):
    _fixed(frames, "S-traced", 50, 37, 3, "50x37x3")


@pytest.mark.parametrize("streams", [1, 2])
def test_eight_blocks_per_workgroup(frames, streams):
    _fixed(frames, "S-traced", 96, 64, 4, f"96x64x4/streams{streams}", streams=streams)


def test_capped_grid_more_than_one_round(frames):
    _fixed(frames, "S-traced", 400, 225, 8, "400x225x8/streams1", streams=1)


def test_three_logical_ranks(frames):
    import torch
    from raytracingoneweekend_amd import _lib as L
    from raytracingoneweekend_amd import shard
    om = frames.om
    W, H, SPP = 96, 64, 4
    w, _ = frames.worlds("S-traced")
    cam = om.default_camera(W / H)
    fz = w.freeze(cam, pipeline="wavefront")
    try:
        p = om.make_params(50, 0.001, 100.0, SPP, W, H, seed=SEED, march_steps=MARCH_STEPS)
        shards = []
        for r in range(3):
            pix = shard.tile_pixels(W, H, r, 3)
            dpix = torch.from_numpy(pix.view(np.int32)).cuda()
            st = torch.zeros(pix.size * 40, dtype=torch.uint8, device="cuda")
            L.check(L.lib.om_render_device_pixels(fz.ctx, C.byref(cam.raw), C.byref(p), C.c_void_p(st.data_ptr()),
                                                  C.c_void_p(dpix.data_ptr()), pix.size, None), fz.ctx)
            torch.cuda.synchronize()
            shards.append(st.cpu().numpy())
    finally:
        fz.close()
    nb, msg = compare_stats(shard.assemble(W, H, shards), frames.expected("S-traced", W, H, SPP), "3 ranks")
    assert nb == 0, msg


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("name", ["S-traced", "sphere"])
def test_adaptive_device_planned_batches(frames, name, streams):
    W, H, SPP = 96, 64, 96
    exp = frames.expected(name, W, H, SPP, adaptive=True)
    assert int(exp["n"].min()) < 16, "pixels must retire within the first call"
    if name == "sphere":
        assert 0 < int((exp["n"] > SPP - 16).sum()) < 64, "the last call must start with less than a block of live pixels"
    got = frames.render(name, W, H, SPP, calls=(16,) * 6, streams=streams, adaptive=True)
    nb, msg = compare_stats(got, exp, f"adaptive/{name}/streams{streams}")
    assert nb == 0, msg


def test_marched_world_raygen(frames):
    _fixed(frames, "S-marched", 40, 24, 2, "marched 40x24x2")


@pytest.mark.parametrize("tail", [2, 0])
def test_traced_world_into_the_tail(frames, tail):
    _fixed(frames, "S-traced", 160, 90, 16, f"160x90x16/tail{tail}", tail=tail)
