"""The frame-from-rays ABI (om_render_rays*) without a GPU: header / exports / binding, the status
codes that need no device, the Python wrapper's argument checks, and the test helper that derives the
thin-lens camera's rays against the one the radiance-query tests use."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from frame_rays_common import frame_rays
from paths_common import camera_paths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["om_render_rays_device", "om_render_rays"]


def test_header_exports_and_binding_agree(om):
    from raytracingoneweekend_amd import _lib
    src = open(os.path.join(ROOT, "include", "ottomarcher.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"\s+", " ", src)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(raw, name), name
    vp, pp = C.c_void_p, C.POINTER(_lib.om_render_params)
    assert _lib.lib.om_render_rays_device.argtypes == [vp, pp, vp, vp, vp, C.c_uint32, vp, vp]
    assert _lib.lib.om_render_rays.argtypes == [vp, pp, vp, vp, vp, C.c_uint32, vp, C.POINTER(_lib.om_counters)]
    assert ("om_status om_render_rays_device(om_ctx* ctx, const om_render_params* p, const om_ray* dev_rays , "
            "const uint64_t* dev_rng , const uint32_t* dev_pixels , uint32_t n_pixels, om_pixel_stats* dev_stats , "
            "void* stream);") in src
    assert ("om_status om_render_rays(om_ctx* ctx, const om_render_params* p, const om_ray* rays, const uint64_t* rng, "
            "const uint32_t* pixels, uint32_t n_pixels, om_pixel_stats* stats, om_counters* counters );") in src
    assert _lib.lib.om_abi_version() == 2                           # new exports only: no layout or meaning changed


def test_cpp_wrapper_declares_render_rays():
    src = open(os.path.join(ROOT, "include", "ottomarcher.hpp")).read()
    assert re.search(r"om_counters render_rays\(std::vector<om_pixel_stats>& stats, const std::vector<om_ray>& rays", src)


def test_null_ctx_is_invalid_and_writes_nothing(om):
    from raytracingoneweekend_amd import _lib
    L = _lib.lib
    p = om.make_params(50, 0.001, 100.0, 4, 4, 2, sample_count=1)
    rays = np.zeros((8, 6), dtype=np.float32)
    stats = np.zeros(8, dtype=_lib.PIXEL_STATS_DTYPE)
    ctr = _lib.om_counters()
    rp, sp = rays.ctypes.data_as(C.c_void_p), stats.ctypes.data_as(C.c_void_p)
    assert L.om_render_rays(None, C.byref(p), rp, None, None, 8, sp, C.byref(ctr)) == _lib.OM_ERR_INVALID
    assert b"null ctx" in L.om_last_error(None)
    assert L.om_render_rays_device(None, C.byref(p), rp, None, None, 8, sp, None) == _lib.OM_ERR_INVALID
    assert L.om_render_rays(None, None, None, None, None, 0, None, None) == _lib.OM_ERR_INVALID
    assert not stats.view(np.uint8).any() and ctr.samples == 0


def _unbound(om):
    """A FrozenHittableList without a ctx: the wrapper's own checks run before any library call."""
    fz = object.__new__(om.FrozenHittableList)
    fz._ctx, fz.device = C.c_void_p(), 0
    return fz


@pytest.mark.parametrize("what", ["rays_shape", "rays_rows", "rays_dtype", "stats_size", "stats_dtype", "rng_dtype",
                                  "rng_size", "pixels_dtype", "pixels_too_many", "pixels_2d", "frame"])
def test_wrapper_rejects_wrong_shapes_and_dtypes(om, what):
    from raytracingoneweekend_amd import _lib
    fz = _unbound(om)
    W, H, S = 4, 2, 3
    rays = np.zeros((S, W * H, 6), dtype=np.float32)
    stats = np.zeros(W * H, dtype=_lib.PIXEL_STATS_DTYPE)
    kw = {}
    if what == "rays_shape":
        rays = np.zeros((S, W * H, 5), dtype=np.float32)
    elif what == "rays_rows":
        rays = np.zeros((S * W * H + 1, 6), dtype=np.float32)      # no whole number of samples
    elif what == "rays_dtype":
        rays = rays.astype(np.float64)
    elif what == "stats_size":
        stats = stats[:-1]
    elif what == "stats_dtype":
        stats = np.zeros((W * H, 40), dtype=np.uint8)
    elif what == "rng_dtype":
        kw["rng"] = np.zeros((S, W * H), dtype=np.int64)
    elif what == "rng_size":
        kw["rng"] = np.zeros(W * H, dtype=np.uint64)
    elif what == "pixels_dtype":
        kw["pixels"], rays = np.arange(5, dtype=np.int64), rays[:, :5].copy()
    elif what == "pixels_too_many":
        kw["pixels"], rays = np.zeros(W * H + 1, dtype=np.uint32), np.zeros((S, W * H + 1, 6), dtype=np.float32)
    elif what == "pixels_2d":
        kw["pixels"] = np.zeros((2, 4), dtype=np.uint32)
    elif what == "frame":
        W = 0
    with pytest.raises(ValueError, match="render_rays"):
        fz.render_rays(stats, rays, W, H, 12, **kw)


def test_wrapper_rejects_mixed_numpy_and_torch(om):
    import torch
    from raytracingoneweekend_amd import _lib
    fz = _unbound(om)
    W, H, S = 4, 2, 3
    rays = np.zeros((S, W * H, 6), dtype=np.float32)
    stats = np.zeros(W * H, dtype=_lib.PIXEL_STATS_DTYPE)
    for args, kw in [((stats, torch.zeros(S, W * H, 6)), {}),
                     ((torch.zeros(W * H, 40, dtype=torch.uint8), rays), {}),
                     ((stats, rays), {"rng": torch.zeros(S, W * H, dtype=torch.int64)}),
                     ((stats, rays), {"pixels": torch.zeros(W * H, dtype=torch.int32)})]:
        with pytest.raises(ValueError, match="all numpy or all torch"):
            fz.render_rays(*args, W, H, 12, **kw)
    with pytest.raises(ValueError, match="on the device"):          # torch, but host tensors
        fz.render_rays(torch.zeros(W * H, 40, dtype=torch.uint8), torch.zeros(S, W * H, 6), W, H, 12)


def test_helper_agrees_with_the_one_sample_helper(oracle):
    """frame_rays with S = 1 is paths_common.camera_paths: the same rays and states, as bits."""
    O = oracle
    W, H, seed = 20, 13, 7
    ocam = O.default_camera(W / H)
    rays, states = frame_rays(O, ocam, W, H, seed, 1)
    r1, s1, _ = camera_paths(O, ocam, W, H, seed)
    assert rays.shape == (1, W * H, 6) and states.shape == (1, W * H)
    assert rays[0].tobytes() == r1.tobytes() and states[0].tobytes() == s1.tobytes()
    px = [259, 0, 77]
    rays, states = frame_rays(O, ocam, W, H, seed, 1, pixels=px)
    assert rays[0].tobytes() == r1[px].tobytes() and states[0].tobytes() == s1[px].tobytes()


def test_helper_samples_are_distinct_streams(oracle):
    """Sample s of a 3-sample table enters ray_color on stream (seed, px, s): the key word differs by sample."""
    O = oracle
    _, states = frame_rays(O, O.default_camera(2.0), 4, 2, 7, 3)
    keys = states >> np.uint64(32)
    assert len(set(keys.reshape(-1).tolist())) == keys.size
