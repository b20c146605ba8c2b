"""The radiance-query ABI (om_ray_color*, om_path_rng_state, om_set_path_batch) without a GPU: record
layouts, header / exports / binding, the host-side RNG state against the Python restatement of om-rng
v2, and argument validation."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from paths_common import advance, path_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["om_path_rng_state", "om_ray_color_device", "om_ray_color", "om_set_path_batch"]


def test_record_sizes(om):
    from raytracingoneweekend_amd import _lib
    assert C.sizeof(_lib.om_path_params) == 32
    assert C.sizeof(_lib.om_radiance) == 20
    assert om.RADIANCE_DTYPE.itemsize == 20
    assert [om.RADIANCE_DTYPE.fields[n][1] for n in ("color", "depth", "obj")] == [0, 12, 16]
    assert [getattr(_lib.om_path_params, n).offset for n in
            ("tmin", "tmax", "march_steps", "max_depth", "seed", "stream_base", "sample")] == [0, 4, 8, 12, 16, 24, 28]


def test_header_exports_and_binding_agree(om):
    from raytracingoneweekend_amd import _lib
    src = open(os.path.join(ROOT, "include", "ottomarcher.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(om_[a-z0-9_]+)\s*\(", src))
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(raw, name), name
        assert getattr(_lib.lib, name).argtypes is not None, name
    for struct in ("om_path_params", "om_radiance"):
        assert re.search(r"typedef struct %s\b" % struct, src), struct


# the (seed, pixel, sample) tuples of tests/test_oracle_kat.py's path-stream test
@pytest.mark.parametrize("seed,pixel,sample", [(1, 0, 0), (1, 12345, 7), (0x5EED, 2073599, 511), (2 ** 63, 7, 2 ** 31)])
@pytest.mark.parametrize("draws", [0, 2, 7, 2 ** 32 - 1])
def test_path_rng_state_matches_python_restatement(om, seed, pixel, sample, draws):
    assert om.path_rng_state(seed, pixel, sample, draws) == advance(path_state(seed, pixel, sample), draws)


def test_path_rng_state_is_the_oracles_stream(om, oracle):
    """The draws that follow the state are the oracle's draws of the same stream from there on."""
    from paths_common import draw
    st = om.path_rng_state(0x5EED, 321, 5, 3)
    got = []
    for _ in range(8):
        d, st = draw(st)
        got.append(d)
    assert np.array_equal(np.array(got, dtype=np.float32), oracle.path_draws(0x5EED, 321, 5, 11)[3:])


def test_argument_validation_without_a_ctx(om):
    from raytracingoneweekend_amd import _lib
    L = _lib.lib
    p = _lib.om_path_params(0.001, 100.0, 1024, 50, 1, 0, 0)
    rays = np.zeros((4, 6), dtype=np.float32)
    out = np.zeros(4, dtype=om.RADIANCE_DTYPE)
    rp, op = rays.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert L.om_ray_color(None, C.byref(p), rp, None, 4, op) == _lib.OM_ERR_INVALID
    assert b"null ctx" in L.om_last_error(None)
    assert L.om_ray_color_device(None, C.byref(p), rp, None, 4, op, None) == _lib.OM_ERR_INVALID
    assert L.om_ray_color(None, None, None, None, 0, None) == _lib.OM_ERR_INVALID
    assert L.om_set_path_batch(None, 0) == _lib.OM_ERR_INVALID
    assert not out.view(np.uint8).any()                             # a failed call writes nothing


def test_argument_validation_with_a_ctx(om):
    """Null pointers, a NaN window, the knob's range, and OM_ERR_STATE before the upload: where a ctx
    can exist (om_create needs a device)."""
    from raytracingoneweekend_amd import _lib
    L = _lib.lib
    ctx = C.c_void_p()
    if L.om_create(0, C.byref(ctx)) != _lib.OM_OK:
        pytest.skip("no device, no ctx")
    try:
        p = _lib.om_path_params(0.001, 100.0, 1024, 50, 1, 0, 0)
        rays = np.zeros((4, 6), dtype=np.float32)
        out = np.zeros(4, dtype=om.RADIANCE_DTYPE)
        rp, op = rays.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
        assert L.om_ray_color(ctx, C.byref(p), rp, None, 4, op) == _lib.OM_ERR_STATE
        assert L.om_ray_color(ctx, None, rp, None, 4, op) == _lib.OM_ERR_INVALID
        nan = _lib.om_path_params(float("nan"), 100.0, 1024, 50, 1, 0, 0)
        assert L.om_ray_color(ctx, C.byref(nan), rp, None, 4, op) == _lib.OM_ERR_INVALID
        for bad in (1, 5, 28):
            assert L.om_set_path_batch(ctx, bad) == _lib.OM_ERR_INVALID
        for ok in (6, 27, 0):
            assert L.om_set_path_batch(ctx, ok) == _lib.OM_OK
        w = om.HittableList.new()
        w += om.Sphere.new_with_radius((0., 0., -3.), 1., om.Material.new_lambertian((0.5, 0.5, 0.5)))
        assert L.om_upload_world(ctx, w.handle) == _lib.OM_OK
        assert L.om_ray_color(ctx, C.byref(p), None, None, 4, op) == _lib.OM_ERR_INVALID
        assert L.om_ray_color(ctx, C.byref(p), rp, None, 4, None) == _lib.OM_ERR_INVALID
        assert L.om_ray_color(ctx, C.byref(p), None, None, 0, None) == _lib.OM_OK      # n == 0: no launch
        assert not out.view(np.uint8).any()
    finally:
        L.om_destroy(ctx)
