"""The any-hit / per-ray-window additions to the C ABI (include/ottomarcher.h), without a device:
om_ray_window's layout in the header, the ctypes mirror and WINDOW_DTYPE; the four new entry
points declared, bound and exported; their null-ctx status; the ABI version unchanged."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ottomarcher.h")
NEW = ["om_occluded_rays_device", "om_occluded_rays", "om_hit_rays_windows_device", "om_hit_rays_windows"]
CTYPES_OF = {"float": C.c_float, "uint32_t": C.c_uint32}
NUMPY_OF = {"float": "<f4", "uint32_t": "<u4"}


def _header_window_fields():
    """[(type, name), ...] of `typedef struct om_ray_window { ... } om_ray_window;`"""
    text = open(HEADER).read()
    m = re.search(r"typedef\s+struct\s+om_ray_window\s*\{([^}]*)\}\s*om_ray_window\s*;", text)
    assert m, "om_ray_window is not declared in the header"
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, names = decl.split(None, 1)
        fields += [(ty, nm.strip()) for nm in names.split(",")]
    return fields


def test_window_record_matches_the_header(om):
    from raytracingoneweekend_amd import _lib as L
    fields = _header_window_fields()
    assert fields == [("float", "tmin"), ("float", "tmax")]
    assert C.sizeof(L.om_ray_window) == 8 and L.WINDOW_DTYPE.itemsize == 8
    assert om.WINDOW_DTYPE is L.WINDOW_DTYPE or om.WINDOW_DTYPE == L.WINDOW_DTYPE
    assert [(n, t) for n, t in L.om_ray_window._fields_] == [(nm, CTYPES_OF[ty]) for ty, nm in fields]
    assert L.WINDOW_DTYPE.names == tuple(nm for _, nm in fields)
    off = 0
    for ty, nm in fields:                                  # field by field: type, offset, no padding
        dt, o = L.WINDOW_DTYPE.fields[nm][:2]
        assert dt == np.dtype(NUMPY_OF[ty]) and o == off == getattr(L.om_ray_window, nm).offset
        off += dt.itemsize
    assert off == 8


def test_new_entry_points_declared_bound_and_exported(om):
    from raytracingoneweekend_amd import _lib as L
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(om_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared, f"{name} is not declared in the header"
        assert name in L.EXPORTS, f"{name} is missing from _lib.EXPORTS"
        f = getattr(L.lib, name)
        assert f.restype is C.c_int32 and f.argtypes is not None
    assert len(L.lib.om_occluded_rays_device.argtypes) == 7 and len(L.lib.om_occluded_rays.argtypes) == 6
    assert len(L.lib.om_hit_rays_windows_device.argtypes) == 7 and len(L.lib.om_hit_rays_windows.argtypes) == 6


def test_abi_version_is_unchanged(om):
    from raytracingoneweekend_amd import _lib as L
    assert L.lib.om_abi_version() == 2
    assert re.search(r"#define\s+OM_ABI_VERSION\s+2\b", open(HEADER).read())


def test_null_ctx_is_invalid_and_writes_nothing(om):
    from raytracingoneweekend_amd import _lib as L
    q = L.om_query_params(0.001, 100.0, 1024, 0)
    rays = np.zeros(4, dtype=L.RAY_DTYPE)
    rays["dir"][:, 2] = -1.0
    win = np.zeros(4, dtype=L.WINDOW_DTYPE)
    occ = np.full(4, 0xAA, dtype=np.uint8)
    hits = np.full(4 * 32, 0xAA, dtype=np.uint8)
    rp, wp = rays.ctypes.data_as(C.c_void_p), win.ctypes.data_as(C.c_void_p)
    op, hp = occ.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p)
    for wins in (wp, None):
        assert L.lib.om_occluded_rays(None, C.byref(q), rp, wins, 4, op) == L.OM_ERR_INVALID
        assert L.lib.om_occluded_rays_device(None, C.byref(q), rp, wins, 4, op, None) == L.OM_ERR_INVALID
        assert L.lib.om_hit_rays_windows(None, C.byref(q), rp, wins, 4, hp) == L.OM_ERR_INVALID
        assert L.lib.om_hit_rays_windows_device(None, C.byref(q), rp, wins, 4, hp, None) == L.OM_ERR_INVALID
    assert L.lib.om_occluded_rays(None, C.byref(q), None, None, 0, None) == L.OM_ERR_INVALID   # null ctx even with n == 0
    assert (occ == 0xAA).all() and (hits == 0xAA).all()
    assert L.lib.om_last_error(None)
