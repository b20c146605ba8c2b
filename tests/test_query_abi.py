"""The ray-query C-ABI without a GPU (include/ottomarcher.h: om_ray / om_hit / om_query_params,
om_hit_rays*, om_world_object_material): record layouts, the numpy / ctypes mirrors, argument
validation that needs no device, and the host-only material lookup."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from scenes_common import kitchen_sink

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "ottomarcher.h")).read()


def test_struct_sizes(om):
    from raytracingoneweekend_amd import _lib
    assert C.sizeof(_lib.om_ray) == 24
    assert C.sizeof(_lib.om_hit) == 32
    assert C.sizeof(_lib.om_query_params) == 16
    assert _lib.RAY_DTYPE.itemsize == 24 and _lib.HIT_DTYPE.itemsize == 32
    assert _lib.lib.om_abi_version() == 2                      # additions only


def test_hit_dtype_matches_header(om):
    """HIT_DTYPE / RAY_DTYPE and the ctypes structs field by field against the header's typedefs."""
    from raytracingoneweekend_amd import _lib
    ctype = {"float": ("<f4", C.c_float), "uint32_t": ("<u4", C.c_uint32)}

    def fields(name):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S).group(1)
        out = []
        for decl in [d.strip() for d in body.split(";") if d.strip()]:
            typ, rest = decl.split(None, 1)
            for item in [x.strip() for x in rest.split(",")]:
                m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", item)
                out.append((m.group(1), typ, int(m.group(2)) if m.group(2) else 0))
        return out

    for name, dtype, struct in (("om_hit", _lib.HIT_DTYPE, _lib.om_hit), ("om_ray", _lib.RAY_DTYPE, _lib.om_ray),
                                ("om_query_params", None, _lib.om_query_params)):
        hdr = fields(name)
        assert [f[0] for f in struct._fields_] == [h[0] for h in hdr]
        off = 0
        for (fname, ftype), (hname, htyp, hlen) in zip(struct._fields_, hdr):
            want = ctype[htyp][1] * hlen if hlen else ctype[htyp][1]
            assert C.sizeof(ftype) == C.sizeof(want) and getattr(struct, fname).offset == off
            if dtype is not None:
                sub, doff = dtype.fields[hname][:2]
                assert doff == off and sub.base == np.dtype(ctype[htyp][0]) and sub.shape == ((hlen,) if hlen else ())
            off += C.sizeof(want)
        assert off == C.sizeof(struct)
        if dtype is not None:
            assert dtype.names == tuple(h[0] for h in hdr) and dtype.itemsize == off
    assert om.HIT_DTYPE is _lib.HIT_DTYPE
    assert "#define OM_QUERY_BLOCK %d" % _lib.OM_QUERY_BLOCK in _header()


def test_header_lists_the_replaced_interface(om):
    assert re.search(r"om_hit_rays\*\s+FrozenHittableList::hit\s+hits\.rs:270-334", _header())


def test_argument_validation_without_a_ctx(om):
    """What can be checked with no device: a null ctx is OM_ERR_INVALID for both entry points,
    whatever else is passed (the other rows of the header's table need a ctx: tests/test_gpu_query.py)."""
    from raytracingoneweekend_amd import _lib
    L = _lib.lib
    q = _lib.om_query_params(0.001, 100.0, 1024, 0)
    rays = np.zeros(1, dtype=_lib.RAY_DTYPE)
    hits = np.zeros(1, dtype=_lib.HIT_DTYPE)
    assert L.om_hit_rays(None, C.byref(q), rays.ctypes.data, 1, hits.ctypes.data) == _lib.OM_ERR_INVALID
    assert L.om_hit_rays(None, C.byref(q), rays.ctypes.data, 0, hits.ctypes.data) == _lib.OM_ERR_INVALID
    assert L.om_hit_rays(None, None, None, 0, None) == _lib.OM_ERR_INVALID
    assert L.om_hit_rays_device(None, C.byref(q), None, 1, None, None) == _lib.OM_ERR_INVALID
    assert b"null ctx" in L.om_last_error(None)
    assert L.om_query_max_grid(None) == 0
    assert not hits.view(np.uint8).any()                        # nothing was written


def test_object_material_in_id_order(om, oracle):
    """kitchen_sink adds one or two objects of every type, each with its own material, out of type
    order: ids run in the type order of hits.rs:370-371 (spheres, cubes, triangles, planes,
    parallelograms, marched spheres, boxes, tori)."""
    from raytracingoneweekend_amd import _lib
    w, _, _, _ = kitchen_sink(om, oracle)
    L, MET, DIE = _lib.OM_LAMBERTIAN, _lib.OM_METAL, _lib.OM_DIELECTRIC
    F = np.float32
    want = [(L, (0.8, 0.3, 0.3), 0.0, 0.0), (MET, (0.8, 0.8, 0.9), 0.2, 0.0),          # spheres
            (MET, (0.9, 0.6, 0.2), 0.0, 0.0), (DIE, None, 0.0, 1.5),                     # cubes
            (L, (0.2, 0.9, 0.2), 0.0, 0.0),                                              # triangle
            (L, (0.5, 0.5, 0.5), 0.0, 0.0),                                              # plane
            (MET, (0.7, 0.7, 0.7), 0.05, 0.0),                                           # parallelogram
            (L, (0.3, 0.3, 0.9), 0.0, 0.0), (MET, (0.9, 0.9, 0.3), 0.1, 0.0), (DIE, None, 0.0, 1.3)]
    assert sum(w.counts().values()) == len(want)
    for obj, (typ, alb, fuzz, ior) in enumerate(want, start=1):
        m = w.material_of(obj).raw
        assert m.type == typ, obj
        if typ == DIE:
            assert F(m.ior) == F(ior), obj
        else:
            assert tuple(F(x) for x in m.albedo) == tuple(F(x) for x in alb), obj
        if typ == MET:
            assert F(m.fuzz) == F(fuzz), obj
    raw = _lib.om_material()
    for bad in (0, len(want) + 1, 0xFFFFFFFF):
        assert _lib.lib.om_world_object_material(w.handle, bad, C.byref(raw)) == _lib.OM_ERR_INVALID
        with pytest.raises(_lib.OmError):
            w.material_of(bad)
    assert _lib.lib.om_world_object_material(None, 1, C.byref(raw)) == _lib.OM_ERR_INVALID
    assert _lib.lib.om_world_object_material(w.handle, 1, None) == _lib.OM_ERR_INVALID


def test_user_sdf_objects_come_last(om):
    w = om.HittableList.new()
    a, b = om.Material.new_dielectric(1.25), om.Material.new_lambertian((0.25, 0.5, 0.75))
    w += om.MarchedSdf.new(om.m4x4("ID"), [("sphere", 0., 0., 0., 0.5)], a)
    w += om.Sphere.new_with_radius((0., 0., 0.), 1., b)
    assert w.material_of(1).raw.type == b.raw.type and w.material_of(2).raw.type == a.raw.type
    assert w.material_of(2).raw.ior == 1.25


def test_hit_fails_loudly_without_device(om):
    from conftest import gpu_available
    if gpu_available():
        pytest.skip("a HIP device is present")
    from raytracingoneweekend_amd import _lib
    with pytest.raises(_lib.OmError):                           # no frozen world without a device ...
        om.random_scene().freeze().hit((0., 0., 0.), (0., 0., -1.))
    fz = object.__new__(om.FrozenHittableList)                  # ... and a ctx that never came to be
    fz._ctx = C.c_void_p()
    with pytest.raises(_lib.OmError, match="null ctx"):
        fz.hit((0., 0., 0.), (0., 0., -1.))
    with pytest.raises(_lib.OmError):
        fz.hit_rays(np.zeros((3, 6), np.float32))
