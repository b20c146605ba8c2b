"""The bulk mesh entry point (om_world_add_triangles, HittableList.add_triangles) and the mesh
builders of scenes.py (CPU only)."""
import ctypes as C

import numpy as np
import pytest

F = np.float32


def _raw(om, w, v, f, mat):
    from raytracingoneweekend_amd import _lib as L
    v = np.ascontiguousarray(v, dtype=F) if v is not None else None
    f = np.ascontiguousarray(f, dtype=np.uint32) if f is not None else None
    return L.lib.om_world_add_triangles(w.handle, v.ctypes.data_as(C.c_void_p) if v is not None else None,
                                        0 if v is None else len(v), f.ctypes.data_as(C.c_void_p) if f is not None else None,
                                        0 if f is None else len(f), C.byref(mat) if mat is not None else None)


def test_bulk_add_equals_one_call_per_face(om):
    v, f = om.icosphere(2, (0.25, 1.0, -0.5), 0.75)
    mat = om.Material.new_metal_fuzz((0.7, 0.8, 0.9), 0.1)
    bulk, single = om.HittableList.new(), om.HittableList.new()
    ground = om.Sphere.new_with_radius((0., -1000., 0.), 1000., om.Material.new_lambertian((0.5, 0.5, 0.5)))
    bulk += ground
    single += ground
    # a triangle ahead of the mesh: the bulk call appends after it, like the single calls
    first = om.Triangle.new3points((0., 0., 0.), (1., 0., 0.), (0., 1., 0.), mat)
    bulk += first
    single += first
    assert bulk.add_triangles(v, f, mat) is bulk
    for a, b, c in f:
        single += om.Triangle.new3points(v[a], v[b], v[c], mat)
    assert bulk.counts() == single.counts() and bulk.counts()["triangles"] == len(f) + 1 == 321
    for k in range(len(f) + 1):
        assert bulk.export(2, k, 29).tobytes() == single.export(2, k, 29).tobytes(), f"triangle {k} differs"
    for obj in (1, 2, 3, 322):
        a, b = bulk.material_of(obj).raw, single.material_of(obj).raw
        assert (a.type, tuple(a.albedo), a.fuzz, a.ior) == (b.type, tuple(b.albedo), b.fuzz, b.ior)


def test_degenerate_triangles_are_accepted_like_new3points(om):
    v = np.array([[0., 0., 0.], [1., 0., 0.], [0., 1., 0.], [np.nan, 0., 0.], [2., 0., 0.]], dtype=F)
    f = np.array([[0, 1, 1], [0, 1, 4], [0, 1, 3], [0, 1, 2]], dtype=np.uint32)   # repeated index, collinear, NaN, good
    mat = om.Material.new_lambertian((0.5, 0.5, 0.5))
    bulk, single = om.HittableList.new(), om.HittableList.new()
    bulk.add_triangles(v, f, mat)
    for a, b, c in f:
        single += om.Triangle.new3points(v[a], v[b], v[c], mat)
    for k in range(len(f)):
        assert bulk.export(2, k, 29).tobytes() == single.export(2, k, 29).tobytes()


def test_bad_index_adds_nothing(om):
    from raytracingoneweekend_amd import _lib as L
    v, f = om.icosphere(1)
    w = om.HittableList.new()
    w.add_triangles(v, f[:5], om.Material.new_lambertian((0.5, 0.5, 0.5)))
    before = w.counts()
    bad = f.copy()
    bad[-1, 2] = len(v)                                     # the last index of the last face: one past the end
    mat = om.Material.new_lambertian((0.5, 0.5, 0.5))
    assert _raw(om, w, v, bad, mat.raw) == L.OM_ERR_INVALID
    assert w.counts() == before
    with pytest.raises(L.OmError):
        w.add_triangles(v, bad, mat)
    assert w.counts() == before


def test_empty_null_and_invalid_material(om):
    from raytracingoneweekend_amd import _lib as L
    v, f = om.icosphere(0)
    w = om.HittableList.new()
    mat = om.Material.new_lambertian((0.5, 0.5, 0.5)).raw
    assert _raw(om, w, v, f[:0], mat) == L.OM_OK                        # n_tri == 0
    assert _raw(om, w, None, None, mat) == L.OM_OK                      # ... with null arrays too
    assert w.counts()["triangles"] == 0
    assert L.lib.om_world_add_triangles(w.handle, None, len(v), f.ctypes.data_as(C.c_void_p), len(f), C.byref(mat)) == L.OM_ERR_INVALID
    assert L.lib.om_world_add_triangles(w.handle, v.ctypes.data_as(C.c_void_p), len(v), None, len(f), C.byref(mat)) == L.OM_ERR_INVALID
    assert L.lib.om_world_add_triangles(None, v.ctypes.data_as(C.c_void_p), len(v), f.ctypes.data_as(C.c_void_p), len(f), C.byref(mat)) == L.OM_ERR_INVALID
    assert _raw(om, w, v, f, None) == L.OM_ERR_INVALID                  # null material
    bad = L.om_material()
    bad.type = 7
    assert _raw(om, w, v, f, bad) == L.OM_ERR_INVALID                   # invalid material
    assert w.counts()["triangles"] == 0
    assert _raw(om, w, v, f, mat) == L.OM_OK and w.counts()["triangles"] == 20


def test_python_argument_checks(om):
    v, f = om.icosphere(0)
    w = om.HittableList.new()
    mat = om.Material.new_lambertian((0.5, 0.5, 0.5))
    with pytest.raises(ValueError):
        w.add_triangles(v.astype(np.float64), f, mat)
    with pytest.raises(ValueError):
        w.add_triangles(v, f.astype(np.int64), mat)
    with pytest.raises(ValueError):
        w.add_triangles(v.reshape(-1), f, mat)
    with pytest.raises(ValueError):
        w.add_triangles(v, f.reshape(-1), mat)
    with pytest.raises(TypeError):
        w.add_triangles(v, f, mat.raw)
    assert w.counts()["triangles"] == 0
    w.add_triangles(v[:, ::1], np.asfortranarray(f), mat)               # any layout: made contiguous
    assert w.counts()["triangles"] == 20


def test_icosphere_sizes(om):
    for level, nv, nf in ((0, 12, 20), (1, 42, 80), (2, 162, 320), (3, 642, 1280)):
        v, f = om.icosphere(level, (1., 2., 3.), 0.5)
        assert v.dtype == np.float32 and f.dtype == np.uint32 and v.shape == (nv, 3) and f.shape == (nf, 3)
        assert int(f.max()) == nv - 1 and len(set(f.reshape(-1).tolist())) == nv
        r = np.linalg.norm(v.astype(np.float64) - np.array([1., 2., 3.]), axis=1)
        assert np.allclose(r, 0.5, atol=1e-6)
        edges = set()
        for a, b, c in f.tolist():                                       # closed, consistently wound: every directed edge once
            for e in ((a, b), (b, c), (c, a)):
                assert e not in edges
                edges.add(e)
        assert all((b, a) in edges for a, b in edges) and len(edges) == 3 * nf
        n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        assert (np.einsum("ij,ij->i", n, v[f[:, 0]] - np.array([1., 2., 3.], dtype=F)) > 0).all(), "outward winding"


def test_heightfield(om):
    v, f = om.heightfield(3, 2, lambda x, z: x + 10 * z, extent=((0., 3.), (0., 1.)))
    assert v.dtype == np.float32 and f.dtype == np.uint32 and v.shape == (12, 3) and f.shape == (12, 3)
    assert np.array_equal(v[:, 1], v[:, 0] + 10 * v[:, 2])
    assert v[:, 0].min() == 0 and v[:, 0].max() == 3 and v[:, 2].max() == 1
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert np.isclose(0.5 * n[:, 1].sum(), 3.0) and (n[:, 1] > 0).all(), "the cells tile the extent, wound upward"


def test_load_obj(om, tmp_path):
    p = tmp_path / "quad.obj"
    p.write_text("# a quad, a triangle by negative indices, v/vt/vn corners\n"
                 "mtllib none.mtl\no thing\n"
                 "v 0 0 0\nv 1 0 0   # trailing comment\nv 1 1 0\nv 0 1 0\n"
                 "vt 0 0\nvn 0 0 1\n"
                 "f 1 2 3 4\n"
                 "v 0.5 0.5 1 1.0\n"
                 "f -1 -5 -4\n"
                 "f 1/1/1 2/1/1 5/1/1\nf 2//1 3//1 5//1\nf 3/1 4/1 5/1\n"
                 "s off\nusemtl m\nl 1 2\n")
    v, f = om.load_obj(str(p))
    assert v.dtype == np.float32 and f.dtype == np.uint32
    assert v.tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1]]
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [4, 0, 1], [0, 1, 4], [1, 2, 4], [2, 3, 4]]
    w = om.HittableList.new()
    w.add_triangles(v, f, om.Material.new_lambertian((0.5, 0.5, 0.5)))
    assert w.counts()["triangles"] == 6
    bad = tmp_path / "bad.obj"
    bad.write_text("v 0 0 0\nf 1 2 3\n")
    with pytest.raises(ValueError):
        om.load_obj(str(bad))
    empty = tmp_path / "empty.obj"
    empty.write_text("# nothing\n")
    v, f = om.load_obj(str(empty))
    assert v.shape == (0, 3) and f.shape == (0, 3)
