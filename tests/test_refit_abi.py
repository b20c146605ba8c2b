"""om_world_update_triangles and the statuses of om_update_triangles* (include/ottomarcher.h), on the
CPU where no ctx is needed; the statuses that need one (OM_ERR_STATE before an upload, the range of
the uploaded world) are the GPU-marked test at the end."""
import ctypes as C

import numpy as np
import pytest

import mesh_common as MC
import refit_common as RC

F = np.float32
K_TRI = 2


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _world(om, v, f, extra=True):
    w = om.HittableList.new()
    if extra:
        w += om.Triangle.new3points((5., 0., 0.), (6., 0., 0.), (5., 1., 0.), om.Material.new_metal((0.9, 0.9, 0.9)))
    w.add_triangles(v, f, om.Material.new_lambertian((0.2, 0.4, 0.9)))
    return w


def _triangles(w):
    return np.stack([w.export(K_TRI, i, 29) for i in range(w.counts()["triangles"])])


def test_update_equals_a_world_built_from_the_new_vertices(om):
    v, f = MC.icosphere(2, (0., 1., 0.), 1.0)
    nv = RC.deform_ico(v)
    w, want = _world(om, v, f), _world(om, nv, f)
    before = _triangles(w)
    w.update_triangles(nv, f, first=1)                    # triangle 0 was added one by one: it stays
    got = _triangles(w)
    assert got.tobytes() == _triangles(want).tobytes()
    assert got[0].tobytes() == before[0].tobytes() and (got[1:] != before[1:]).any(axis=1).all()
    assert w.material_of(1).mat_type == om.Material.new_metal((0.9, 0.9, 0.9)).mat_type and w.material_of(2).mat_type == om.Material.new_lambertian((0., 0., 0.)).mat_type, "materials stay"
    # a partial range, and without indices: triangle k from vertices 3k, 3k + 1, 3k + 2
    w2 = _world(om, v, f)
    w2.update_triangles(np.ascontiguousarray(nv[f[10:20]].reshape(-1, 3)), first=11)
    got2 = _triangles(w2)
    assert got2[11:21].tobytes() == got[11:21].tobytes() and got2[:11].tobytes() == before[:11].tobytes()
    assert got2[21:].tobytes() == before[21:].tobytes()


def test_statuses_and_all_or_nothing(om):
    from raytracingoneweekend_amd import _lib as L
    lib = L.lib
    v, f = MC.icosphere(2, (0., 1., 0.), 1.0)
    nv = RC.deform_ico(v)
    w = _world(om, v, f, extra=False)
    before = _triangles(w)
    n = len(f)
    up = lambda first, vp, nvert, ip, nt: lib.om_world_update_triangles(w.handle, first, vp, nvert, ip, nt)
    assert up(0, _ptr(nv), len(nv), _ptr(f), 0) == L.OM_OK and up(n, None, 0, None, 0) == L.OM_OK, "n_tri == 0"
    assert lib.om_world_update_triangles(None, 0, _ptr(nv), len(nv), _ptr(f), n) == L.OM_ERR_INVALID
    assert up(0, None, len(nv), _ptr(f), n) == L.OM_ERR_INVALID, "null vertices with work to do"
    assert up(1, _ptr(nv), len(nv), _ptr(f), n) == L.OM_ERR_INVALID and up(n + 1, _ptr(nv), len(nv), _ptr(f), 0) == L.OM_ERR_INVALID, \
        "a range past the world's triangles"
    assert up(0, _ptr(nv), 5, None, 2) == L.OM_ERR_INVALID, "without indices triangle k needs vertex 3k + 2"
    bad = f.copy()
    bad[n - 1, 2] = len(nv)
    assert up(0, _ptr(nv), len(nv), _ptr(bad), n) == L.OM_ERR_INVALID
    assert _triangles(w).tobytes() == before.tobytes(), "a failed call writes nothing"
    with pytest.raises(om._lib.OmError):
        w.update_triangles(nv, bad)
    with pytest.raises(ValueError):
        w.update_triangles(nv.astype(np.float64), f)
    # the ctx forms without a ctx
    assert lib.om_update_triangles(None, 0, _ptr(nv), len(nv), _ptr(f), n) == L.OM_ERR_INVALID
    assert lib.om_update_triangles_device(None, 0, _ptr(nv), len(nv), _ptr(f), n, None) == L.OM_ERR_INVALID
    u = L.om_update_info()
    assert lib.om_get_update_info(None, C.byref(u)) == L.OM_ERR_INVALID
    assert C.sizeof(L.om_update_info) == 16 and lib.om_abi_version() == 2


@pytest.mark.gpu
def test_ctx_statuses(om):
    from raytracingoneweekend_amd import _lib as L
    lib = L.lib
    v, f = MC.icosphere(2, (0., 1., 0.), 1.0)
    n = len(f)
    ctx = C.c_void_p()
    L.check(lib.om_create(0, C.byref(ctx)))
    try:
        u = L.om_update_info()
        assert lib.om_update_triangles(ctx, 0, _ptr(v), len(v), _ptr(f), n) == L.OM_ERR_STATE, "before om_upload_world"
        assert lib.om_update_triangles_device(ctx, 0, _ptr(v), len(v), _ptr(f), n, None) == L.OM_ERR_STATE
        assert lib.om_get_update_info(ctx, C.byref(u)) == L.OM_ERR_STATE
        w = _world(om, v, f, extra=False)
        L.check(lib.om_upload_world(ctx, w.handle), ctx)
        assert lib.om_update_triangles(ctx, 0, _ptr(v), len(v), _ptr(f), 0) == L.OM_OK, "n_tri == 0 launches nothing"
        assert lib.om_update_triangles(ctx, 1, _ptr(v), len(v), _ptr(f), n) == L.OM_ERR_INVALID, "past the world's triangles"
        assert lib.om_update_triangles(ctx, 0, None, len(v), _ptr(f), n) == L.OM_ERR_INVALID
        assert lib.om_get_update_info(ctx, None) == L.OM_ERR_INVALID
        L.check(lib.om_get_update_info(ctx, C.byref(u)), ctx)
        assert (u.updates, u.triangles, u.unbounded, u.skipped) == (0, 0, 0, 0)
        # a world without triangles has nothing to move
        s = om.HittableList.new()
        s += om.Sphere.new_with_radius((0., 0., 0.), 1.0, om.Material.new_lambertian((0.5, 0.5, 0.5)))
        L.check(lib.om_upload_world(ctx, s.handle), ctx)
        assert lib.om_update_triangles(ctx, 0, _ptr(v), len(v), _ptr(f), 1) == L.OM_ERR_INVALID
        assert lib.om_update_triangles(ctx, 0, _ptr(v), len(v), _ptr(f), 0) == L.OM_OK
    finally:
        lib.om_destroy(ctx)
