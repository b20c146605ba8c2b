"""The moved meshes of the refit tests (test_refit_host.py, test_refit_abi.py, test_gpu_refit.py):
the worlds of tests/mesh_common.py with the vertices of one mesh displaced, in numpy float32, the
same arrays to every side (update_triangles, a world built from the new vertices, the oracle).

  ico2 family (ico2, ico2x2, below, degen): v' = c + (v - c) * 1.25 * (1 + 0.2 sin(3x + 1) cos(2z))
          + (0.35, 0.15, -0.25), c = (0, 1, 0), every operation in float32, left to right
  hf48    the height function of mesh_common.hf_height with its sine's phase advanced by 1.7

`first` is the first triangle (of the triangle kind) of the moved mesh: the last mesh of the world.
"""
import numpy as np

import mesh_common as MC

F = np.float32
WORLDS = ["ico2", "hf48", "below", "degen", "ico2x2"]


def deform_ico(v):
    v = np.ascontiguousarray(v, dtype=F)
    c = np.array([0., 1., 0.], dtype=F)
    s = (F(1.0) + F(0.2) * np.sin(F(3.0) * v[:, 0] + F(1.0), dtype=F) * np.cos(F(2.0) * v[:, 2], dtype=F)).astype(F)
    k = (F(1.25) * s).astype(F)
    out = (c + (v - c) * k[:, None]).astype(F) + np.array([0.35, 0.15, -0.25], dtype=F)
    return np.ascontiguousarray(out.astype(F))


def hf_height_moved(x, z):
    x, z = x.astype(F), z.astype(F)
    h = (F(0.45) * np.sin(F(1.3) * x + F(1.7), dtype=F) * np.cos(F(1.1) * z, dtype=F) - F(0.05)).astype(F)
    return np.maximum(h, F(0.0)).astype(F)


def moved_vertices(name, v):
    """the displaced vertices of world `name`'s mesh"""
    if name == "hf48":
        return np.ascontiguousarray(np.stack([v[:, 0], hf_height_moved(v[:, 0], v[:, 2]), v[:, 2]], axis=1).astype(F))
    return deform_ico(v)


def first_triangle(items):
    """index, among the world's triangles, of the first triangle of its last mesh"""
    meshes = [it for it in items if it[0] == "mesh"]
    return sum(len(m[2]) for m in meshes[:-1])


def moved_spec(om, name):
    """-> (items of the original world, items with the last mesh moved, first, new vertices, faces)"""
    items = MC.spec(om, name)
    k = max(i for i, it in enumerate(items) if it[0] == "mesh")
    _, v, f, m = items[k]
    nv = moved_vertices(name, v)
    moved = list(items)
    moved[k] = ("mesh", nv, f, m)
    return items, moved, first_triangle(items), nv, f
