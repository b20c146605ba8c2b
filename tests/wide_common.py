"""Worlds of the wide-BVH2 tests (test_wide_regimes.py, test_gpu_wide.py): mesh_common's base (ground,
three ellipsoids, one cube) plus an n x n-cell smooth heightfield of 2 n^2 triangles over [-3, 3]^2,
sized around the limits of the compressed BVH2's 16-bit child codes:

  W15    n = 227: 103 058 triangles, the largest n whose max-leaf tree still fits the 15-bit codes
         (32 682 nodes, 32 683 leaves): read through L2 as before, wide nodes emitted too
  W15P   n = 228: 103 968 triangles, the smallest n past them: the wide regime
  W16P   n = 330: 217 800 triangles, more than 65 536 nodes and records: a u16 stack entry or a
         16-bit record index would truncate

The n are pinned from tests/cpp/wide_regimes' report (tests/test_wide_regimes.py asserts the regime of
each, so a builder change that moves a limit fails there by name).
"""
import numpy as np

import mesh_common as MC

F = np.float32
N = {"W15": 227, "W15P": 228, "W16P": 330}


def smooth_height(x, z):
    """float32 in, float32 out: y = 0.3 sin(2.1 x) cos(1.7 z) + 1, no flat part"""
    x, z = x.astype(F), z.astype(F)
    return (F(0.3) * np.sin(F(2.1) * x, dtype=F) * np.cos(F(1.7) * z, dtype=F) + F(1.0)).astype(F)


def field(n):
    from raytracingoneweekend_amd.scenes import heightfield
    return heightfield(n, n, smooth_height, extent=((-3., 3.), (-3., 3.)))


def spec_n(om, n):
    v, f = field(n)
    return MC._base(om) + [("mesh", v, f, MC.LAM((0.3, 0.7, 0.3)))]


def spec(om, name):
    return spec_n(om, N[name])


def build_product(om, items):
    """the product's HittableList alone (the oracle's world takes 1.6 s per 100k faces: the GPU tests
    build it once per world, tests/test_gpu_wide.py)"""
    w = om.HittableList.new()
    for it in items:
        kind, alb, fuzz, ior = it[-1]
        m = (om.Material.new_lambertian(alb) if kind == "lambertian" else
             om.Material.new_metal_fuzz(alb, fuzz) if kind == "metal" else om.Material.new_dielectric(ior))
        if it[0] == "sphere_radius":
            w += om.Sphere.new_with_radius(it[1], it[2], m)
        elif it[0] == "sphere":
            w += om.Sphere.new(om.Mat4x4(it[1].ravel()), m)
        elif it[0] == "cube":
            w += om.Cube.new(om.Mat4x4(it[1].ravel()), m)
        else:
            w.add_triangles(it[1], it[2], m)
    return w
