"""Front-end scene builders of main.rs, over the mirrored API.

`random_scene` (main.rs:37-100) has two equivalent builders:
  * random_scene(seed)     -> the native builder om_world_random_scene (fast; 10k variant too)
  * random_scene_api(seed) -> the same scene composed through the Python mirror of the
                              reference API (Material / m4x4 / Sphere.new / `world +=`),
                              exactly as main.rs writes it; tests assert both agree bit for bit.
Both draw from om-rng's SplitMix64 host stream in the reference's draw order.
"""
import numpy as np

from . import _lib as L
from ._lib import check, lib
from .api import (Camera, HittableList, Material, MarchedTorus, Parallelogram, Sphere, Triangle, Cube, m4x4)

F = np.float32
PI = F(3.1415926535897932385)  # utils.rs:29

# scene variants
S_TRACED = 0          # random_scene minus the torus block — configs C0/C1/C4
S_FULL = 1            # random_scene exactly as main.rs:37-100 (torus included)


class SplitMix64:
    """om-rng host stream (SplitMix64) (replaces rand::thread_rng, utils.rs:25)."""

    M = (1 << 64) - 1

    def __init__(self, state):
        self.s = state & self.M

    def next_u64(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & self.M
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & self.M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & self.M
        return z ^ (z >> 31)

    def rand(self):                                        # f32::rand  utils.rs:25
        return F(self.next_u64() >> 40) * F(5.9604644775390625e-8)

    def rand_range(self, lo, hi):                          # utils.rs:26
        r = self.rand()
        return r * (F(hi) - F(lo)) + F(lo)


def random_scene(seed=0x5EED, with_torus=False, grid_half=11, extras=True):
    """main.rs:37-100 via the native builder.  grid_half=50 gives the ~10k-sphere variant (config C3)."""
    w = HittableList.new()
    flags = (1 if with_torus else 0) | (0 if extras else 2)
    check(lib.om_world_random_scene(w.handle, int(seed), flags, int(grid_half)))
    return w


def basic_scene():
    """main.rs:103-110."""
    w = HittableList.new()
    check(lib.om_world_basic_scene(w.handle))
    return w


def marched_scene():
    """SDF scene of config C2: marched ground, box, sphere and random_scene's torus."""
    w = HittableList.new()
    check(lib.om_world_marched_scene(w.handle))
    return w


def random_scene_api(seed=0x5EED, with_torus=False, grid_half=11, extras=True):
    """main.rs:37-100 written against the mirrored API, statement for statement."""
    g = SplitMix64(seed)
    world = HittableList.new()
    mat_ground = Material.new_lambertian((0.5, 0.5, 0.5))
    world += Sphere.new_with_radius((0., -1000., 0.), 1000.0, mat_ground)
    for a in range(-grid_half, grid_half):
        af = F(a)
        for b in range(-grid_half, grid_half):
            bf = F(b)
            cx = af + F(0.9) * g.rand()
            cz = bf + F(0.9) * g.rand()
            center = (cx, F(0.2), cz)
            d = [center[0] - F(4.), center[1] - F(0.2), center[2] - F(0.)]
            length = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2], dtype=F)
            if length > F(0.9):
                mat_prob = g.rand()
                if mat_prob < F(0.8):
                    c1 = (g.rand(), g.rand(), g.rand())
                    c2 = (g.rand(), g.rand(), g.rand())
                    sphere_mat = Material.new_lambertian(tuple(c1[i] * c2[i] for i in range(3)))
                elif mat_prob < F(0.95):
                    albedo = (g.rand_range(0.5, 1.), g.rand_range(0.5, 1.), g.rand_range(0.5, 1.))
                    fuzz = g.rand_range(0., 0.5)
                    sphere_mat = Material.new_metal_fuzz(albedo, fuzz)
                else:
                    sphere_mat = Material.new_dielectric(1.5)
                m = m4x4("TR", center) \
                    ^ m4x4("RX", g.rand() * F(2.) * PI) ^ m4x4("RY", g.rand() * F(2.) * PI) ^ m4x4("RZ", g.rand() * F(2.) * PI) \
                    ^ m4x4("SC", g.rand() + F(1.), g.rand() + F(1.), g.rand() + F(1.)) \
                    ^ m4x4("SC", 0.2, 0.2, 0.2)
                world += Sphere.new(m, sphere_mat)
    if with_torus:
        mat = Material.new_dielectric(1.5)
        local_to_world = m4x4("TR", 0., 1., 0.) ^ m4x4("RX", 0.6) ^ m4x4("RZ", F(1.33) * F(2.) * PI)
        world += MarchedTorus.new(local_to_world, (0.5, 0.1, 0.1), mat)
    if extras:
        p1 = (F(7.), F(1.), F(0.))
        p2 = (F(6.), F(1.1), F(0.5))
        p3 = (F(6.), F(1.5), F(0.))
        world += Parallelogram.new3points(p1, p2, p3, Material.new_metal((1., 0.5, 1.)))
        world += Triangle.new3points((p1[0] + F(0.), p1[1] + F(0.5), p1[2] + F(0.)), p2, p3,
                                     Material.new_lambertian((1., 1., 0.)))
        mat = Material.new_metal((0.7, 0.6, 0.5))
        m = m4x4("TR", 4., 1., 0.) ^ m4x4("RX", g.rand() * F(2.) * PI) ^ m4x4("RY", g.rand() * F(2.) * PI) \
            ^ m4x4("RZ", g.rand() * F(2.) * PI)
        world += Cube.new(m, mat)
    return world


# ---------------------------------------------------------------- triangle meshes
# (vertices (V, 3) float32, faces (T, 3) uint32) pairs for HittableList.add_triangles


def icosphere(level=2, center=(0., 0., 0.), radius=1.0):
    """A sphere of 20 * 4**level triangles: the icosahedron, every face split in four `level` times,
    the vertices pushed out to the sphere.  level 2: 162 vertices, 320 faces.  Outward winding."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    verts = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
             (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    verts = [np.asarray(v, dtype=np.float64) / np.linalg.norm(v) for v in verts]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
             (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
             (8, 6, 7), (9, 8, 1)]
    for _ in range(int(level)):
        mid = {}

        def midpoint(a, b):
            key = (a, b) if a < b else (b, a)
            if key not in mid:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]

        split = []
        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            split += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = split
    v = np.asarray(verts, dtype=np.float64) * float(radius) + np.asarray(center, dtype=np.float64)
    return np.ascontiguousarray(v, dtype=np.float32), np.asarray(faces, dtype=np.uint32)


def heightfield(nx, nz, fn, extent=((0., 1.), (0., 1.))):
    """A terrain of nx x nz cells, two triangles each: vertex (i, j) lies at x = x0 + (x1 - x0) i / nx,
    z = z0 + (z1 - z0) j / nz, y = fn(x, z) (fn takes and returns arrays).  Upward winding."""
    (x0, x1), (z0, z1) = extent
    x = (x0 + (x1 - x0) * np.arange(nx + 1, dtype=np.float64) / nx).astype(np.float32)
    z = (z0 + (z1 - z0) * np.arange(nz + 1, dtype=np.float64) / nz).astype(np.float32)
    gx, gz = np.meshgrid(x, z, indexing="ij")
    gy = np.asarray(fn(gx, gz), dtype=np.float32).reshape(gx.shape)
    v = np.stack([gx, gy, gz], axis=-1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nx), np.arange(nz), indexing="ij")
    a = (i * (nz + 1) + j).ravel()                       # (i, j), then (i, j+1), (i+1, j), (i+1, j+1)
    b, c, d = a + 1, a + (nz + 1), a + (nz + 2)
    f = np.stack([np.stack([a, b, c], axis=1), np.stack([c, b, d], axis=1)], axis=1).reshape(-1, 3)
    return np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.uint32)


def load_obj(path):
    """A minimal Wavefront OBJ reader: `v x y z` and `f` lines only.  `a/b/c` corner forms are reduced
    to the vertex index, negative indices count back from the last vertex read so far, polygons are
    fan-triangulated (corners 0, k, k+1); every other line is ignored."""
    verts, faces = [], []
    with open(path, "r", encoding="utf-8", errors="replace") as fh:
        for line in fh:
            tok = line.split("#", 1)[0].split()
            if not tok:
                continue
            if tok[0] == "v" and len(tok) >= 4:
                verts.append([float(tok[1]), float(tok[2]), float(tok[3])])
            elif tok[0] == "f" and len(tok) >= 4:
                idx = []
                for corner in tok[1:]:
                    k = int(corner.split("/", 1)[0])
                    k = k - 1 if k > 0 else len(verts) + k
                    if not 0 <= k < len(verts):
                        raise ValueError(f"{path}: face corner {corner!r} names no vertex read so far")
                    idx.append(k)
                faces += [(idx[0], idx[k], idx[k + 1]) for k in range(1, len(idx) - 1)]
    return (np.asarray(verts, dtype=np.float32).reshape(-1, 3), np.asarray(faces, dtype=np.uint32).reshape(-1, 3))


def default_camera(aspect_ratio):
    """main.rs:136-142: lookfrom (13,2,3), lookat 0, vup +y, vfov 20, aperture 0.1, focus 10."""
    return Camera.new((13., 2., 3.), (0., 0., 0.), (0., 1., 0.), 20., aspect_ratio, 0.1, 10.)
