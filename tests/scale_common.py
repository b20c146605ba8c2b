"""Worlds and ray sets away from the scene scale every other test runs at (coordinates within
+-15, radii >= 0.2, ray origins inside the world or 13 away): tiny primitives, far ray origins,
worlds far from the coordinate origin, near-singular transforms.  Used by
tests/test_scale_conservative.py (CPU) and tests/test_gpu_scale.py.

A world is a list of items, built identically on the product and the oracle side (`build`) and
written for tests/cpp/leaf_boxes.cpp by `dump`:
    ("sphere_radius", center, radius, mat) | ("sphere", l2w 4x4 f32, mat) | ("cube", l2w 4x4 f32, mat) |
    ("tri", p0, p1, p2, mat) | ("para", p0, p1, p2, mat) |
    ("msphere", center, radius, mat) | ("mbox", center, sizes, mat) | ("mtorus", l2w 4x4 f32, sizes, mat)
with mat = (kind, albedo, fuzz, ior).  Transforms are composed in float32 by the product's own
Mat4x4 product and handed to both sides as the same 16 floats.

Worlds (spec): `tiny`, `cluster`, `cluster_a` / `cluster_b` (the cluster translated to FAR_A /
FAR_B), `sliver`, `facets` (the cluster's cubes, triangles and parallelograms alone), `marched` (the
cluster plus three marched objects).  Each holds 20 triangles and
4 parallelograms, so the barycentric primitives are tree leaves (OM_BARY_TREE_MIN = 16).

Ray sets (all float32 with unit directions, numpy default_rng with fixed seeds):
  silhouette(items, D)  for every tree-resident primitive and each of 8 directions e (the six axis
      directions, where the primitive touches its bounding box, and two random ones): the support
      point p of the primitive in direction e, displaced outward by k margins, k uniform in
      [-5, 40], is the target; the origin lies D away from it in a random direction perpendicular to
      e.  For a sphere that is the closed form: impact parameter r + k * margin.  `margin` is the
      inflation the tree builder gives the primitive's box on that axis,
      1e-3 * (1 + extent) + 1e-5 * max|coord| (for a random e: the largest of the three).
  pinhole(om, items, D) the centre rays of a 24 x 16 frame of a camera D away from the world's
      centre, field of view chosen so that the world fills the frame.
  inside(items)         300 rays from random points of the world's bounds, random directions.
"""
import struct

import numpy as np

F = np.float32
D64 = np.float64

LAM = lambda c: ("lambertian", c, 0.0, 0.0)
MET = lambda c, f: ("metal", c, f, 0.0)
DIE = lambda i: ("dielectric", (0., 0., 0.), 0.0, i)
PALETTE = [LAM((0.8, 0.3, 0.2)), MET((0.7, 0.8, 0.9), 0.1), DIE(1.5), LAM((0.1, 0.6, 0.2)), MET((0.9, 0.6, 0.3), 0.4)]

FAR_A = (3.0e4, 0.0, -2.0e4)      # a half-precision plane has ulp 16 here
FAR_B = (1.0e5, 50.0, 1.0e5)      # beyond the half range: half_out gives +-inf
DISTANCES = (13.0, 1e2, 1e3, 1e4, 1e5)
KHUGE = 100.0                      # om_bvh.cpp: a bound with an extent above 2 * kHuge stays outside the trees
SPHERE_REACH = 16.0                # om_tuning.h OM_SPHERE_REACH: so does a sphere whose margin cannot cover its test's rounding from there
SLAB_REACH = 8192.0                # om_tuning.h OM_SLAB_REACH: a query ray beyond the slab test's reach takes the reference loop
U = 2.0 ** -24
K_LO, K_HI = -5.0, 40.0            # the silhouette band, in inflation margins
PW, PH = 24, 16                    # pinhole frame
VIEW_DIR = np.array([13., 2., 3.]) / np.linalg.norm([13., 2., 3.])   # the default camera's direction


def _icosahedron(center, radius):
    from raytracingoneweekend_amd.scenes import icosphere
    v, f = icosphere(0, (0., 0., 0.), 1.0)
    return (v.astype(D64) * radius + np.asarray(center, D64)).astype(F), f


def _tr(om, c):
    return om.m4x4("TR", float(c[0]), float(c[1]), float(c[2]))


def _bary_items(om, rng, center, radius, spread, edge, n_mat):
    """a 20-triangle icosahedron of `radius` and 4 parallelograms of edge `edge`, around `center`"""
    items = []
    c = np.asarray(center, D64)
    v, f = _icosahedron(c + np.array([0.6, 0.3, -0.5]) * spread, radius)
    for k, (a, b, d) in enumerate(f):
        items.append(("tri", v[a], v[b], v[d], PALETTE[(n_mat + k) % 5]))
    for k in range(4):
        o = c + (rng.random(3) - 0.5) * 2.0 * spread
        u = rng.standard_normal(3); u /= np.linalg.norm(u)
        w = rng.standard_normal(3); w -= u * (u @ w); w /= np.linalg.norm(w)
        w = w + 0.3 * u
        items.append(("para", o.astype(F), (o + u * edge).astype(F), (o + w * edge).astype(F), PALETTE[(n_mat + k) % 5]))
    return items


def _tiny(om):
    """Ground + 24 spheres of radius 1e-3 .. 1e-2, 12 of radius 1e-2 .. 0.2 on a ring around them, 8 cubes of length 2e-3 .. 2e-2 (every other one
    rotated), an icosahedron of radius 5e-3 and 4 parallelograms of edge 5e-3, all within 0.08 of (0, 1, 0)."""
    rng = np.random.default_rng(20261101)
    items = [("sphere_radius", (0., -1000., 0.), 1000., LAM((0.5, 0.5, 0.5)))]
    c0 = np.array([0., 1., 0.])
    radii = np.logspace(-3, -2, 24)
    for k, r in enumerate(radii):
        g = np.array([k % 4 - 1.5, (k // 4) % 3 - 1.0, k // 12 - 0.5]) * 0.035 + (rng.random(3) - 0.5) * 0.01
        c = (c0 + g).astype(F)
        items.append(("sphere_radius", tuple(float(x) for x in c), float(F(r)), PALETTE[k % 5]))
    for k, ln in enumerate(np.logspace(np.log10(2e-3), np.log10(2e-2), 8)):
        c = c0 + np.array([(k % 4 - 1.5) * 0.04, 0.06, (k // 4 - 0.5) * 0.05])
        m = _tr(om, c)
        if k % 2:
            m = m ^ om.m4x4("RY", 0.3 + 0.4 * k) ^ om.m4x4("RX", 0.2 * k)
        m = m ^ om.m4x4("SC", float(ln), float(ln), float(ln))
        items.append(("cube", m.to_numpy(), PALETTE[(k + 2) % 5]))
    # radii from 1e-2 to 0.2, on both sides of the radius (about 0.1) below which a sphere leaves the trees:
    # on a ring of radius 1.2 around the small ones, every other one a little higher
    for k, r in enumerate(np.logspace(-2, np.log10(0.2), 12)):
        a = 2.0 * np.pi * k / 12.0
        c = (c0 + np.array([1.2 * np.cos(a), 0.15 * (k % 2), 1.2 * np.sin(a)])).astype(F)
        items.append(("sphere_radius", tuple(float(x) for x in c), float(F(r)), PALETTE[(k + 1) % 5]))
    return items + _bary_items(om, rng, c0 + np.array([0., -0.05, 0.]), 5e-3, 0.05, 5e-3, 1)


def _cluster(om, at=(0., 0., 0.)):
    """40 spheres with r in [0.2, 1] (every third a rotated ellipsoid, anisotropy up to 10:1), 8 rotated
    cubes, an icosahedron and 4 parallelograms within 5 units of `at`."""
    rng = np.random.default_rng(20261102)
    at = np.asarray(at, D64)
    items = []

    def place(rmax):
        p = rng.standard_normal(3)
        return at + p / np.linalg.norm(p) * (5.0 - rmax) * rng.random() ** (1.0 / 3.0)

    for k in range(40):
        r = 0.2 + 0.8 * rng.random()
        c = place(r)
        ang = rng.random(3) * 6.2831855
        aniso = 1.0 + 9.0 * rng.random(2)
        if k % 3 == 2:
            m = _tr(om, c) ^ om.m4x4("RX", float(ang[0])) ^ om.m4x4("RY", float(ang[1])) ^ om.m4x4("RZ", float(ang[2])) \
                ^ om.m4x4("SC", float(r), float(r / aniso[0]), float(r / aniso[1]))
        else:
            m = _tr(om, c) ^ om.m4x4("SC", float(r), float(r), float(r))
        items.append(("sphere", m.to_numpy(), PALETTE[k % 5]))
    for k in range(8):
        s = 0.3 + 0.7 * rng.random(3)
        c = place(1.0)
        ang = rng.random(3) * 6.2831855
        m = _tr(om, c) ^ om.m4x4("RX", float(ang[0])) ^ om.m4x4("RY", float(ang[1])) ^ om.m4x4("RZ", float(ang[2])) \
            ^ om.m4x4("SC", float(s[0]), float(s[1]), float(s[2]))
        items.append(("cube", m.to_numpy(), PALETTE[(k + 1) % 5]))
    return items + _bary_items(om, rng, at, 0.8, 3.0, 0.9, 3)


def _sliver(om):
    """Near-singular transforms: ellipsoids scaled (1, 1e-3, 1) and (5, 5, 1e-4) under rotations, cubes with
    one side of 1e-4, needle triangles (one edge 1e-3 of the other) and parallelograms."""
    rng = np.random.default_rng(20261103)
    items = []
    for k in range(8):
        c = (rng.random(3) - 0.5) * 12.0
        ang = 0.3 + rng.random(3) * 5.0
        sc = (1.0, 1e-3, 1.0) if k % 2 == 0 else (5.0, 5.0, 1e-4)
        m = _tr(om, c) ^ om.m4x4("RX", float(ang[0])) ^ om.m4x4("RY", float(ang[1])) ^ om.m4x4("RZ", float(ang[2])) \
            ^ om.m4x4("SC", *[float(x) for x in sc])
        items.append(("sphere", m.to_numpy(), PALETTE[k % 5]))
    for k in range(6):
        c = (rng.random(3) - 0.5) * 12.0
        ang = 0.3 + rng.random(3) * 5.0
        sc = [1.0 + rng.random(), 1.0 + rng.random(), 1.0 + rng.random()]
        sc[k % 3] = 1e-4
        m = _tr(om, c) ^ om.m4x4("RZ", float(ang[0])) ^ om.m4x4("RX", float(ang[1])) ^ om.m4x4("SC", *[float(x) for x in sc])
        items.append(("cube", m.to_numpy(), PALETTE[(k + 1) % 5]))
    for k in range(20):
        o = (rng.random(3) - 0.5) * 12.0
        u = rng.standard_normal(3); u /= np.linalg.norm(u)
        w = rng.standard_normal(3); w -= u * (u @ w); w /= np.linalg.norm(w)
        items.append(("tri", o.astype(F), (o + u * 3.0).astype(F), (o + u * 1.5 + w * 3e-3).astype(F), PALETTE[k % 5]))
    for k in range(4):
        o = (rng.random(3) - 0.5) * 12.0
        u = rng.standard_normal(3); u /= np.linalg.norm(u)
        w = rng.standard_normal(3); w -= u * (u @ w); w /= np.linalg.norm(w)
        items.append(("para", o.astype(F), (o + u * 2.0).astype(F), (o + w * 2e-3).astype(F), PALETTE[(k + 2) % 5]))
    return items


def spec(om, name):
    if name == "tiny":
        return _tiny(om)
    if name == "cluster":
        return _cluster(om)
    if name == "cluster_a":
        return _cluster(om, FAR_A)
    if name == "cluster_b":
        return _cluster(om, FAR_B)
    if name == "sliver":
        return _sliver(om)
    if name == "facets":
        # the cluster without its spheres: from D = 1e4 on Sphere::hit accepts nearly every ray of the
        # band and its winners hide what the cube and barycentric tests do out there
        return [it for it in _cluster(om) if it[0] != "sphere"]
    if name == "marched":
        tor = om.m4x4("TR", -2.5, 2.0, 1.0) ^ om.m4x4("RX", 0.8)
        return _cluster(om) + [("msphere", (3.0, -2.0, 2.5), 0.8, LAM((0.3, 0.3, 0.9))),
                               ("mbox", (-3.0, -2.5, -2.0), (0.6, 0.5, 0.7), MET((0.9, 0.9, 0.3), 0.1)),
                               ("mtorus", tor.to_numpy(), (0.9, 0.25, 0.25), DIE(1.3))]
    raise KeyError(name)


def items_of(ow):
    """The traced primitives of an oracle world as items (transforms and points as the world holds
    them; one grey material): the geometry of a world that a scene builder made, here g17."""
    n = ow.counts()
    grey = LAM((0.5, 0.5, 0.5))
    items = [("sphere", ow.affine(0, i)[:16].reshape(4, 4), grey) for i in range(n[0])]
    items += [("cube", ow.affine(1, i)[:16].reshape(4, 4), grey) for i in range(n[1])]
    for kind, cnt, flag in (("tri", n[2], 1), ("para", n[4], 0)):
        for i in range(cnt):
            b = ow.bary(flag, i)
            o = b[0:3]
            items.append((kind, o, (o + b[3:6] * b[6]).astype(F), (o + b[7:10] * b[10]).astype(F), grey))
    assert n[3] == 0, "planes sit between the triangles and the parallelograms in the global index"
    return items


# g17: random_scene(0x5EED, grid_half=17), the first BVH2 read through L2 with half-precision node
# planes (tests/test_tree_regimes.py test_first_l2_tree_has_direct_codes); the far sets aim at every
# 12th of its ~1200 tree primitives
L2_WORLD, L2_EVERY = "g17", 12
WORLDS = ["tiny", "cluster", "cluster_a", "cluster_b", "sliver", "facets"]
FAR = (1e3, 1e4, 1e5)
WORLD_DISTANCES = {"tiny": (13.0,), "cluster": DISTANCES, "cluster_a": DISTANCES, "cluster_b": DISTANCES, "sliver": DISTANCES,
                   "facets": DISTANCES, L2_WORLD: FAR}


def world(om, O, name):
    """-> (items, product world, oracle world)"""
    if name == L2_WORLD:
        from scenes_common import REGIME_WORLDS
        w, ow = REGIME_WORLDS[name][0](om, O)
        return items_of(ow), w, ow
    items = spec(om, name)
    return (items,) + build(om, O, items)


def _mats(om, O, m):
    kind, alb, fuzz, ior = m
    if kind == "lambertian":
        return om.Material.new_lambertian(alb), O.material(kind, alb)
    if kind == "metal":
        return om.Material.new_metal_fuzz(alb, fuzz), O.material(kind, alb, fuzz=fuzz)
    return om.Material.new_dielectric(ior), O.material(kind, ior=ior)


def build(om, O, items):
    """-> (product HittableList, oracle World) of the same items in the same order."""
    w, ow = om.HittableList.new(), O.World()
    for it in items:
        m, m_ = _mats(om, O, it[-1])
        k = it[0]
        if k == "sphere_radius":
            w += om.Sphere.new_with_radius(it[1], it[2], m); ow.add_sphere_radius(it[1], it[2], m_)
        elif k == "sphere":
            w += om.Sphere.new(om.Mat4x4(it[1].ravel()), m); ow.add_sphere(it[1], m_)
        elif k == "cube":
            w += om.Cube.new(om.Mat4x4(it[1].ravel()), m); ow.add_cube(it[1], m_)
        elif k == "tri":
            w += om.Triangle.new3points(it[1], it[2], it[3], m); ow.add_triangle(it[1], it[2], it[3], m_)
        elif k == "para":
            w += om.Parallelogram.new3points(it[1], it[2], it[3], m); ow.add_parallelogram(it[1], it[2], it[3], m_)
        elif k == "msphere":
            w += om.MarchedSphere(it[1], it[2], m); ow.add_marched_sphere(it[1], it[2], m_)
        elif k == "mbox":
            w += om.MarchedBox(it[1], it[2], m); ow.add_marched_box(it[1], it[2], m_)
        elif k == "mtorus":
            w += om.MarchedTorus.new(om.Mat4x4(it[1].ravel()), it[2], m); ow.add_marched_torus(it[1], it[2], m_)
        else:
            raise KeyError(k)
    return w, ow


def dump(items, path):
    """The traced geometry for tests/cpp/leaf_boxes.cpp: u32 item count, then per item a u32 tag
    (1 sphere_radius: 4 f32; 2 sphere, 3 cube: 16 f32; 5 triangle, 6 parallelogram: 9 f32)."""
    traced = [it for it in items if it[0] in ("sphere_radius", "sphere", "cube", "tri", "para")]
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(traced)))
        for it in traced:
            if it[0] == "sphere_radius":
                fh.write(struct.pack("<I4f", 1, *it[1], it[2]))
            elif it[0] in ("sphere", "cube"):
                fh.write(struct.pack("<I", 2 if it[0] == "sphere" else 3) + np.asarray(it[1], dtype="<f4").tobytes())
            else:
                pts = np.concatenate([np.asarray(p, dtype="<f4") for p in it[1:4]])
                fh.write(struct.pack("<I", 5 if it[0] == "tri" else 6) + pts.tobytes())


# ------------------------------------------------------------------ primitives in float64
class Prim:
    """A traced primitive with a bound: its global index gi (type order: spheres, cubes, triangles,
    parallelograms; obj id = gi + 1), its un-inflated bound lo / hi as om_bvh.cpp computes it, the
    builder's inflation margin per axis, and its support point in a direction."""

    def __init__(self, kind, gi, A=None, c=None, pts=None):
        self.kind, self.gi = kind, gi
        if kind in ("sphere", "cube"):
            self.A, self.c = np.asarray(A, D64), np.asarray(c, D64)
            h = np.sqrt((self.A ** 2).sum(axis=1)) if kind == "sphere" else 0.5 * np.abs(self.A).sum(axis=1)
            self.lo, self.hi = self.c - h, self.c + h
        else:
            self.pts = np.asarray(pts, D64)
            self.lo, self.hi = self.pts.min(axis=0), self.pts.max(axis=0)
        mag = max(np.abs(self.lo).max(), np.abs(self.hi).max())
        self.margin = 1e-3 * (1.0 + (self.hi - self.lo)) + 1e-5 * mag

    @property
    def bounded(self):
        """in the trees of the parent commit (every bound that is not huge): what the ray sets aim at and
        what the discriminating count is taken over, whatever the build under test keeps in its trees"""
        return bool((self.hi - self.lo + 2.0 * self.margin).max() <= 2.0 * KHUGE)

    @property
    def in_tree(self):
        """in the trees of this build: bounded, and no thin sphere (om_bvh.cpp thin_sphere: the worst case of
        the test's rounding from SPHERE_REACH away, 8 u D^2 rmax / rmin^2, passes the smallest margin it gets)"""
        return self.bounded and not self.thin

    @property
    def thin(self):
        if self.kind != "sphere":
            return False
        sv = np.linalg.svd(self.A, compute_uv=False)
        h = 0.5 * (self.hi - self.lo)
        mag = max(np.abs(self.lo).max(), np.abs(self.hi).max())
        margin = min(1e-3 * (1.0 + sv.max()) + 1e-5 * np.linalg.norm(self.c), (1e-3 * (1.0 + 2.0 * h) + 1e-5 * mag).min())
        return bool(8.0 * U * SPHERE_REACH ** 2 * sv.max() / sv.min() ** 2 > margin)

    def support(self, e):
        if self.kind == "sphere":
            g = self.A.T @ e
            return self.c + self.A @ g / np.linalg.norm(g)
        if self.kind == "cube":
            return self.c + self.A @ (0.5 * np.sign(self.A.T @ e))
        return self.pts[np.argmax(self.pts @ e)]


def prims(items):
    """The bounded traced primitives of a world, in global-index order."""
    out = {"sphere": [], "cube": [], "tri": [], "para": []}
    for it in items:
        k = it[0]
        if k == "sphere_radius":
            out["sphere"].append(("sphere", np.eye(3) * float(F(it[2])), np.asarray(it[1], F).astype(D64), None))
        elif k in ("sphere", "cube"):
            m = np.asarray(it[1], F).astype(D64)
            out[k].append((k, m[:3, :3], m[:3, 3], None))
        elif k in ("tri", "para"):
            p = np.stack([np.asarray(x, F).astype(D64) for x in it[1:4]])
            if k == "para":
                p = np.concatenate([p, [p[1] + p[2] - p[0]]])
            out[k].append((k, None, None, p))
    res, gi = [], 0
    for k in ("sphere", "cube", "tri", "para"):          # (no planes in these worlds: they sit between tri and para)
        for kind, A, c, p in out[k]:
            res.append(Prim(kind, gi, A, c, p))
            gi += 1
    return res


def tree_prims(items):
    """the primitives the ray sets aim at: the bounded ones (the tree residents of the parent commit)"""
    return [p for p in prims(items) if p.bounded]


def far_origin(rays, root):
    """om_wavefront.hip far_origin: with d the origin's largest axis distance from the root box (0 inside)
    and R the box's diagonal, 2 sqrt(3) d + R passes SLAB_REACH"""
    o = rays[:, :3].astype(D64)
    d = np.maximum(np.maximum(root[:3] - o, o - root[3:]).max(axis=1), 0.0)
    return 2.0 * np.sqrt(3.0) * d + np.linalg.norm(root[3:] - root[:3]) > SLAB_REACH


def world_ball(items):
    """centre and radius of a ball around the tree-resident primitives"""
    tp = tree_prims(items)
    lo = np.min([p.lo for p in tp], axis=0)
    hi = np.max([p.hi for p in tp], axis=0)
    return 0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo))


# ------------------------------------------------------------------ ray sets
def _unit64(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _pack(o, q):
    """float32 rays from float64 origins towards float64 targets: the origin is rounded first, the
    direction is the unit vector from the ROUNDED origin, rounded once."""
    o32 = np.asarray(o, D64).astype(F)
    d = _unit64(np.asarray(q, D64) - o32.astype(D64)).astype(F)
    return np.ascontiguousarray(np.concatenate([o32, d], axis=1))


def silhouette(items, D, seed=20261110, per_dir=4, only=None):
    """-> (rays (n, 6) f32, gi (n,) of the primitive each ray is aimed at)"""
    rng = np.random.default_rng(seed + int(round(np.log10(D) * 8)))
    axes = [np.eye(3)[i] * s for i in range(3) for s in (1.0, -1.0)]
    org, tgt, who = [], [], []
    tp = tree_prims(items)
    for p in (tp if only is None else [tp[i] for i in only]):
        dirs = axes + list(_unit64(rng.standard_normal((2, 3))))
        for j, e in enumerate(dirs):
            m = p.margin[j // 2] if j < 6 else p.margin.max()
            s = p.support(e)
            for _ in range(per_dir):
                k = K_LO + (K_HI - K_LO) * rng.random()
                q = s + e * k * m
                u = rng.standard_normal(3)
                u = _unit64(u - e * (u @ e))
                org.append(q + D * u); tgt.append(q); who.append(p.gi)
    return _pack(np.array(org), np.array(tgt)), np.array(who, dtype=np.int64)


def far_camera(om, O, items, D, aspect=PW / PH, aperture=0.0):
    """A camera D away from the world's centre along the default camera's direction; the world fills the frame."""
    c, r = world_ball(items)
    frm = tuple(float(x) for x in (c + VIEW_DIR * D).astype(F))
    at = tuple(float(x) for x in c.astype(F))
    fov = float(np.degrees(2.0 * np.arctan(r / D)))
    args = (frm, at, (0., 1., 0.), fov, aspect, aperture, float(D))
    return om.Camera.new(*args), O.camera(*args)


def pinhole(om, O, items, D):
    from scenes_common import pinhole_rays
    cam, _ = far_camera(om, O, items, D)
    return np.ascontiguousarray(pinhole_rays(cam, PW, PH))


def inside(items, n=300, seed=20261120):
    rng = np.random.default_rng(seed)
    c, r = world_ball(items)
    o = c + (rng.random((n, 3)) - 0.5) * 2.0 * r / np.sqrt(3.0)
    return _pack(o, o + _unit64(rng.standard_normal((n, 3))))


def windows(name, D):
    """the two call windows of a far set; the tiny world: the default window"""
    return [(0.001, 100.0)] if name == "tiny" else [(0.001, float("inf")), (0.001, 2.0 * D)]


# rays per (primitive, direction); enlarged where 4 left fewer than 32 discriminating rays
# (tests/test_scale_conservative.py test_sets_discriminate): the cluster at D = 1e2, where the error only
# just passes the margin (28 of 2688 rays with 4), the tiny world, whose band of 40 margins is
# 4 .. 40 radii wide, cluster_b at D = 1e3, whose margin of 1.0 makes the band wider than the world, and
# facets at D = 1e5, where the cube and triangle tests move by 2 margins only
PER_DIR = {("tiny", 13.0): 12, ("cluster", 1e2): 8, ("cluster_b", 1e3): 32, ("facets", 1e5): 80}


def ray_sets(om, O, name, items):
    """{D: (rays, aimed_gi)}: silhouette + pinhole rays per distance (aimed_gi = -1 for the pinhole
    rays); key 0.0: the rays that start inside the world (the control)."""
    out = {}
    only = range(0, len(tree_prims(items)), L2_EVERY) if name == L2_WORLD else None
    for D in WORLD_DISTANCES[name]:
        s, who = silhouette(items, D, per_dir=PER_DIR.get((name, D), 4), only=only)
        p = pinhole(om, O, items, D)
        out[D] = (np.ascontiguousarray(np.concatenate([s, p])), np.concatenate([who, np.full(len(p), -1, np.int64)]))
    ins = inside(items)
    out[0.0] = (ins, np.full(len(ins), -1, np.int64))
    return out


# ------------------------------------------------------------------ float64 geometry of float32 rays
def line_misses_box(rays, lo, hi):
    """The float64 LINE of each float32 ray against the box [lo, hi] (arrays broadcast per ray):
    True where the line does not meet it."""
    o, d = rays[:, :3].astype(D64), rays[:, 3:].astype(D64)
    near, far = slab(o, d, lo, hi)
    return near > far


def slab(o, d, lo, hi):
    """per-ray [near, far] of the float64 line o + t d in the box; a zero direction component
    constrains nothing when the origin is inside the slab and everything otherwise"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    tn, tf = np.minimum(t0, t1), np.maximum(t0, t1)
    zero = d == 0
    ins = (o >= lo) & (o <= hi)
    tn = np.where(zero, np.where(ins, -np.inf, np.inf), tn)
    tf = np.where(zero, np.where(ins, np.inf, -np.inf), tf)
    return tn.max(axis=1), tf.min(axis=1)


_ORACLE = {}


def oracle_answers(om, O, name, key, ow, rays, tmin, tmax):
    """oracle records of a ray set, computed once per process and shared by the test modules"""
    from scenes_common import oracle_hits
    k = (name, key, float(tmin), float(tmax))
    if k not in _ORACLE:
        _ORACLE[k] = oracle_hits(om, ow, rays, tmin, tmax)
        _ORACLE[k].setflags(write=False)
    return _ORACLE[k]


# ------------------------------------------------------------------ the known disagreement
# (world, D) sets at which the culls are still NOT conservative: spheres and ellipsoids of radius
# 0.14 .. 1 seen from 1e2 or 1e3 away.  tests/test_scale_conservative.py finds winners beyond their leaf
# boxes there, and on the device every kernel but `brute` gives other records than the oracle.  The two
# lists agree set for set.  A case of this table is a strict expected failure in both modules, and only
# with the failure pinned below (KnownDisagreement): a fix turns it into an unexpected pass, any other
# breakage into a plain failure.  Gone from the table since thin spheres stay outside the trees and query
# rays beyond the slab test's reach take the reference loop: tiny, every sliver set, every set from D = 1e4 on.
NOT_CONSERVATIVE = {(w, 1e3) for w in ("cluster", "cluster_a", "cluster_b", L2_WORLD)}
# `culled` alone also differs at the cluster's D = 1e2 set (2 of 4992 records): its bounding sphere's margin,
# 1e-3 * (1 + r) + 1e-5 |c|, is smaller than the box's 1e-3 * (1 + 2 r) + 1e-5 |coord|
NOT_CONSERVATIVE_CULLED = NOT_CONSERVATIVE | {("cluster", 1e2)}
XFAIL_REASON = ("the box inflation is absolute, the error of the float32 sphere test grows with D^2 / radius: the culls "
                "skip spheres of radius 0.14 .. 1 that Sphere::hit accepts from 1e2 .. 1e3 away (DESIGN.md §5.3)")


class KnownDisagreement(AssertionError):
    """The one failure an expected-failure case may end with: a cull skipped a primitive that the
    reference loop accepts (CPU: a winner past its box; device: records that lost the oracle's winner
    and nothing else).  Raised only after the test has checked that nothing else is wrong."""


def xfail_known(cond):
    import pytest
    return [pytest.mark.xfail(strict=True, raises=KnownDisagreement, reason=XFAIL_REASON)] if cond else []


def sets_of(name):
    """the distances of a world's sets, the inside rays (0.0) last"""
    return list(WORLD_DISTANCES[name]) + [0.0]
