"""Python mirror of the reference's scene/render API, driving the HIP hot path.

Names and argument meaning follow the Rust sources so a front-end reads the same:

    world = HittableList.new()
    world += Sphere.new_with_radius((0., -1000., 0.), 1000., Material.new_lambertian((0.5, 0.5, 0.5)))
    m = m4x4("TR", center) ^ m4x4("RX", a) ^ m4x4("SC", 0.2, 0.2, 0.2)       # main.rs:65-68
    world += Sphere.new(m, mat)
    camera = Camera.new(lookfrom, lookat, vup, 20., 3/2, 0.1, 10.)           # camera.rs:38
    frozen = world.freeze(camera)                                             # hits.rs:87-89
    pixels = PixelsBox.new(W * H)                                             # render_thread.rs:53-65
    render(camera, frozen, max_depth, 0.001, 100., spp, W, H, pixels)         # render_thread.rs:145

All arithmetic happens in libottomarcher.so (host f32 builders + HIP kernels);
this module only marshals arguments.
"""
import contextlib
import ctypes as C

import numpy as np

from . import _lib as L
from ._lib import check, f3, fptr, lib

__all__ = [
    "Material", "Mat4x4", "m4x4", "Camera", "Sphere", "Cube", "Triangle", "Parallelogram", "InfinitePlane",
    "MarchedSphere", "MarchedBox", "MarchedTorus", "MarchedSdf", "HittableList", "FrozenHittableList", "PixelsBox", "render",
    "RenderStats", "HitRecord", "HIT_DTYPE", "RAY_DTYPE", "WINDOW_DTYPE", "RADIANCE_DTYPE", "path_rng_state",
]

HIT_DTYPE = L.HIT_DTYPE     # om_hit: t, point, normal, obj (hits.rs:11-17)
RAY_DTYPE = L.RAY_DTYPE     # om_ray: orig, dir (ray.rs:5-8)
WINDOW_DTYPE = L.WINDOW_DTYPE   # om_ray_window: tmin, tmax of one ray
RADIANCE_DTYPE = L.RADIANCE_DTYPE   # om_radiance: color, depth, obj (ray_color's triple, render_thread.rs:128-143)


def path_rng_state(seed, pixel, sample, draws=0):
    """State of the om-rng v2 path stream (seed, pixel, sample) after `draws` draws (om_path_rng_state):
    low word the Weyl counter, high word the key.  om_render's sample has drawn 2 + 2 * (lens-disc
    tries) times when ray_color starts."""
    return int(lib.om_path_rng_state(int(seed), int(pixel) & 0xFFFFFFFF, int(sample) & 0xFFFFFFFF, int(draws) & 0xFFFFFFFF))


# ---------------------------------------------------------------- materials.rs
class Material:
    """materials.rs:18-38 — tagged union; constructors mirror Material::new_*."""

    def __init__(self, raw):
        self.raw = raw

    @staticmethod
    def new_lambertian(albedo):
        return Material(lib.om_material_lambertian(*[float(x) for x in albedo]))

    @staticmethod
    def new_metal(albedo):
        return Material(lib.om_material_metal(*[float(x) for x in albedo]))

    @staticmethod
    def new_metal_fuzz(albedo, fuzz):
        return Material(lib.om_material_metal_fuzz(*[float(x) for x in albedo], float(fuzz)))

    @staticmethod
    def new_dielectric(index_of_refraction):
        return Material(lib.om_material_dielectric(float(index_of_refraction)))

    @property
    def mat_type(self):
        return self.raw.type

    def __repr__(self):
        r = self.raw
        return f"Material(type={r.type}, albedo={tuple(r.albedo)}, fuzz={r.fuzz}, ior={r.ior})"


# ---------------------------------------------------------------- math/mat4x4.rs
class Mat4x4:
    """Row-major f32 4x4 (mat4x4.rs:8-10); `a ^ b` is dot_mat (mat4x4.rs:167-178)."""

    def __init__(self, values):
        self.m = L.F16(*[float(x) for x in values])

    @staticmethod
    def _out(fn, *args):
        out = L.F16()
        check(fn(*args, fptr(out)))
        return Mat4x4(list(out))

    @classmethod
    def identity(cls):
        return cls._out(lib.om_mat4_identity)

    @classmethod
    def new_translate(cls, v):
        return cls._out(lib.om_mat4_translate, fptr(f3(v)))

    @classmethod
    def new_scale(cls, v):
        return cls._out(lib.om_mat4_scale, fptr(f3(v)))

    @classmethod
    def new_rotate_x(cls, f):
        return cls._out(lib.om_mat4_rotate, 0, float(f))

    @classmethod
    def new_rotate_y(cls, f):
        return cls._out(lib.om_mat4_rotate, 1, float(f))

    @classmethod
    def new_rotate_z(cls, f):
        return cls._out(lib.om_mat4_rotate, 2, float(f))

    def dot_mat(self, other):
        return Mat4x4._out(lib.om_mat4_mul, fptr(self.m), fptr(other.m))

    def __xor__(self, other):
        return self.dot_mat(other)

    def fast_homogenous_inverse(self):
        return Mat4x4._out(lib.om_mat4_fast_homogenous_inverse, fptr(self.m))

    def to_numpy(self):
        return np.array(list(self.m), dtype=np.float32).reshape(4, 4)


def m4x4(kind="ID", *args):
    """The m4x4! macro (mat4x4.rs:181-209): RX/RY/RZ angle, TR x,y,z | TR v, SC x,y,z | SC v, ID."""
    if kind in ("ID", None):
        return Mat4x4.identity()
    if kind in ("RX", "RY", "RZ"):
        return {"RX": Mat4x4.new_rotate_x, "RY": Mat4x4.new_rotate_y, "RZ": Mat4x4.new_rotate_z}[kind](args[0])
    v = args[0] if len(args) == 1 else args
    if kind == "TR":
        return Mat4x4.new_translate(v)
    if kind == "SC":
        return Mat4x4.new_scale(v)
    raise ValueError(f"m4x4!: unknown kind {kind}")


# ---------------------------------------------------------------- camera.rs
class Camera:
    """camera.rs:10-59."""

    def __init__(self, raw):
        self.raw = raw

    @staticmethod
    def new(lookfrom, lookat, vup, vfov_in_degrees, aspect_ratio, aperture, focus_dist):
        raw = L.om_camera()
        check(lib.om_camera_new(fptr(f3(lookfrom)), fptr(f3(lookat)), fptr(f3(vup)), float(vfov_in_degrees),
                                float(aspect_ratio), float(aperture), float(focus_dist), C.byref(raw)))
        return Camera(raw)

    @staticmethod
    def world_camera(vfov_in_degrees, aspect_ratio):                                 # camera.rs:33-35
        return Camera.new((0., 0., 0.), (0., 0., -1.), (0., 1., 0.), vfov_in_degrees, aspect_ratio, 0., 1.)


# ---------------------------------------------------------------- traced.rs / marched.rs
class _Prim:
    def add_to(self, world_ptr):
        raise NotImplementedError


class Sphere(_Prim):
    """traced.rs:13-32 — unit sphere under an affine local_to_world (ellipsoid)."""

    def __init__(self, adder):
        self._adder = adder

    @staticmethod
    def new(m_local_to_world, mat):
        m = m_local_to_world
        return Sphere(lambda w: lib.om_world_add_sphere(w, fptr(m.m), C.byref(mat.raw)))

    @staticmethod
    def new_with_radius(o, r, mat):
        c = f3(o)
        return Sphere(lambda w: lib.om_world_add_sphere_radius(w, fptr(c), float(r), C.byref(mat.raw)))

    def add_to(self, w):
        return self._adder(w)


class Cube(Sphere):
    """traced.rs:229-247 — unit cube (half-extent 0.5) under an affine map."""

    @staticmethod
    def new(m_local_to_world, mat):
        m = m_local_to_world
        return Cube(lambda w: lib.om_world_add_cube(w, fptr(m.m), C.byref(mat.raw)))

    @staticmethod
    def new_with_length(o, length, mat):
        c = f3(o)
        return Cube(lambda w: lib.om_world_add_cube_length(w, fptr(c), float(length), C.byref(mat.raw)))


class Triangle(Sphere):
    """Barycentric<1> (traced.rs:118-226)."""

    _three = "om_world_add_triangle"
    _basis = "om_world_add_triangle_basis"

    @classmethod
    def new3points(cls, origin, upoint, vpoint, mat):
        a, b, c = f3(origin), f3(upoint), f3(vpoint)
        fn = getattr(lib, cls._three)
        return cls(lambda w: fn(w, fptr(a), fptr(b), fptr(c), C.byref(mat.raw)))

    @classmethod
    def new(cls, origin, u, v, u_length, v_length, mat):
        a, b, c = f3(origin), f3(u), f3(v)
        fn = getattr(lib, cls._basis)
        return cls(lambda w: fn(w, fptr(a), fptr(b), fptr(c), float(u_length), float(v_length), C.byref(mat.raw)))


class Parallelogram(Triangle):
    """Barycentric<0> (traced.rs:118-225)."""

    _three = "om_world_add_parallelogram"
    _basis = "om_world_add_parallelogram_basis"


class InfinitePlane(Sphere):
    """traced.rs:77-116."""

    @staticmethod
    def new(center, normal, material):
        a, b = f3(center), f3(normal)
        return InfinitePlane(lambda w: lib.om_world_add_plane(w, fptr(a), fptr(b), C.byref(material.raw)))


class MarchedSphere(Sphere):
    """marched.rs:50-76 (struct literal MarchedSphere{center, radius, material})."""

    def __init__(self, center, radius, material):
        c = f3(center)
        super().__init__(lambda w: lib.om_world_add_marched_sphere(w, fptr(c), float(radius), C.byref(material.raw)))


class MarchedBox(Sphere):
    """marched.rs:79-102 (struct literal MarchedBox{center, sizes, material})."""

    def __init__(self, center, sizes, material):
        c, s = f3(center), f3(sizes)
        super().__init__(lambda w: lib.om_world_add_marched_box(w, fptr(c), fptr(s), C.byref(material.raw)))


class MarchedTorus(Sphere):
    """marched.rs:105-151."""

    @staticmethod
    def new(m_local_to_world, local_sizes, mat):
        m, s = m_local_to_world, f3(local_sizes)
        return MarchedTorus(lambda w: lib.om_world_add_marched_torus(w, fptr(m.m), fptr(s), C.byref(mat.raw)))


class MarchedSdf(Sphere):
    """A user marched object, the device form of `HittableList += Arc<dyn Marched>` (hits.rs:96-100):
    an `impl Marched` whose local_sdf is a postfix program of om_sdf_op (include/ottomarcher.h),
    under MarchedTorus's transform and the trait's default normal (marched.rs:14-44, 139-151).

        MarchedSdf.new(m4x4("TR", 0, 1, 0), [("box", 0, 0, 0, .5, .5, .5), ("sphere", 0, 0, 0, .65),
                                             ("intersect",)], Material.new_metal((.8, .6, .2)))
    """

    @staticmethod
    def new(m_local_to_world, ops, mat):
        m, arr = m_local_to_world, L.sdf_ops(ops)
        return MarchedSdf(lambda w: lib.om_world_add_marched_sdf(w, fptr(m.m), arr.ctypes.data_as(C.c_void_p), arr.size,
                                                                C.byref(mat.raw)))


# ---------------------------------------------------------------- hits.rs
def _mesh_arrays(what, vertices, faces):
    """-> contiguous (V, 3) float32 vertices and (T, 3) uint32 faces (or None) of a numpy mesh"""
    v = np.ascontiguousarray(vertices)
    if v.dtype != np.float32 or v.ndim != 2 or v.shape[1] != 3:
        raise ValueError(f"{what}: vertices must be a (V, 3) float32 array")
    if faces is None:
        return v, None
    f = np.ascontiguousarray(faces)
    if f.dtype != np.uint32 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"{what}: faces must be a (T, 3) uint32 array")
    return v, f


class HittableList:
    """hits.rs:37-110 — host-side list; `world += prim` appends in type order."""

    def __init__(self):
        self._w = C.c_void_p()
        check(lib.om_world_create(C.byref(self._w)))

    @staticmethod
    def new():
        return HittableList()

    def __del__(self):
        if getattr(self, "_w", None) and self._w.value:
            lib.om_world_destroy(self._w)
            self._w = C.c_void_p()

    @property
    def handle(self):
        return self._w

    def __iadd__(self, prim):
        if not isinstance(prim, _Prim):
            # Arc<dyn Traced> user types (hits.rs:91-95) cannot cross the C-ABI; a user marched
            # object is a MarchedSdf (an SDF program)
            raise TypeError("only the reference's primitive types and MarchedSdf can be added to a device world")
        check(prim.add_to(self._w))
        return self

    def add_triangles(self, vertices, faces, material):
        """A triangle mesh with one material (om_world_add_triangles): `vertices` (V, 3) float32,
        `faces` (T, 3) uint32 vertex indices.  Face k becomes Triangle.new3points(v[f[k, 0]], v[f[k, 1]],
        v[f[k, 2]], material), in order, exactly as T `world += Triangle.new3points(...)` would; one C call
        for the whole mesh.  All or nothing: an index past the last vertex adds no triangle and raises."""
        v = np.ascontiguousarray(vertices)
        f = np.ascontiguousarray(faces)
        if v.dtype != np.float32 or v.ndim != 2 or v.shape[1] != 3:
            raise ValueError("add_triangles: vertices must be a (V, 3) float32 array")
        if f.dtype != np.uint32 or f.ndim != 2 or f.shape[1] != 3:
            raise ValueError("add_triangles: faces must be a (T, 3) uint32 array")
        if not isinstance(material, Material):
            raise TypeError("add_triangles: material must be a Material")
        check(lib.om_world_add_triangles(self._w, v.ctypes.data_as(C.c_void_p), v.shape[0], f.ctypes.data_as(C.c_void_p),
                                         f.shape[0], C.byref(material.raw)))
        return self

    def update_triangles(self, vertices, faces=None, first=0):
        """Move triangles of this world (om_world_update_triangles): triangles first .. first + T - 1,
        in the order they were added, become Triangle.new3points(v[f[k, 0]], v[f[k, 1]], v[f[k, 2]]) and
        keep their materials and obj ids; without `faces`, triangle k takes vertices 3k, 3k + 1,
        3k + 2.  All or nothing.  A frozen world made earlier does not change
        (FrozenHittableList.update_triangles moves that one)."""
        v, f = _mesh_arrays("update_triangles", vertices, faces)
        check(lib.om_world_update_triangles(self._w, int(first), v.ctypes.data_as(C.c_void_p), v.shape[0],
                                            f.ctypes.data_as(C.c_void_p) if f is not None else None,
                                            f.shape[0] if f is not None else v.shape[0] // 3))
        return self

    def clear(self):
        check(lib.om_world_clear(self._w))

    def counts(self):
        out = (C.c_uint32 * 8)()
        check(lib.om_world_counts(self._w, out))
        n = C.c_uint32()
        check(lib.om_world_marched_sdf_count(self._w, C.byref(n)))
        return dict(zip(["spheres", "cubes", "triangles", "infinite_planes", "parallelograms",
                         "marched_spheres", "marched_boxes", "marched_torus", "marched_sdf"], list(out) + [n.value]))

    def export(self, kind, index, n):
        out = (C.c_float * n)()
        check(lib.om_world_export(self._w, int(kind), int(index), fptr(out), n))
        return np.array(list(out), dtype=np.float32)

    def material_of(self, obj):
        """HitRecord.material (hits.rs:16) of an obj id as hit() / om_pixel_stats report it
        (global type-order index + 1); raises for 0 or an id past the last object."""
        raw = L.om_material()
        check(lib.om_world_object_material(self._w, int(obj), C.byref(raw)))
        return Material(raw)

    def tree_info(self):
        """The trees a freeze of this world builds and the regime kernel "auto" traces them in
        (om_world_tree_info: host only, no device): a dict of records, always_tested, b2_nodes,
        b2_leaves, b2_depth, b2_max_leaf, regime ("none" / "lds" / "l2" / "wide" / "fallback_bvh")
        and lds_bytes (the wavefront's LDS per workgroup in that regime)."""
        ti = L.om_tree_info()
        check(lib.om_world_tree_info(self._w, C.byref(ti)))
        return L.tree_info_dict(ti)

    def freeze(self, cam=None, device=0, kernel="auto", pipeline="auto"):
        """hits.rs:87-89: snapshot to device memory (the camera is unused: the camera hash is out of scope)."""
        return FrozenHittableList(self, device=device, kernel=kernel, pipeline=pipeline)


class FrozenHittableList:
    """hits.rs:63-69 — a world resident in HBM on one device (om_ctx)."""

    def __init__(self, world, device=0, kernel="auto", pipeline="auto"):
        self._ctx = C.c_void_p()
        check(lib.om_create(int(device), C.byref(self._ctx)))
        check(lib.om_upload_world(self._ctx, world.handle), self._ctx)
        self.set_kernel(kernel)
        self.set_pipeline(pipeline)
        self.device = device

    def set_pipeline(self, pipeline):
        check(lib.om_set_pipeline(self._ctx, L.PIPELINES[pipeline] if isinstance(pipeline, str) else int(pipeline)),
              self._ctx)

    def set_kernel(self, kernel):
        check(lib.om_set_kernel(self._ctx, L.KERNELS[kernel] if isinstance(kernel, str) else int(kernel)), self._ctx)

    def tree_info(self):
        """HittableList.tree_info() for the uploaded world, with the regime and LDS bytes of this
        frozen world's own kernel choice (om_get_tree_info)."""
        ti = L.om_tree_info()
        check(lib.om_get_tree_info(self._ctx, C.byref(ti)), self._ctx)
        return L.tree_info_dict(ti)

    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            lib.om_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        self.close()

    @property
    def ctx(self):
        return self._ctx

    def counters(self):
        c = L.om_counters()
        check(lib.om_get_counters(self._ctx, C.byref(c)), self._ctx)
        return {n: getattr(c, n) for n, _ in L.om_counters._fields_}

    def hit(self, orig, dir, tmin=0.001, tmax=100.0, march_steps=1024):
        """FrozenHittableList::hit (hits.rs:270-334) for one ray -> HitRecord or None.  `dir` is
        used as given; a unit direction is the precondition (Ray::new, ray.rs:12)."""
        rays = np.array([list(orig) + list(dir)], dtype=np.float32)
        h = self.hit_rays(rays, tmin, tmax, march_steps)[0]
        if h["obj"] == 0:
            return None
        return HitRecord(float(h["t"]), h["point"].copy(), h["normal"].copy(), int(h["obj"]))

    def hit_rays(self, rays, tmin=0.001, tmax=100.0, march_steps=1024, out=None, stream=None, windows=None):
        """Closest hits of a batch of rays (om_hit_rays / om_hit_rays_device).

        `rays`: an (n, 6) float32 array (orig, dir per row; or an n-vector of RAY_DTYPE) -> an
        n-vector of HIT_DTYPE (obj 0, t inf on a miss), synchronous; or a torch ROCm tensor of
        that shape on this world's device -> an (n, 8) float32 tensor of om_hit records on the
        device (column 7 holds the obj bits: `.view(torch.int32)`), traced in place with no host
        copy, asynchronously, in the order of `stream` (a non-null hipStream_t) or, by default, of
        torch's current stream on that device: the query runs after the work already queued there
        (the ops that made `rays`) and before what is queued afterwards (the readers of the result).
        When torch's current stream is the null stream, whose handle the C entry point would read as
        "the ctx's own stream", the launch goes to a side stream of this object that is ordered
        with the null stream by events on both sides.

        `windows`: one [tmin, tmax] per ray instead of the call's (om_hit_rays_windows*): an (n, 2)
        float32 array or an n-vector of WINDOW_DTYPE; with torch rays, an (n, 2) float32 tensor on
        the rays' device.  Windows are not validated: every ray gets the reference's answer for
        its own window, NaN and negative bounds included."""
        return self._query("hit_rays", rays, tmin, tmax, march_steps, windows, out, stream)

    def occluded(self, rays, tmin=0.001, tmax=100.0, march_steps=1024, windows=None, out=None, stream=None):
        """Any-hit query: hit(ray, tmin, tmax).is_some() per ray (om_occluded_rays /
        om_occluded_rays_device), for shadow, visibility and ambient-occlusion rays.

        `rays` and `windows` as for hit_rays.  numpy in -> a numpy bool n-vector, synchronous; a
        torch ROCm tensor in -> a torch.uint8 n-vector (0 / 1) on the same device, asynchronous,
        with the stream rules of hit_rays."""
        return self._query("occluded", rays, tmin, tmax, march_steps, windows, out, stream)

    @contextlib.contextmanager
    def _launch_stream(self, what, device, stream, tensors):
        """The stream rules of the device forms (hit_rays' docstring) -> the hipStream_t to launch on:
        `stream` (a non-null handle) or torch's current stream on `device`; when that is the null
        stream, a side stream of this object ordered with it by events on both sides, on which
        `tensors` are recorded so that the allocator does not reuse them under the kernel."""
        import torch
        if stream is not None and int(stream) == 0:
            raise ValueError(f"{what}: stream 0 is the ctx's own stream to the library; pass a stream or none")
        cur = side = None
        if stream is None:
            cur = torch.cuda.current_stream(device)
            stream = cur.cuda_stream
            if stream == 0:                                       # torch's null stream: order a side stream with it
                if getattr(self, "_torch_side", None) is None:
                    self._torch_side = torch.cuda.Stream(device=device)
                side = self._torch_side
                side.wait_stream(cur)
                stream = side.cuda_stream
        try:
            yield stream
        finally:
            if side is not None:
                for t in tensors:
                    t.record_stream(side)
                cur.wait_stream(side)

    def update_triangles(self, vertices, faces=None, first=0, stream=None):
        """Move triangles of the uploaded world in place (om_update_triangles /
        om_update_triangles_device): triangles first .. first + T - 1 (in the order
        they were added) become Triangle.new3points(v[f[k, 0]], v[f[k, 1]], v[f[k, 2]]); without
        `faces`, triangle k takes vertices 3k, 3k + 1, 3k + 2.  The trees keep their topology and every
        box is recomputed, so every later answer is the reference's for the moved mesh.

        numpy in (`vertices` (V, 3) float32, `faces` (T, 3) uint32): synchronous; an index past the
        last vertex raises and changes nothing.  torch ROCm tensors in ((V, 3) float32, (T, 3) int32
        or uint32, on this world's device): in place with no host copy, asynchronous, with the stream
        rules of hit_rays; a face with an index outside the vertices is left as it was and counted
        in update_info()["skipped"]."""
        what = "update_triangles"
        if type(vertices).__module__.split(".")[0] == "torch":
            import torch
            v, f = vertices, faces
            if not v.is_cuda or v.dtype != torch.float32 or v.dim() != 2 or v.shape[1] != 3 or not v.is_contiguous():
                raise ValueError(f"{what}: need a contiguous (V, 3) float32 tensor on the device")
            if v.device.index != int(self.device):
                raise ValueError(f"{what}: vertices are on {v.device}, the world is on device {self.device}")
            if f is not None:
                if type(f).__module__.split(".")[0] != "torch" or not f.is_cuda or f.device != v.device or f.dim() != 2 \
                        or f.shape[1] != 3 or not f.is_contiguous() or f.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
                    raise ValueError(f"{what}: faces must be a contiguous (T, 3) int32 / uint32 tensor on the vertices' device")
            n_tri = f.shape[0] if f is not None else v.shape[0] // 3
            with self._launch_stream(what, v.device, stream, [v] + ([f] if f is not None else [])) as st:
                check(lib.om_update_triangles_device(self._ctx, int(first), C.c_void_p(v.data_ptr()), v.shape[0],
                                                     C.c_void_p(f.data_ptr()) if f is not None else None, n_tri, C.c_void_p(st)),
                      self._ctx)
            return self
        v, f = _mesh_arrays(what, vertices, faces)
        check(lib.om_update_triangles(self._ctx, int(first), v.ctypes.data_as(C.c_void_p), v.shape[0],
                                      f.ctypes.data_as(C.c_void_p) if f is not None else None,
                                      f.shape[0] if f is not None else v.shape[0] // 3), self._ctx)
        return self

    def update_info(self):
        """om_get_update_info: updates since the upload, and of the last one the triangles rewritten,
        those given an all-covering box for a non-finite value (unbounded) and those skipped for an
        index outside the vertices.  Synchronises like counters()."""
        u = L.om_update_info()
        check(lib.om_get_update_info(self._ctx, C.byref(u)), self._ctx)
        return {n: int(getattr(u, n)) for n, _ in L.om_update_info._fields_}

    def _query(self, what, rays, tmin, tmax, march_steps, windows, out, stream):
        occ = what == "occluded"
        q = L.om_query_params(float(tmin), float(tmax), int(march_steps), 0)
        if type(rays).__module__.split(".")[0] == "torch":
            import torch
            if not rays.is_cuda or rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 6 \
                    or not rays.is_contiguous():
                raise ValueError(f"{what}: need a contiguous (n, 6) float32 tensor on the device")
            if rays.device.index != int(self.device):
                raise ValueError(f"{what}: rays are on {rays.device}, the world is on device {self.device}")
            n = rays.shape[0]
            if windows is not None:
                if type(windows).__module__.split(".")[0] != "torch" or not windows.is_cuda or windows.dtype != torch.float32 \
                        or tuple(windows.shape) != (n, 2) or not windows.is_contiguous() or windows.device != rays.device:
                    raise ValueError(f"{what}: windows must be a contiguous (n, 2) float32 tensor on the rays' device")
            shape, dtype = ((n,), torch.uint8) if occ else ((n, 8), torch.float32)
            if out is None:
                out = torch.empty(shape, dtype=dtype, device=rays.device)
            elif type(out).__module__.split(".")[0] != "torch" or not out.is_cuda or out.dtype != dtype \
                    or tuple(out.shape) != shape or not out.is_contiguous() or out.device != rays.device:
                raise ValueError(f"{what}: out must be a contiguous {shape} {dtype} tensor on the rays' device")
            wp = C.c_void_p(windows.data_ptr()) if windows is not None else None
            with self._launch_stream(what, rays.device, stream, [rays, out] + ([windows] if windows is not None else [])) as st:
                if occ:
                    check(lib.om_occluded_rays_device(self._ctx, C.byref(q), C.c_void_p(rays.data_ptr()), wp, n,
                                                      C.c_void_p(out.data_ptr()), C.c_void_p(st)), self._ctx)
                elif windows is not None:
                    check(lib.om_hit_rays_windows_device(self._ctx, C.byref(q), C.c_void_p(rays.data_ptr()), wp, n,
                                                         C.c_void_p(out.data_ptr()), C.c_void_p(st)), self._ctx)
                else:
                    check(lib.om_hit_rays_device(self._ctx, C.byref(q), C.c_void_p(rays.data_ptr()), n,
                                                 C.c_void_p(out.data_ptr()), C.c_void_p(st)), self._ctx)
            return out
        a = np.ascontiguousarray(rays)
        if a.dtype == L.RAY_DTYPE:
            a = a.reshape(-1)
        else:
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.ndim != 2 or a.shape[1] != 6:
                raise ValueError(f"{what}: need an (n, 6) float32 array")
        n = a.shape[0]
        wp = None
        if windows is not None:
            if type(windows).__module__.split(".")[0] == "torch":
                raise ValueError(f"{what}: numpy rays need numpy windows")
            w = np.ascontiguousarray(windows)
            if w.dtype == L.WINDOW_DTYPE:
                w = w.reshape(-1)
                ok = w.shape[0] == n
            else:
                ok = w.dtype == np.float32 and w.ndim == 2 and w.shape == (n, 2)
            if not ok:
                raise ValueError(f"{what}: windows must be an (n, 2) float32 array or an n-vector of WINDOW_DTYPE")
            wp = w.ctypes.data_as(C.c_void_p)
        if occ:
            res = np.empty(n, dtype=np.uint8)
            check(lib.om_occluded_rays(self._ctx, C.byref(q), a.ctypes.data_as(C.c_void_p), wp, n,
                                       res.ctypes.data_as(C.c_void_p)), self._ctx)
            return res.view(np.bool_)
        hits = np.empty(n, dtype=L.HIT_DTYPE)
        if windows is not None:
            check(lib.om_hit_rays_windows(self._ctx, C.byref(q), a.ctypes.data_as(C.c_void_p), wp, n,
                                          hits.ctypes.data_as(C.c_void_p)), self._ctx)
        else:
            check(lib.om_hit_rays(self._ctx, C.byref(q), a.ctypes.data_as(C.c_void_p), n, hits.ctypes.data_as(C.c_void_p)),
                  self._ctx)
        return hits

    def set_path_batch(self, paths_log2):
        """Paths per batch of ray_color: 2^paths_log2 (6..27; 0 = default), a pure scheduling knob
        (om_set_path_batch)."""
        check(lib.om_set_path_batch(self._ctx, int(paths_log2)), self._ctx)

    def ray_color(self, rays, max_depth=50, tmin=0.001, tmax=100.0, march_steps=1024, seed=1, stream_base=0, sample=0,
                  rng=None, out=None, stream=None):
        """ray_color (render_thread.rs:128-143) of a batch of caller-given rays: the renderer's bounce
        loop entered with any ray (om_ray_color / om_ray_color_device).

        `rays` as for hit_rays.  numpy in -> an n-vector of RADIANCE_DTYPE (color, depth = the first
        segment's t or inf, obj = the first-hit id or 0), synchronous.  A torch ROCm tensor in -> an
        (n, 5) float32 tensor of om_radiance records on the device (column 4 holds the obj bits),
        asynchronous, with the stream rules of hit_rays.
        The path of ray i draws from `rng[i]` (uint64 PathRng states, path_rng_state; a numpy array
        with numpy rays, an int64 tensor on the rays' device with torch rays) or, by default, from the
        stream (seed, stream_base + i mod 2^32, sample) from its start.  Callers that want several
        samples per ray repeat the call with another `sample`."""
        what = "ray_color"
        p = L.om_path_params(float(tmin), float(tmax), int(march_steps), int(max_depth), int(seed),
                             int(stream_base) & 0xFFFFFFFF, int(sample) & 0xFFFFFFFF)
        if type(rays).__module__.split(".")[0] == "torch":
            import torch
            if not rays.is_cuda or rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 6 \
                    or not rays.is_contiguous():
                raise ValueError(f"{what}: need a contiguous (n, 6) float32 tensor on the device")
            if rays.device.index != int(self.device):
                raise ValueError(f"{what}: rays are on {rays.device}, the world is on device {self.device}")
            n = rays.shape[0]
            if rng is not None:
                if type(rng).__module__.split(".")[0] != "torch" or not rng.is_cuda or rng.dtype != torch.int64 \
                        or tuple(rng.shape) != (n,) or not rng.is_contiguous() or rng.device != rays.device:
                    raise ValueError(f"{what}: rng must be a contiguous (n,) int64 tensor on the rays' device")
            if out is None:
                out = torch.empty((n, 5), dtype=torch.float32, device=rays.device)
            elif type(out).__module__.split(".")[0] != "torch" or not out.is_cuda or out.dtype != torch.float32 \
                    or tuple(out.shape) != (n, 5) or not out.is_contiguous() or out.device != rays.device:
                raise ValueError(f"{what}: out must be a contiguous (n, 5) float32 tensor on the rays' device")
            rp = C.c_void_p(rng.data_ptr()) if rng is not None else None
            with self._launch_stream(what, rays.device, stream, [rays, out] + ([rng] if rng is not None else [])) as st:
                check(lib.om_ray_color_device(self._ctx, C.byref(p), C.c_void_p(rays.data_ptr()), rp, n,
                                              C.c_void_p(out.data_ptr()), C.c_void_p(st)), self._ctx)
            return out
        a = np.ascontiguousarray(rays)
        if a.dtype == L.RAY_DTYPE:
            a = a.reshape(-1)
        else:
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.ndim != 2 or a.shape[1] != 6:
                raise ValueError(f"{what}: need an (n, 6) float32 array")
        n = a.shape[0]
        rp = None
        if rng is not None:
            if type(rng).__module__.split(".")[0] == "torch":
                raise ValueError(f"{what}: numpy rays need numpy rng states")
            r = np.ascontiguousarray(rng, dtype=np.uint64)
            if r.shape != (n,):
                raise ValueError(f"{what}: rng must hold one uint64 state per ray")
            rp = r.ctypes.data_as(C.c_void_p)
        if out is None:
            out = np.empty(n, dtype=L.RADIANCE_DTYPE)
        elif not isinstance(out, np.ndarray) or out.dtype != L.RADIANCE_DTYPE or out.shape != (n,) or not out.flags.c_contiguous:
            raise ValueError(f"{what}: out must be a contiguous n-vector of RADIANCE_DTYPE")
        check(lib.om_ray_color(self._ctx, C.byref(p), a.ctypes.data_as(C.c_void_p), rp, n, out.ctypes.data_as(C.c_void_p)),
              self._ctx)
        return out

    def render_rays(self, pixels_box, rays, image_width, image_height, samples_per_pixel, max_depth=50, tmin=0.001,
                    tmax=100.0, march_steps=1024, rng=None, pixels=None, adaptive=True, seed=1, stream=None):
        """Samples of a frame from caller-given rays: render()'s pass loop with `rays` in the place of
        Camera::get_ray (om_render_rays / om_render_rays_device), for any camera model.

        `rays` is (S, n, 6) or (S * n, 6) float32, sample-major: sample s of listed pixel k is row
        s * n + k, and the call takes S samples.  The pixel of entry k is `pixels[k]` (row-major
        indices, each at most once), or k with `pixels` None, where n = image_width * image_height.
        For s in order, a pixel takes the sample iff its Stats.n < samples_per_pixel and, with
        `adaptive`, it has not retired; the sample is ray_color(ray) added by Stats::add, as in
        render().  A pixel that is full or retired reads no ray, so a frame can be grown over any
        number of calls.  The path draws from `rng` (path_rng_state values, shaped like the rays
        without the last axis) or, by default, from the stream (seed, pixel, Stats.n).

        numpy in: `pixels_box` is a PixelsBox or a W*H array of om_pixel_stats, `rng` uint64, `pixels`
        uint32; synchronous, returns the call's RenderStats.  torch ROCm tensors in: `pixels_box` is
        the frame's Stats on the device, W*H records of 40 bytes in a contiguous tensor (for one a
        (W*H, 40) uint8 tensor), `rng` int64, `pixels` int32 holding the uint32 indices; asynchronous
        with the stream rules of hit_rays, returns None (counters() reads the counters)."""
        what = "render_rays"
        W, H = int(image_width), int(image_height)
        if W <= 0 or H <= 0:
            raise ValueError(f"{what}: image_width and image_height must be positive")
        is_torch = lambda x: type(x).__module__.split(".")[0] == "torch"
        given = [x for x in (rays, rng, pixels, pixels_box) if x is not None]
        dev = is_torch(rays)
        if any(is_torch(x) != dev for x in given):
            raise ValueError(f"{what}: rays, rng, pixels and the Stats are all numpy or all torch")
        if pixels is not None and (pixels.ndim != 1 or pixels.shape[0] > W * H):
            raise ValueError(f"{what}: pixels is a vector of at most image_width * image_height indices")
        n = W * H if pixels is None else int(pixels.shape[0])
        if dev:
            import torch
            if not rays.is_cuda or rays.dtype != torch.float32 or not rays.is_contiguous():
                raise ValueError(f"{what}: need contiguous float32 rays on the device")
            if rays.device.index != int(self.device):
                raise ValueError(f"{what}: rays are on {rays.device}, the world is on device {self.device}")
        else:
            rays = np.ascontiguousarray(rays)
            if rays.dtype != np.float32:
                raise ValueError(f"{what}: need float32 rays")
        if rays.ndim == 3 and tuple(rays.shape[1:]) == (n, 6):
            S = int(rays.shape[0])
        elif rays.ndim == 2 and rays.shape[1] == 6 and n and rays.shape[0] % n == 0:
            S = int(rays.shape[0]) // n
        elif rays.ndim == 2 and rays.shape[1] == 6 and rays.shape[0] == 0:
            S = 0
        else:
            raise ValueError(f"{what}: rays must be (S, {n}, 6) or (S * {n}, 6)")
        p = make_params(max_depth, tmin, tmax, samples_per_pixel, W, H, sample_count=S, seed=seed,
                        march_steps=march_steps, adaptive=adaptive)
        if dev:
            st = pixels_box
            if not st.is_cuda or not st.is_contiguous() or st.device != rays.device \
                    or st.numel() * st.element_size() != W * H * 40:
                raise ValueError(f"{what}: the Stats must be a contiguous tensor of W*H 40-byte records on the rays' device")
            if rng is not None and (not rng.is_cuda or rng.dtype != torch.int64 or rng.numel() != S * n
                                    or not rng.is_contiguous() or rng.device != rays.device):
                raise ValueError(f"{what}: rng must be a contiguous int64 tensor on the rays' device, one state per ray")
            if pixels is not None and (not pixels.is_cuda or pixels.dtype != torch.int32 or not pixels.is_contiguous()
                                       or pixels.device != rays.device):
                raise ValueError(f"{what}: pixels must be a contiguous int32 tensor on the rays' device")
            ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
            with self._launch_stream(what, rays.device, stream, [t for t in (rays, rng, pixels, st) if t is not None]) as hs:
                check(lib.om_render_rays_device(self._ctx, C.byref(p), ptr(rays), ptr(rng), ptr(pixels), n, ptr(st),
                                                C.c_void_p(hs)), self._ctx)
            return None
        buf = pixels_box.pixels if isinstance(pixels_box, PixelsBox) else pixels_box
        if not isinstance(buf, np.ndarray) or buf.dtype != L.PIXEL_STATS_DTYPE or buf.size != W * H \
                or not buf.flags["C_CONTIGUOUS"]:
            raise ValueError(f"{what}: pixels_box must be a contiguous W*H om_pixel_stats array")
        rp = pp = None
        if rng is not None:
            if rng.dtype != np.uint64 or rng.size != S * n:
                raise ValueError(f"{what}: rng must hold one uint64 state per ray")
            rng = np.ascontiguousarray(rng)
            rp = rng.ctypes.data_as(C.c_void_p)
        if pixels is not None:
            if pixels.dtype != np.uint32:
                raise ValueError(f"{what}: pixels must be uint32")
            pixels = np.ascontiguousarray(pixels)
            pp = pixels.ctypes.data_as(C.c_void_p)
        ctr = L.om_counters()
        check(lib.om_render_rays(self._ctx, C.byref(p), rays.ctypes.data_as(C.c_void_p), rp, pp, n,
                                 buf.ctypes.data_as(C.c_void_p), C.byref(ctr)), self._ctx)
        return RenderStats({k: getattr(ctr, k) for k, _ in L.om_counters._fields_})

    def query_max_grid(self):
        """Workgroups of the largest query launch on this device (om_query_max_grid)."""
        return int(lib.om_query_max_grid(self._ctx))


class HitRecord:
    """hits.rs:11-17: t, point, normal and the obj id (HittableList.material_of gives the material)."""
    __slots__ = ("t", "point", "normal", "obj")

    def __init__(self, t, point, normal, obj):
        self.t, self.point, self.normal, self.obj = t, point, normal, obj

    def __repr__(self):
        return f"HitRecord(t={self.t}, point={tuple(self.point)}, normal={tuple(self.normal)}, obj={self.obj})"


# ---------------------------------------------------------------- render_thread.rs
class PixelsBox:
    """The caller-owned framebuffer (render_thread.rs:42-65): W*H om_pixel_stats."""

    def __init__(self, image_size):
        self.pixels = np.zeros(int(image_size), dtype=L.PIXEL_STATS_DTYPE)
        self._pinned = None

    @staticmethod
    def new(image_size):
        return PixelsBox(image_size)

    def pin(self):
        """Page-lock the framebuffer (om_host_register) so render()'s copies run as DMA; kept
        until the box dies or `pixels` is replaced.  Best effort, like the C++ render(): a
        refused registration (memlock limit, an already registered buffer) leaves the buffer
        pageable, and the copies still work.  Done by render() on first use (needs a HIP device)."""
        if self._pinned is not None and self._pinned is not self.pixels:
            self.unpin()                                   # `pixels` was replaced: release the old one
        if self._pinned is None and self.pixels.nbytes:
            if lib.om_host_register(self.pixels.ctypes.data, self.pixels.nbytes) == L.OM_OK:
                self._pinned = self.pixels                 # a reference: the array cannot be freed while registered
        return self

    def unpin(self):
        if getattr(self, "_pinned", None) is not None:
            lib.om_host_unregister(self._pinned.ctypes.data)
            self._pinned = None

    def __del__(self):
        self.unpin()


def make_params(max_depth, tmin, tmax, samples_per_pixel, image_width, image_height, sample_count=None,
                seed=1, march_steps=1024, adaptive=False, sample_begin=0):
    p = L.om_render_params()
    p.width, p.height = int(image_width), int(image_height)
    p.spp_total = int(samples_per_pixel)
    p.sample_begin = int(sample_begin)
    p.sample_count = int(samples_per_pixel if sample_count is None else sample_count)
    p.max_depth = int(max_depth)
    p.tmin, p.tmax = float(tmin), float(tmax)
    p.march_steps = int(march_steps)
    p.adaptive = 1 if adaptive else 0
    p.seed = int(seed)
    return p


class RenderStats(dict):
    pass


def render(camera, world, max_depth, tmin, tmax, samples_per_pixel, image_width, image_height, pixels_box,
           tid=0, assigned_thread=None, samples_atom=None, *, seed=1, march_steps=1024, adaptive=True,
           sample_count=None):
    """render_thread::render (render_thread.rs:145-202) for the whole frame.

    `adaptive` defaults to True, as the reference always retires a pixel once bad_avgs
    reaches 5 (ThreadPixels::add_run, render_thread.rs:97-101,195-198) and credits its
    untaken samples to samples_atom; pass adaptive=False for a fixed-spp render (the
    BASELINE metric).

    The reference spawns num_cpus-1 threads with disjoint pixel sets (main.rs:200-214);
    here tid 0 renders every pixel on the device and other tids return at once, so a
    front-end that still spawns threads stays correct.  `samples_atom`, if given, is a
    one-element list incremented by the credited samples (render_thread.rs:196-198).
    """
    if tid != 0:
        return None
    p = make_params(max_depth, tmin, tmax, samples_per_pixel, image_width, image_height,
                    sample_count=sample_count, seed=seed, march_steps=march_steps, adaptive=adaptive)
    buf = pixels_box.pixels if isinstance(pixels_box, PixelsBox) else pixels_box
    if buf.dtype != L.PIXEL_STATS_DTYPE or buf.size != p.width * p.height or not buf.flags["C_CONTIGUOUS"]:
        raise ValueError("pixels must be a contiguous W*H om_pixel_stats array")
    if isinstance(pixels_box, PixelsBox) and p.width * p.height > 0:
        pixels_box.pin()
    ctr = L.om_counters()
    check(lib.om_render(world.ctx, C.byref(camera.raw), C.byref(p), buf.ctypes.data_as(C.c_void_p), C.byref(ctr)),
          world.ctx)
    out = RenderStats({n: getattr(ctr, n) for n, _ in L.om_counters._fields_})
    if samples_atom is not None:
        samples_atom[0] += out["credited"]
    return out


# ---------------------------------------------------------------- main.rs draw_to_sdl
def display(frozen, pixels_box, image_width, image_height, view="normal", rgb=None):
    """One draw_to_sdl view (main.rs:360-437) of the framebuffer, computed on the device
    of `frozen` -> (H, W, 3) uint8 RGB.  `view`: a name of _lib.VIEWS or 0-6 (the
    reference's keypad modes).  Pass the previous `rgb` to keep the reference's
    behaviour for pixels its box filter never visits (W or H == 2)."""
    st = pixels_box.pixels if isinstance(pixels_box, PixelsBox) else pixels_box
    st = np.ascontiguousarray(st)
    W, H = int(image_width), int(image_height)
    if st.dtype != L.PIXEL_STATS_DTYPE or st.size != W * H:
        raise ValueError("display: need W*H om_pixel_stats")
    mode = L.VIEWS.index(view) if isinstance(view, str) else int(view)
    out = np.zeros(W * H * 3, dtype=np.uint8) if rgb is None else np.ascontiguousarray(rgb, dtype=np.uint8).reshape(-1).copy()
    check(lib.om_display(frozen.ctx, st.ctypes.data, W, H, mode, out.ctypes.data), frozen.ctx)
    return out.reshape(H, W, 3)


def write_bmp(path, rgb):
    """24-bit BMP of an (H, W, 3) uint8 image (the F12 save, main.rs:473-476)."""
    a = np.ascontiguousarray(rgb, dtype=np.uint8)
    check(lib.om_write_bmp(str(path).encode(), a.ctypes.data, a.shape[1], a.shape[0]))


def write_ppm(path, rgb):
    """Binary PPM (P6) of an (H, W, 3) uint8 image."""
    a = np.ascontiguousarray(rgb, dtype=np.uint8)
    check(lib.om_write_ppm(str(path).encode(), a.ctypes.data, a.shape[1], a.shape[0]))
