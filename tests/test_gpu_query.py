"""Ray queries (om_hit_rays*, FrozenHittableList.hit_rays) against the CPU oracle, ray by ray.

Every om_hit record must be identical to oracle.World.hit on the same float32 ray: all 32 bytes
(t, point, normal, obj), a miss being obj 0, t +inf, point = normal = 0.  Only the edge-ray test
lets NaN payload bits differ (x86's default NaN carries the sign bit, gfx950's does not).

Ray sets (numpy, fixed seed; directions normalised once in float32 here, the same bits to both sides):
  (a) pinhole rays through the pixel centres of a 48x32 frame of the world's camera,
  (b) one random unit direction from every oracle hit point of (a): origins on surfaces, the tmin rule,
  (c) rays from random points of the scene's bounds (below the ground surface included): many start
      inside objects, so the far roots are taken.

Witness thresholds (test_sets_test_the_tree), measured with the oracle alone on the CPU, seed RAY_SEED:
  distinct hit objects per set: g11 283, g15 377, g16 437, g17 445, g23 495, g50x 755, g91x 842,
                                c7x18 423, c8x17 429                      -> smallest 283
      (g0x and g0 hold 1 and 9 objects and hit 1 and 4: exempt from this bound)
  share of rays that hit:       c7x18 0.574, c8x17 0.575, g15 0.657, g11 0.660, g16 0.662, g17 0.666,
                                g23 0.674, g50x 0.694, g91x 0.698         -> smallest 0.574
                                g0x 0.471, g0 0.498 (no field of spheres to hit) -> smallest 0.471
  (set (a) alone hits 0.78-1.00; about half of set (c)'s random directions leave for the sky)
The test asserts 80 % of the smallest of each group: >= 226 distinct objects and a hit share >= 0.459
for the worlds with a tree of spheres, a hit share >= 0.3768 for g0x and g0; every set is far above
the 50 distinct objects below which it would be too weak to test a tree.
"""
import ctypes as C

import numpy as np
import pytest

from scenes_common import REGIME_WORLDS, _unit, kitchen_sink, oracle_hits, pinhole_rays, tie_scene  # noqa: F401  (re-exported)

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 48, 32
RAY_SEED = 20261019
KERNELS = ["brute", "culled", "bvh", "sbvh", "bvh2", "bvh4"]
REGIMES = ["g0x", "g0", "g11", "g16", "g17", "g23", "g50x", "g91x", "c7x18", "c8x17"]
SBVH_WORLDS = ["g15", "g16"]
SMALL_WORLDS = ("g0x", "g0")
MIN_DISTINCT, MIN_HIT_SHARE = 226, 0.459          # 80 % of the smallest measured values (docstring)
MIN_HIT_SHARE_SMALL = 0.3768                      # the same for g0x / g0 (smallest 0.471)


def ray_sets(om, ow, cam, lo, hi, seed=RAY_SEED, tmin=0.001, tmax=100.0):
    """Sets (a), (b), (c) of the module docstring, concatenated, with the oracle's answers."""
    rng = np.random.default_rng(seed)
    a = pinhole_rays(cam)
    ea = oracle_hits(om, ow, a, tmin, tmax)
    on = ea["obj"] != 0
    b = np.concatenate([ea["point"][on], _unit(rng.standard_normal((int(on.sum()), 3)))], axis=1).astype(F)
    n_c = W * H
    oc = (np.asarray(lo, F) + rng.random((n_c, 3), dtype=F) * (np.asarray(hi, F) - np.asarray(lo, F))).astype(F)
    c = np.concatenate([oc, _unit(rng.standard_normal((n_c, 3)))], axis=1).astype(F)
    rays = np.ascontiguousarray(np.concatenate([a, b, c], axis=0))
    exp = np.concatenate([ea, oracle_hits(om, ow, b, tmin, tmax), oracle_hits(om, ow, c, tmin, tmax)])
    return rays, exp


def compare_hits(got, exp, label, nan_payload=False):
    """All 32 bytes of every record; nan_payload: a NaN float only has to be a NaN on both sides."""
    g, e = got.copy(), exp.copy()
    if nan_payload:
        gf, ef = g.view(F).reshape(-1, 8)[:, :7], e.view(F).reshape(-1, 8)[:, :7]
        gn, en = np.isnan(gf), np.isnan(ef)
        assert np.array_equal(gn, en), f"{label}: NaN-ness differs on {int((gn != en).any(axis=1).sum())} rays"
        gf[gn] = 0.0
        ef[en] = 0.0
    bad = np.nonzero((g.view(np.uint8).reshape(-1, 32) != e.view(np.uint8).reshape(-1, 32)).any(axis=1))[0]
    rows = [f"ray {i}: got t={got['t'][i]!r} p={got['point'][i]} n={got['normal'][i]} obj={got['obj'][i]} | "
            f"exp t={exp['t'][i]!r} p={exp['point'][i]} n={exp['normal'][i]} obj={exp['obj'][i]}" for i in bad[:5]]
    assert len(bad) == 0, f"{label}: {len(bad)}/{len(got)} records differ\n" + "\n".join(rows)


def _set_oracle_steps(oracle, ow, steps):
    f = oracle.lib.oro_world_set_march_steps
    f.restype, f.argtypes = None, [C.c_void_p, C.c_uint32]
    f(ow.h, int(steps))


def _grid_bounds(name):
    if name.startswith("c"):
        s = F(int(name.split("x")[1]) * 0.5 + 1.0)
        return (-s, F(-0.3), -s), (s, F(0.9), s)
    g = F(int(name[1:].rstrip("x")) + 2)
    return (-g, F(-0.3), -g), (g, F(1.5), g)


class _Cache:
    """Worlds and oracle answers, each built once per module and never changed."""

    def __init__(self, om, oracle):
        self.om, self.oracle, self.d = om, oracle, {}

    def regime(self, name):
        if name not in self.d:
            wb, cb = REGIME_WORLDS[name]
            w, ow = wb(self.om, self.oracle)
            cam, _ = cb(self.om, self.oracle, W / H)
            lo, hi = _grid_bounds(name)
            self.d[name] = (w,) + ray_sets(self.om, ow, cam, lo, hi)
        return self.d[name]

    def kitchen(self):
        if "kitchen" not in self.d:
            w, ow, cam, _ = kitchen_sink(self.om, self.oracle)
            self.d["kitchen"] = (w,) + ray_sets(self.om, ow, cam, (-3., -0.8, -3.5), (3., 2.2, 1.))
        return self.d["kitchen"]


@pytest.fixture(scope="module")
def cache(om, oracle):
    return _Cache(om, oracle)


def _query(w, rays, kernel="auto", **kw):
    fz = w.freeze(kernel=kernel)
    try:
        return fz.hit_rays(rays, **kw)
    finally:
        fz.close()


# ------------------------------------------------------------------ worlds x kernels
@pytest.mark.parametrize("kernel", KERNELS)
def test_kitchen_sink_every_kernel(om, cache, kernel):
    w, rays, exp = cache.kitchen()
    compare_hits(_query(w, rays, kernel), exp, f"kitchen_sink/{kernel}")


def test_kitchen_sink_rays_reach_every_primitive_type(om, cache):
    _, rays, exp = cache.kitchen()
    assert set(range(1, 11)) <= set(int(x) for x in exp["obj"]), sorted(set(int(x) for x in exp["obj"]))
    assert (exp["obj"] == 0).any()                               # and some rays miss


def _zoo(om, oracle):
    from test_gpu_parity import _marched_zoo
    w, ow, cam, _ = _marched_zoo(om, oracle)
    ops = [("box", 0., 0., 0., 0.25, 0.25, 0.25), ("sphere", 0., 0., 0., 0.32), ("intersect",)]
    l2w = om.m4x4("TR", 1.0, 0.35, -0.9) ^ om.m4x4("RY", 0.6) ^ om.m4x4("SC", 1.2, 0.9, 1.0)
    w += om.MarchedSdf.new(l2w, ops, om.Material.new_metal((0.8, 0.6, 0.2)))
    ow.add_marched_sdf(l2w.to_numpy(), ops, oracle.material("metal", (0.8, 0.6, 0.2)))
    return w, ow, cam


@pytest.fixture(scope="module")
def zoo(om, oracle):
    """_marched_zoo + one MarchedSdf program object, with the oracle's answers at 512 and 7 march steps."""
    w, ow, cam = _zoo(om, oracle)
    out = {}
    for steps in (512, 7):
        _set_oracle_steps(oracle, ow, steps)
        out[steps] = ray_sets(om, ow, cam, (-1.6, -0.3, -1.6), (1.6, 2.0, 1.6))
    _set_oracle_steps(oracle, ow, 1024)
    return w, out


@pytest.mark.parametrize("steps", [512, 7])
def test_marched_zoo_with_sdf_program(om, zoo, steps):
    w, sets = zoo
    rays, exp = sets[steps]
    assert int(exp["obj"].max()) == 9                            # the program object (last id) is hit
    compare_hits(_query(w, rays, march_steps=steps), exp, f"marched zoo/{steps} steps")


def test_march_step_cap_decides_rays(zoo):
    """From the oracle alone: with 7 steps the cap ends marches that 512 steps finish.  Set (a) is
    the same in both (set (b) starts from (a)'s hit points, which the cap moves)."""
    _, sets = zoo
    n = W * H
    a512, a7 = sets[512][1][:n], sets[7][1][:n]
    assert np.array_equal(sets[512][0][:n], sets[7][0][:n])
    differ = int((a512.view(np.uint8).reshape(-1, 32) != a7.view(np.uint8).reshape(-1, 32)).any(axis=1).sum())
    assert differ > 0


def test_marched_scene(om, oracle):
    w, ow = om.marched_scene(), oracle.marched_scene()
    cam = om.default_camera(W / H)
    rays, exp = ray_sets(om, ow, cam, (-4., -0.3, -4.), (4., 2.5, 4.))
    assert len(set(int(x) for x in exp["obj"])) >= 4
    compare_hits(_query(w, rays), exp, "marched_scene")


@pytest.mark.parametrize("kernel", ["bvh2", "bvh4"])
@pytest.mark.parametrize("name", REGIMES)
def test_tree_regimes(om, cache, name, kernel):
    w, rays, exp = cache.regime(name)
    compare_hits(_query(w, rays, kernel), exp, f"{name}/{kernel}")


@pytest.mark.parametrize("name", SBVH_WORLDS)
def test_sbvh_staging_cut(om, cache, name):
    w, rays, exp = cache.regime(name)
    compare_hits(_query(w, rays, "sbvh"), exp, f"{name}/sbvh")


@pytest.mark.parametrize("name", sorted(set(REGIMES + SBVH_WORLDS)))
def test_sets_test_the_tree(cache, name):
    """From the oracle alone: the rays of a set hit many different objects of the tree, and most
    of them hit something (thresholds: module docstring)."""
    _, rays, exp = cache.regime(name)
    distinct = len(set(int(x) for x in exp["obj"]) - {0})
    share = float((exp["obj"] != 0).mean())
    print(f"{name}: {len(rays)} rays, {distinct} distinct objects, hit share {share:.3f}")
    if name in SMALL_WORLDS:
        assert distinct >= 1 and share >= MIN_HIT_SHARE_SMALL
    else:
        assert distinct >= MIN_DISTINCT and share >= MIN_HIT_SHARE


# ------------------------------------------------------------------ ray counts
def test_ray_counts_partial_waves_blocks_and_looping_workgroups(om, cache):
    """n = 1 .. 513 (a partial wave, a partial workgroup) and 4 x 512 x (resident grid) + 3 (every
    workgroup loops, the last block is partial): each equals the first n records of one large
    call, whose head is checked against the oracle."""
    from raytracingoneweekend_amd import _lib
    w, rays, exp = cache.regime("g11")
    fz = w.freeze(kernel="bvh2")
    grid = fz.query_max_grid()
    assert grid > 0 and grid % 4 == 0
    big_n = 4 * _lib.OM_QUERY_BLOCK * grid + 3
    big_rays = np.ascontiguousarray(np.resize(rays, (big_n, 6)))
    big = fz.hit_rays(big_rays)
    compare_hits(big[:len(rays)], exp, "g11/large call head")
    reps = big_n // len(rays)
    tiled = big[:reps * len(rays)].view(np.uint8).reshape(reps, -1)
    assert (tiled == tiled[0]).all(), "repeated rays of the large call gave different records"
    compare_hits(big[reps * len(rays):], exp[:big_n - reps * len(rays)], "g11/large call tail")
    for n in (1, 63, 64, 65, 511, 512, 513):
        got = fz.hit_rays(big_rays[:n])
        assert got.tobytes() == big[:n].tobytes(), f"n = {n} differs from the head of the large call"
    fz.close()


# ------------------------------------------------------------------ ties
def test_tie_scene_later_duplicate_wins(om, oracle):
    """tie_scene: exact duplicates with other materials (test_gpu_edge_cases).  The unit sphere at
    (4,1,0) is added 10 times (ids 122..131): every ray that hits it must report the last copy."""
    w, ow = tie_scene(om, oracle)
    cam = om.default_camera(W / H)
    rays, exp = ray_sets(om, ow, cam, (-6., -0.3, -6.), (6., 2.5, 6.))
    ids = set(int(x) for x in exp["obj"])
    assert 131 in ids and not ids & set(range(122, 131))
    for kernel in ("bvh2", "bvh4", "brute"):
        compare_hits(_query(w, rays, kernel), exp, f"ties/{kernel}")


# ------------------------------------------------------------------ edge rays
EDGE_WINDOWS = [(0.001, 100.0), (5.0, 1.0), (0.001, float("inf")), (0.0, 100.0), (0.0, float("inf"))]


@pytest.fixture(scope="module")
def edge(om, oracle, cache):
    """Rays with NaN / inf components beside ordinary ones, and the oracle's answers for every
    window of EDGE_WINDOWS (computed once, shared by the kernels).  (A ray that is NaN throughout
    keeps `unstuck` stepping to its 2^22-step safety cap in a marched world, about a second for one
    lane: none is used here.)"""
    _, rays, _ = cache.kitchen()
    ow = kitchen_sink(om, oracle)[1]
    nan, inf = F("nan"), F("inf")
    base = rays[[5, 700, 1400, 1600, 2200, len(rays) - 10]].copy()
    odd = np.repeat(base, 2, axis=0)
    odd[0, 0] = nan; odd[1, 4] = nan; odd[2, 1] = inf; odd[3, 3] = -inf; odd[4, 5] = inf; odd[5, 2] = -inf
    odd[6, 0] = nan; odd[6, 4] = inf; odd[7, 3] = nan; odd[7, 5] = nan; odd[8, :3] = inf; odd[9, 4] = nan; odd[10, 2] = nan; odd[11, 3] = inf
    both = np.ascontiguousarray(np.concatenate([odd, rays[::97]]))
    return both, {win: oracle_hits(om, ow, both, *win) for win in EDGE_WINDOWS}


@pytest.mark.parametrize("kernel", ["bvh2", "bvh4", "brute"])
def test_edge_rays(om, cache, edge, kernel):
    """Non-finite ray components; tmin > tmax, tmax = inf, tmin = 0.  obj exact; t, point and
    normal with NaN == NaN (the compare_stats_nan_payload idea)."""
    w = cache.kitchen()[0]
    both, answers = edge
    fz = w.freeze(kernel=kernel)
    for (tmin, tmax), exp in answers.items():
        got = fz.hit_rays(both, tmin, tmax)
        assert np.array_equal(got["obj"], exp["obj"]), f"{kernel} [{tmin}, {tmax}]: obj differs"
        compare_hits(got, exp, f"edge/{kernel} [{tmin}, {tmax}]", nan_payload=True)
    fz.close()


def test_edge_rays_are_edge_cases(edge):
    """From the oracle alone: non-finite rays hit and miss, and infinite components do not always
    give the answer NaN components give (the tree traversals' closed form for NaN rays)."""
    _, answers = edge
    exp = answers[EDGE_WINDOWS[0]]
    odd = exp[:12]
    assert np.isnan(odd["t"]).any() and len(set(odd["obj"].tolist())) >= 2
    assert (answers[(5.0, 1.0)]["obj"][12:] == 0).all()           # tmin > tmax: no finite ray hits


# ------------------------------------------------------------------ entry points
def _params(L, tmin=0.001, tmax=100.0, steps=1024, reserved=0):
    return L.om_query_params(tmin, tmax, steps, reserved)


def test_status_codes(om, cache):
    from raytracingoneweekend_amd import _lib as L
    w, rays, exp = cache.regime("g11")
    some = np.nonzero(exp["obj"])[0][:8]
    r = np.ascontiguousarray(rays[some])
    hits = np.zeros(8, dtype=om.HIT_DTYPE)
    rp, hp = r.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p)
    ctx = C.c_void_p()
    L.check(L.lib.om_create(0, C.byref(ctx)))
    q = _params(L)
    assert L.lib.om_hit_rays(ctx, C.byref(q), rp, 8, hp) == L.OM_ERR_STATE          # before om_upload_world
    assert L.lib.om_hit_rays_device(ctx, C.byref(q), rp, 8, hp, None) == L.OM_ERR_STATE
    L.check(L.lib.om_upload_world(ctx, w.handle), ctx)
    assert L.lib.om_hit_rays(ctx, C.byref(q), rp, 0, hp) == L.OM_OK
    assert L.lib.om_hit_rays(ctx, C.byref(q), None, 0, None) == L.OM_OK             # n == 0 launches nothing
    assert L.lib.om_hit_rays_device(ctx, C.byref(q), None, 0, None, None) == L.OM_OK
    assert not hits.view(np.uint8).any()
    assert L.lib.om_hit_rays(ctx, None, rp, 8, hp) == L.OM_ERR_INVALID
    assert L.lib.om_hit_rays(ctx, C.byref(q), None, 8, hp) == L.OM_ERR_INVALID
    assert L.lib.om_hit_rays(ctx, C.byref(q), rp, 8, None) == L.OM_ERR_INVALID
    assert L.lib.om_hit_rays_device(ctx, C.byref(q), None, 8, None, None) == L.OM_ERR_INVALID
    for bad in (_params(L, reserved=1), _params(L, tmin=float("nan")), _params(L, tmax=float("nan"))):
        assert L.lib.om_hit_rays(ctx, C.byref(bad), rp, 8, hp) == L.OM_ERR_INVALID
        assert L.lib.om_hit_rays_device(ctx, C.byref(bad), rp, 8, hp, None) == L.OM_ERR_INVALID
    assert not hits.view(np.uint8).any()                                           # no failed call wrote a record
    assert L.lib.om_hit_rays(ctx, C.byref(q), rp, 8, hp) == L.OM_OK
    assert hits.tobytes() == exp[some].tobytes()
    L.lib.om_destroy(ctx)


def test_single_ray_mirror(om, cache):
    w, rays, exp = cache.regime("g11")
    fz = w.freeze()
    seen = set()
    for k in (0, 100, 777, 1535, 1600, 3000):
        h = fz.hit(rays[k, :3], rays[k, 3:])
        if exp["obj"][k] == 0:
            assert h is None
        else:
            assert h.obj == exp["obj"][k] and F(h.t) == exp["t"][k]
            assert np.array_equal(h.point, exp["point"][k]) and np.array_equal(h.normal, exp["normal"][k])
            assert w.material_of(h.obj).raw.type in (0, 1, 2)
        seen.add(h is None)
    assert False in seen
    fz.close()


def test_device_entry_point_streams_counters_and_progress(om, cache):
    """Torch tensors through om_hit_rays_device (no host copy) == the host entry point; two queries
    queued back to back on one stream between two om_render_device calls leave renders and queries
    equal to their single runs; counters: segments == n, samples == 0; om_progress untouched."""
    import torch
    from raytracingoneweekend_amd import _lib as L
    w, rays, exp = cache.regime("g11")
    cam = om.default_camera(W / H)
    n = len(rays)
    p = om.make_params(50, 0.001, 100.0, 4, W, H, sample_count=2, seed=11)

    def render_pair(fz, frame, st, between=None):
        L.check(L.lib.om_render_device(fz.ctx, C.byref(cam.raw), C.byref(p), C.c_void_p(frame.data_ptr()), C.c_void_p(st)), fz.ctx)
        out = between() if between else None
        L.check(L.lib.om_render_device(fz.ctx, C.byref(cam.raw), C.byref(p), C.c_void_p(frame.data_ptr()), C.c_void_p(st)), fz.ctx)
        return out

    s = torch.cuda.Stream()
    fz = w.freeze()
    ref_frame = torch.zeros(W * H * 40, dtype=torch.uint8, device="cuda")
    render_pair(fz, ref_frame, s.cuda_stream)
    s.synchronize()
    host = fz.hit_rays(rays)
    compare_hits(host, exp, "g11/host entry point")
    fz.close()

    fz = w.freeze()
    prog = L.lib.om_progress(fz.ctx)
    assert prog and prog[0] == 0
    d_rays = torch.from_numpy(rays).cuda()
    d_rev = torch.from_numpy(np.ascontiguousarray(rays[::-1])).cuda()
    frame = torch.zeros(W * H * 40, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L.check(L.lib.om_reset_counters(fz.ctx, C.c_void_p(s.cuda_stream)), fz.ctx)
    h1 = fz.hit_rays(d_rays, stream=s.cuda_stream)                 # alone: segments == n, samples == 0
    s.synchronize()
    ctr = fz.counters()
    assert ctr["segments"] == n and ctr["samples"] == 0 and ctr["credited"] == 0
    assert ctr["prim_tests"] > 0 and ctr["pre_tests"] > 0 and ctr["march_steps"] == 0
    assert prog[0] == 0

    def two_queries():
        return fz.hit_rays(d_rays, stream=s.cuda_stream), fz.hit_rays(d_rev, stream=s.cuda_stream)

    before = prog[0]
    q1, q2 = render_pair(fz, frame, s.cuda_stream, two_queries)
    s.synchronize()
    assert torch.equal(frame, ref_frame), "renders around the queries differ from the renders alone"
    credited = fz.counters()["credited"]
    assert prog[0] - before == credited == 4 * W * H                # the renders' credit only
    for got, want, label in ((h1, host, "device"), (q1, host, "queued 1"), (q2, host[::-1], "queued 2")):
        g = got.cpu().numpy().view(om.HIT_DTYPE).reshape(-1)
        assert g.tobytes() == np.ascontiguousarray(want).tobytes(), f"{label}: differs from the host entry point"
    # an unaligned record array (4-byte aligned only) takes the scalar load/store path: same records
    pad_r = torch.zeros(n * 6 + 1, dtype=torch.float32, device="cuda")
    pad_h = torch.zeros(n * 8 + 1, dtype=torch.float32, device="cuda")
    pad_r[1:] = d_rays.reshape(-1)
    torch.cuda.synchronize()
    q = _params(L)
    L.check(L.lib.om_hit_rays_device(fz.ctx, C.byref(q), C.c_void_p(pad_r.data_ptr() + 4), n, C.c_void_p(pad_h.data_ptr() + 4),
                                     C.c_void_p(s.cuda_stream)), fz.ctx)
    s.synchronize()
    assert pad_h[1:].cpu().numpy().tobytes() == host.tobytes() and float(pad_h[0]) == 0.0
    fz.close()


def test_torch_default_stream_is_ordered_with_the_query(om, cache):
    """hit_rays(tensor) with no stream= while torch is on its null stream: the rays are computed by
    torch ops queued just before (a long chain, so they are not ready when the call returns to the
    host), the result is read by torch right after, with no synchronise in between.  It must equal
    the host entry point on the same rays."""
    import torch
    w, rays, exp = cache.regime("g11")
    fz = w.freeze()
    host = fz.hit_rays(rays)
    compare_hits(host, exp, "g11/host entry point")
    assert torch.cuda.current_stream().cuda_stream == 0
    src = torch.from_numpy(rays).cuda()
    torch.cuda.synchronize()
    for _ in range(3):
        big = torch.ones((1 << 24,), dtype=torch.float32, device="cuda")
        for _ in range(20):                                       # work queued ahead of the rays' producer
            big = big * 1.0
        d_rays = (src * big[:1]).contiguous()                     # src * 1.0: the same bits, made on the device
        got = fz.hit_rays(d_rays)                                 # no stream=, no synchronise
        flat = got.clone()                                        # a torch reader on the null stream
        assert flat.cpu().numpy().view(om.HIT_DTYPE).reshape(-1).tobytes() == host.tobytes()
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):                                # a non-null current stream is used as it is
        got = fz.hit_rays(src.clone())
        assert got.cpu().numpy().view(om.HIT_DTYPE).reshape(-1).tobytes() == host.tobytes()
    with pytest.raises(ValueError):
        fz.hit_rays(src, stream=0)
    with pytest.raises(ValueError):
        fz.hit_rays(src.cpu().to(torch.float64))
    fz.close()
