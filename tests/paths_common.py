"""Helpers of the radiance-query tests (om_ray_color*): the om-rng v2 path stream restated in Python,
and the ray and RNG state with which one sample of the oracle's render enters ray_color.

One pixel, one sample of oracle.render IS ray_color of one ray (render_thread.rs:176-199): the
sample's stream gives two jitter draws, then two draws per try of the lens-disc rejection
(camera.rs:60-65, vec3.rs:108-113), and ray_color goes on with the stream from there.  So for pixel
px of a W x H frame with spp_total = 1 the helper replays the draws of path_state(seed, px, 0),
forms (u, v) in float32 in render_pixel's op order, counts the disc tries, takes the ray from the
oracle's own camera (oro_get_ray with the stream advanced past the jitter) and hands out the state
advanced past 2 + 2 * tries draws.  The expected record is then the oracle's one-sample Stats of
that pixel: sum = 0 + colour, avg_depth = depth, bloom = bloom_hash(first-hit id).  No bounce loop is
restated here.
"""
import ctypes as C

import numpy as np

F = np.float32
M64 = (1 << 64) - 1
WEYL = 0x9E3779B9


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def seed_key(seed):
    return mix64((seed + 0x632BE59BD9B4E019) & M64)


def path_state(seed, pixel, sample):
    """PathRng state of stream (seed, pixel, sample) at its start: low word s, high word k."""
    return mix64(((pixel << 32) | sample) ^ seed_key(seed))


def advance(state, draws):
    """The state after `draws` draws: the Weyl counter moves, the key stays."""
    return (state & ~0xFFFFFFFF & M64) | (((state & 0xFFFFFFFF) + draws * WEYL) & 0xFFFFFFFF)


def draw(state):
    """-> (the next draw as float32, the state after it)"""
    state = advance(state, 1)
    x = (state & 0xFFFFFFFF) ^ (state >> 32)
    x ^= x >> 16
    x = (x * 0x21F0AAAD) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x735A2D97) & 0xFFFFFFFF
    x ^= x >> 15
    return F(x >> 8) * F(5.9604644775390625e-8), state


def camera_path(O, ocam, W, H, seed, px, jt):
    """Ray, ray_color's entry state and the disc tries of sample 0 of pixel px (spp_total = 1)."""
    s0 = path_state(seed, px, 0)
    d0, st = draw(s0)
    d1, st = draw(st)
    line = px // W
    col = px - W * line
    i_rand = (d0 + jt[0, 0]) / F(2.0)                               # render_thread.rs:188-191
    j_rand = (d1 + jt[0, 1]) / F(2.0)
    u = (F(col) + i_rand) / (F(W) - F(1.0))
    v = F(1.0) - (F(line) + j_rand) / (F(H) - F(1.0))
    tries = 0
    while True:                                                     # rand_in_unit_disc, vec3.rs:108-113
        a, st = draw(st)
        b, st = draw(st)
        tries += 1
        x = a * F(2.0) + F(-1.0)
        y = b * F(2.0) + F(-1.0)
        if (x * x + y * y) + F(0.0) < F(1.0):
            break
    out = (C.c_float * 6)()
    O.lib.oro_get_ray(C.byref(ocam), float(u), float(v), C.c_uint64(advance(s0, 2)), O.fp(out))
    assert st == advance(s0, 2 + 2 * tries)
    return np.array(list(out), dtype=F), st, tries


def camera_paths(O, ocam, W, H, seed, pixels=None):
    """camera_path for every listed pixel (default: the frame) -> rays (n, 6) float32, states (n,)
    uint64, tries (n,)."""
    jt = O.jitter_table(seed, 1)
    pixels = range(W * H) if pixels is None else pixels
    rows = [camera_path(O, ocam, W, H, seed, int(px), jt) for px in pixels]
    rays = np.ascontiguousarray(np.stack([r[0] for r in rows]).astype(F))
    states = np.array([r[1] for r in rows], dtype=np.uint64)
    return rays, states, np.array([r[2] for r in rows])


def first_ids(ow, rays, tmin=0.001, tmax=100.0):
    """The id of oracle.World.hit per ray (0: a miss)."""
    ids = np.zeros(len(rays), dtype=np.uint32)
    for k, r in enumerate(rays):
        h = ow.hit(r[:3], r[3:], tmin, tmax)
        ids[k] = 0 if h is None else h[1]
    return ids


def expected_records(om, O, stats, ids):
    """One-sample Stats of the oracle + the first-hit ids -> what om_ray_color must return, with the
    colour as Stats.sum holds it (0 + colour).  Checks bloom == bloom_hash(id) on the way."""
    assert (stats["n"] == 1).all()
    exp = np.zeros(len(stats), dtype=om.RADIANCE_DTYPE)
    exp["color"], exp["depth"], exp["obj"] = stats["sum"], stats["avg_depth"], ids
    blooms = np.array([O.bloom_hash(int(i)) for i in ids], dtype=np.uint64)
    assert np.array_equal(stats["bloom"], blooms), "oracle: bloom of the sample is not bloom_hash(World.hit's id)"
    return exp


def compare_records(got, exp, label):
    """color + 0.0, depth and obj, as bits."""
    g = got.copy()
    g["color"] = g["color"] + F(0.0)                               # Stats.sum = 0 + colour: -0 -> +0
    bad = np.nonzero((g.view(np.uint8).reshape(-1, 20) != exp.view(np.uint8).reshape(-1, 20)).any(axis=1))[0]
    rows = [f"ray {i}: got color={got['color'][i]} depth={got['depth'][i]!r} obj={got['obj'][i]} | "
            f"exp color={exp['color'][i]} depth={exp['depth'][i]!r} obj={exp['obj'][i]}" for i in bad[:5]]
    assert len(bad) == 0, f"{label}: {len(bad)}/{len(got)} records differ\n" + "\n".join(rows)
