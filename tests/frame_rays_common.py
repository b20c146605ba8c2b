"""Helpers of the frame-from-rays tests (om_render_rays*): the rays and RNG states with which every
sample of the oracle's thin-lens render enters ray_color.

paths_common.camera_path does this for sample 0 of a one-sample frame.  Here it is sample s of a
frame with spp_total = S: the stream is path_state(seed, px, s), the jitter row is jt[s] of
O.jitter_table(seed, S), and the float32 operations keep render_pixel's order.  A frame rendered
through om_render_rays from these rays and states must then be oracle.render's frame, bit for bit:
a pixel takes its samples in order, so sample s of the table is the pixel's sample with Stats.n == s
(of a frame that starts from zeroed Stats), whether or not adaptive retirement stops it earlier.
"""
import ctypes as C

import numpy as np

from paths_common import advance, draw, path_state

F = np.float32


def camera_sample(O, ocam, W, H, seed, px, s, jt):
    """Ray and ray_color's entry state of sample s of pixel px; jt is the frame's jitter table."""
    s0 = path_state(seed, px, s)
    d0, st = draw(s0)
    d1, st = draw(st)
    line = px // W
    col = px - W * line
    i_rand = (d0 + jt[s, 0]) / F(2.0)                               # render_thread.rs:188-191
    j_rand = (d1 + jt[s, 1]) / F(2.0)
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
    return np.array(list(out), dtype=F), st


def frame_rays(O, ocam, W, H, seed, S, pixels=None):
    """camera_sample for samples 0 .. S-1 of every listed pixel (default: the frame in row-major
    order) -> rays (S, n, 6) float32, states (S, n) uint64, sample-major as om_render_rays reads them."""
    jt = O.jitter_table(seed, S)
    pixels = list(range(W * H)) if pixels is None else [int(p) for p in pixels]
    rays = np.zeros((S, len(pixels), 6), dtype=F)
    states = np.zeros((S, len(pixels)), dtype=np.uint64)
    for s in range(S):
        for k, px in enumerate(pixels):
            rays[s, k], states[s, k] = camera_sample(O, ocam, W, H, seed, px, s, jt)
    return rays, states


def fold_records(O, stats, records):
    """Stats::add of one om_radiance record per pixel, through the oracle's own add (in place)."""
    col = (C.c_float * 3)()
    for k in range(len(stats)):
        col[0], col[1], col[2] = (float(x) for x in records["color"][k])
        O.lib.oro_stats_add(C.c_void_p(stats[k:k + 1].ctypes.data), O.fp(col), float(records["depth"][k]),
                            C.c_uint64(int(records["obj"][k])))


def differing(got, exp):
    """Indices of the pixels whose 40 bytes differ."""
    g = np.ascontiguousarray(got).view(np.uint8).reshape(-1, 40)
    e = np.ascontiguousarray(exp).view(np.uint8).reshape(-1, 40)
    return np.nonzero((g != e).any(axis=1))[0]


def assert_frames_equal(got, exp, label):
    bad = differing(got, exp)
    rows = [f"pixel {i}: got {got[i]} | exp {exp[i]}" for i in bad[:4]]
    assert len(bad) == 0, f"{label}: {len(bad)}/{len(exp)} pixels differ\n" + "\n".join(rows)
