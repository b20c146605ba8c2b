"""The C++ mirror's frames from caller-given rays (include/ottomarcher.hpp:
FrozenHittableList::render_rays), exercised by the compiled driver tests/cpp/test_render_rays.cpp
(built by __graft_entry__.build()).

CPU: the error statuses that need no device.
GPU: the adaptive 12-spp frame of S-traced at 20x13 from the thin-lens camera's own rays
(tests/frame_rays_common.py), every om_pixel_stats compared as bytes with the oracle's render; the
driver itself checks that calls of one sample, small batches and a pixel list give the same frame."""
import os
import subprocess

import numpy as np
import pytest

from frame_rays_common import assert_frames_equal, frame_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_render_rays")


@pytest.fixture(scope="module")
def exe(om):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE), "-f", "Makefile.rays", "test_render_rays"])
    return EXE


def test_cpp_errors_without_a_device(exe):
    r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "cpu ok" in r.stdout


@pytest.mark.gpu
def test_cpp_render_rays_matches_oracle(exe, om, oracle, tmp_path):
    W, H, seed, spp = 20, 13, 7, 12
    ow, ocam = oracle.random_scene(0x5EED), oracle.default_camera(W / H)
    rays, states = frame_rays(oracle, ocam, W, H, seed, spp)
    rec = np.zeros(spp * W * H, dtype=np.dtype([("ray", "<f4", (6,)), ("state", "<u8")]))
    rec["ray"], rec["state"] = rays.reshape(-1, 6), states.reshape(-1)
    rays_in, stats_out = tmp_path / "rays.bin", tmp_path / "stats.bin"
    rec.tofile(rays_in)
    r = subprocess.run([exe, "gpu", str(W), str(H), str(spp), str(rays_in), str(stats_out)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gpu ok" in r.stdout
    got = np.fromfile(stats_out, dtype=oracle.PIXEL_STATS_DTYPE)
    exp, _ = oracle.render(ow, ocam, oracle.params(W, H, spp, seed=seed, adaptive=True))
    assert_frames_equal(got, exp, "cpp/g11 adaptive")
