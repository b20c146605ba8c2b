"""The C++ mirror's radiance queries (include/ottomarcher.hpp: FrozenHittableList::ray_color),
exercised by the compiled driver tests/cpp/test_paths.cpp (built by __graft_entry__.build()).

CPU: record layouts, om_path_rng_state's advance rule and the error statuses that need no device.
GPU: ray_color over S-traced for the camera paths of a 48x32 frame, every om_radiance record compared
as bits with the oracle's one-sample render (tests/paths_common.py)."""
import os
import subprocess

import numpy as np
import pytest

from paths_common import camera_paths, compare_records, expected_records, first_ids

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_paths")


@pytest.fixture(scope="module")
def exe(om):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE), "-f", "Makefile.paths", "test_paths"])
    return EXE


def test_cpp_layouts_and_errors(exe):
    r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "cpu ok" in r.stdout


@pytest.mark.gpu
def test_cpp_ray_color_matches_oracle(exe, om, oracle, tmp_path):
    W, H, seed = 48, 32, 7
    ow, ocam = oracle.random_scene(0x5EED), oracle.default_camera(W / H)
    rays, states, _ = camera_paths(oracle, ocam, W, H, seed)
    rec = np.zeros(len(rays), dtype=np.dtype([("ray", "<f4", (6,)), ("state", "<u8")]))
    rec["ray"], rec["state"] = rays, states
    paths_in, records_out = tmp_path / "paths.bin", tmp_path / "records.bin"
    rec.tofile(paths_in)
    r = subprocess.run([EXE, "gpu", str(paths_in), str(records_out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gpu ok" in r.stdout
    got = np.fromfile(records_out, dtype=om.RADIANCE_DTYPE)
    stats, _ = oracle.render(ow, ocam, oracle.params(W, H, 1, seed=seed))
    compare_records(got, expected_records(om, oracle, stats, first_ids(ow, rays)), "cpp/g11")
