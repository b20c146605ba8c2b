"""The C++ mirror's any-hit queries and per-ray windows (include/ottomarcher.hpp:
FrozenHittableList::occluded / occluded_rays / hit_rays with windows), exercised by the compiled
driver tests/cpp/test_occlusion.cpp (built by __graft_entry__.build(), or here when missing).

CPU: the record size and the error statuses that need no device.  GPU: occluded_rays and hit_rays
over S-traced with 1500 random rays, each with its own window, compared exactly with the CPU
oracle's hit(ray, tmin_i, tmax_i); occluded() == the batch form (checked inside the driver)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_occlusion")


@pytest.fixture(scope="module")
def exe(om):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE), "-f", "Makefile.occlusion", "test_occlusion"])
    return EXE


def test_cpp_null_arguments(exe):
    r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "cpu ok" in r.stdout


@pytest.mark.gpu
def test_cpp_occluded_rays_match_oracle(exe, om, oracle, tmp_path):
    F = np.float32
    rng = np.random.default_rng(6)
    n = 1500                                              # three workgroups, the last one partial
    orig = (np.array([-12., 0.05, -12.], F) + rng.random((n, 3), dtype=F) * np.array([24., 1.5, 24.], F)).astype(F)
    d = rng.standard_normal((n, 3)).astype(F)
    d = (d / np.sqrt((d * d).sum(axis=1, dtype=F), dtype=F)[:, None]).astype(F)
    rays = np.ascontiguousarray(np.concatenate([orig, d], axis=1), dtype=F)
    # windows [0.001, tmax_i], tmax_i log-uniform in [0.05, 50]: most closest roots of these rays lie
    # in that range, so the windows cut on both sides of them
    win = np.zeros(n, dtype=om.WINDOW_DTYPE)
    win["tmin"] = F(0.001)
    win["tmax"] = np.exp(rng.uniform(np.log(0.05), np.log(50.0), n)).astype(F)
    paths = [tmp_path / x for x in ("rays.bin", "windows.bin", "occ.bin", "hits.bin")]
    rays.tofile(paths[0])
    win.tofile(paths[1])
    r = subprocess.run([exe, "gpu"] + [str(p) for p in paths], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gpu ok" in r.stdout
    got = np.fromfile(paths[2], dtype=np.uint8)
    hits = np.fromfile(paths[3], dtype=om.HIT_DTYPE)
    ow = oracle.random_scene(0x5EED)
    exp = np.zeros(n, dtype=om.HIT_DTYPE)
    exp["t"] = np.inf
    full = np.zeros(n, dtype=bool)
    for k, ray in enumerate(rays):
        h = ow.hit(ray[:3], ray[3:], win["tmin"][k], win["tmax"][k])
        if h is not None:
            exp[k] = (h[0][0], h[0][1:4], h[0][4:7], h[1])
        full[k] = ow.hit(ray[:3], ray[3:]) is not None
    occ = exp["obj"] != 0
    print(f"{int(occ.sum())} of {n} occluded inside their window, {int(full.sum())} hit in [0.001, 100]")
    assert 0 < int(occ.sum()) < int(full.sum()) < n        # the windows decide rays
    assert set(got.tolist()) <= {0, 1}
    assert np.array_equal(got != 0, occ), f"{int(((got != 0) != occ).sum())}/{n} rays differ from the oracle"
    bad = int((hits.view(np.uint8).reshape(-1, 32) != exp.view(np.uint8).reshape(-1, 32)).any(axis=1).sum())
    assert bad == 0, f"{bad}/{n} windowed records differ from the oracle"
