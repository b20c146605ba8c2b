"""The C++ mirror's ray queries (include/ottomarcher.hpp: FrozenHittableList::hit / hit_rays,
HittableList::material_of), exercised by the compiled driver tests/cpp/test_query.cpp (built by
__graft_entry__.build()).

CPU: material_of in id order and the error statuses that need no device.  GPU: hit_rays over
S-traced, every om_hit record compared byte for byte with the CPU oracle; hit() == the batch."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_query")


@pytest.fixture(scope="module")
def exe(om):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE), "-f", "Makefile.query", "test_query"])
    return EXE


def test_cpp_material_of_and_errors(exe):
    r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "cpu ok" in r.stdout


@pytest.mark.gpu
def test_cpp_hit_rays_match_oracle(exe, om, oracle, tmp_path):
    F = np.float32
    rng = np.random.default_rng(5)
    n = 1500                                              # three workgroups, the last one partial
    orig = (np.array([-12., 0.05, -12.], F) + rng.random((n, 3), dtype=F) * np.array([24., 1.5, 24.], F)).astype(F)
    d = rng.standard_normal((n, 3)).astype(F)
    d = (d / np.sqrt((d * d).sum(axis=1, dtype=F), dtype=F)[:, None]).astype(F)
    rays = np.ascontiguousarray(np.concatenate([orig, d], axis=1), dtype=F)
    rays_in, hits_out = tmp_path / "rays.bin", tmp_path / "hits.bin"
    rays.tofile(rays_in)
    r = subprocess.run([exe, "gpu", str(rays_in), str(hits_out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gpu ok" in r.stdout
    got = np.fromfile(hits_out, dtype=om.HIT_DTYPE)
    ow = oracle.random_scene(0x5EED)
    exp = np.zeros(n, dtype=om.HIT_DTYPE)
    exp["t"] = np.inf
    for k, ray in enumerate(rays):
        h = ow.hit(ray[:3], ray[3:])
        if h is not None:
            exp[k] = (h[0][0], h[0][1:4], h[0][4:7], h[1])
    assert 0 < int((exp["obj"] != 0).sum()) < n and len(set(exp["obj"].tolist())) > 50
    bad = int((got.view(np.uint8).reshape(-1, 32) != exp.view(np.uint8).reshape(-1, 32)).any(axis=1).sum())
    assert bad == 0, f"{bad}/{n} records differ from the oracle"
