"""The C++ mirror's update_triangles / update_info (include/ottomarcher.hpp), exercised by the
compiled driver tests/cpp/test_refit.cpp (built by __graft_entry__.build()).

CPU: HittableList::update_triangles == a world built from the new vertices, all-or-nothing, the
statuses that need no device.  GPU: an icosphere frozen, moved through
FrozenHittableList::update_triangles (refit_common.deform_ico) and traced: every om_hit record equals
the CPU oracle's for a world built from the moved vertices, byte for byte."""
import os
import struct
import subprocess

import numpy as np
import pytest

import mesh_common as MC
import refit_common as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_refit")


@pytest.fixture(scope="module")
def exe(om):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE), "-f", "Makefile.refitapi", "test_refit"])
    return EXE


def test_cpp_host_update_and_errors(exe):
    r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "cpu ok" in r.stdout


@pytest.mark.gpu
def test_cpp_update_then_hit_rays_match_oracle(exe, om, oracle, tmp_path):
    from scenes_common import oracle_hits, pinhole_rays
    from test_gpu_query import compare_hits
    F = np.float32
    v, f = MC.icosphere(2, (0., 1., 0.), 1.0)
    nv = RC.deform_ico(v)
    cam = om.Camera.new((3.2, 2.0, 4.0), (0., 1., 0.), (0., 1., 0.), 35., 1.5, 0.0, 5.0)
    rays = np.ascontiguousarray(pinhole_rays(cam))
    ow = oracle.World()
    ow.add_sphere_radius((0., -1000., 0.), 1000., oracle.material("lambertian", (0.5, 0.5, 0.5)))
    for a, b, c in f:
        ow.add_triangle(nv[a], nv[b], nv[c], oracle.material("lambertian", (0.2, 0.4, 0.9)))
    exp = oracle_hits(om, ow, rays)
    assert len(set(exp["obj"].tolist())) >= 100, "the rays reach the moved mesh"
    mesh_in, rays_in, hits_out = tmp_path / "mesh.bin", tmp_path / "rays.bin", tmp_path / "hits.bin"
    with open(mesh_in, "wb") as fh:
        fh.write(struct.pack("<II", len(v), len(f)) + v.astype("<f4").tobytes() + nv.astype("<f4").tobytes() + f.astype("<u4").tobytes())
    rays.astype(F).tofile(rays_in)
    r = subprocess.run([exe, "gpu", str(mesh_in), str(rays_in), str(hits_out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(hits_out, dtype=om.HIT_DTYPE)
    compare_hits(got, exp, "C++ update_triangles + hit_rays")
