"""Where the triangles of the mesh test worlds are kept, and which tree regime each world lands in
(CPU only; the mesh counterpart of test_tree_regimes.py).

From OM_BARY_TREE_MIN triangles + parallelograms on, the builder (om_bvh.cpp select) puts them into the SBVH / BVH2 /
BVH4 leaves beside the spheres and cubes.  tests/test_gpu_mesh.py traces and
renders the worlds of tests/mesh_common.py against the oracle; this test pins, from the host-only
report of tests/cpp/mesh_regimes.cpp on the same numpy arrays, that each of them IS in the regime it
was chosen for: retuning OM_BARY_TREE_MIN, a budget or a leaf cap fails here by name.
"""
import json
import os
import subprocess

import pytest

import mesh_common as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
WORLDS = ["ico2", "ico2x2", "hf48", "below", "degen"]


@pytest.fixture(scope="module")
def report(om, tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "Makefile.mesh", "mesh_regimes"])
    d = tmp_path_factory.mktemp("mesh_worlds")
    args = []
    for name in WORLDS:
        path = str(d / f"{name}.bin")
        MC.dump(MC.spec(om, name), path)
        args += [name, path]
    out = subprocess.run([os.path.join(CPP, "mesh_regimes")] + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    return {r["world"]: r for r in rows}


def test_every_world_is_reported_with_its_primitives(report, om, oracle):
    assert set(WORLDS) == set(report)
    for name in WORLDS:
        w, ow = MC.build(om, oracle, MC.spec(om, name))
        assert sum(w.counts().values()) == report[name]["prims"] == sum(ow.counts())
        assert w.counts()["triangles"] == report[name]["triangles"]
    assert report["ico2"]["bary_tree_min"] == MC.OM_BARY_TREE_MIN


def test_ico2_bvh2_in_lds_with_direct_codes(report):
    r = report["ico2"]
    # (the small ellipsoid, semi-axes 0.03 .. 0.05, is a thin sphere: outside the trees like the ground)
    assert r["triangles"] == 320 and r["rec_bary"] == 320 and r["rec_other"] == 3, "ground and the small ellipsoid outside, 2 ellipsoids + cube inside"
    assert r["always2"] == 2
    assert r["always_tri_boxed"] == 0 and r["always_tri_unbounded"] == 0
    assert r["b2_ok"] == 1 and r["b2_lds_bytes"] != 0 and r["b2_direct"] == 1
    assert r["b4_ok"] == 1 and r["b4_lds_bytes"] != 0 and r["lds_bytes"] != 0, "BVH4 and the megakernel's SBVH staged too"


def test_ico2x2_every_triangle_has_its_duplicate_in_the_tree(report):
    r = report["ico2x2"]
    assert r["triangles"] == 640 and r["rec_bary"] == 640
    assert r["b2_ok"] == 1 and r["b2_lds_bytes"] != 0 and r["b2_direct"] == 1


def test_hf48_leaf_table_and_half_nodes_through_l2(report):
    r = report["hf48"]
    assert r["triangles"] == 4608 and r["rec_bary"] == 4608 and r["srecs"] >= 2048
    assert r["b2_ok"] == 1 and r["b2_direct"] == 0, "leaf table expected"
    assert r["b2_lds_bytes"] == 0, "tree expected past the LDS budget: read through L2 with half-precision nodes"
    assert r["max_leaf"] == 1, "L2 trees are built with one record per leaf"
    assert r["b4_ok"] == 1 and r["b4_lds_bytes"] == 0
    assert r["nonfinite_planes"] == 0


def test_leaves_mix_kinds(report):
    """Some leaf of a staged tree holds a triangle beside a sphere or the cube (leaves of up to 8)."""
    assert report["ico2"]["mixed_leaves"] + report["ico2x2"]["mixed_leaves"] + report["degen"]["mixed_leaves"] >= 1


def test_below_the_threshold_keeps_the_always2_layout(report):
    r = report["below"]
    assert r["triangles"] == MC.OM_BARY_TREE_MIN - 1
    assert r["rec_bary"] == 0 and r["srecs"] == r["rec_other"] == 3, "no barycentric record in srecs (2 ellipsoids + cube)"
    assert r["always_tri_boxed"] == r["triangles"] and r["always_tri_unbounded"] == 0, "all of them in always2 with boxes"
    assert r["always2"] == r["triangles"] + 2, "the ground, the small ellipsoid (a thin sphere) and the triangles"


def test_degenerate_triangle_stays_outside_unbounded(report):
    r = report["degen"]
    assert r["triangles"] == 33
    assert r["rec_bary"] == 32, "the 32 good triangles are in the tree"
    assert r["always_tri_unbounded"] == 1 and r["always_tri_boxed"] == 0, "the degenerate one: always2, unbounded"
    assert r["nonfinite_planes"] == 0, "no cull sees a NaN"
