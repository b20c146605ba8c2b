"""The ray-ordered LDS copy of the f32 BVH2 nodes decides what the unordered node test decides
(CPU only; DESIGN.md §5.6, raytracingoneweekend_amd/csrc/om_b2_planes.h).

tests/cpp/ordered_planes.cpp freezes every world whose BVH2 is staged in LDS -- the regime worlds
g0, g11, g15, g16, c7x17, c7x18, c8x17 of tests/scenes_common.py REGIME_WORLDS and the ico2 mesh of
tests/mesh_common.py -- rewrites each node as the stager does and runs, for every node, rays of all
eight sign octants, axis-parallel rays with one and two zero components of either sign, rays from
the node's own planes and from inside its boxes, and random rays through both forms of the visit.
The program fails on any difference in h0, h1 or swap, and on any near / far value that is not the
same bits or a zero of the other sign (no compare tells those apart; the report counts them).
This test pins that every world was walked, with both outcomes of every decision seen.
"""
import json
import os
import subprocess

import pytest

import mesh_common as MC
from scenes_common import REGIME_WORLDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
LDS_WORLDS = ["g0", "g11", "g15", "g16", "c7x17", "c7x18", "c8x17"]
MESHES = ["ico2"]


@pytest.fixture(scope="module")
def report(om, tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "Makefile.planes", "ordered_planes"])
    d = tmp_path_factory.mktemp("planes_worlds")
    args = []
    for name in MESHES:
        path = str(d / f"{name}.bin")
        MC.dump(MC.spec(om, name), path)
        args += [name, path]
    out = subprocess.run([os.path.join(CPP, "ordered_planes")] + args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    return {r["world"]: r for r in rows}


def test_every_lds_world_is_walked(report):
    assert set(LDS_WORLDS) <= set(REGIME_WORLDS)
    assert set(LDS_WORLDS + MESHES) == set(report)
    for name, r in report.items():
        assert r["mismatch"] == 0, name
        assert r["zero_sign"] == 0, f"{name}: on these rays near and far are the same bits throughout"
        # 40 octant + 24 two-zero + 24 one-zero directions, from 3 shared and 3 per-node origins, + 96 random rays
        assert r["directions"] == 88 and r["tests"] == r["b2nodes"] * (88 * 6 + 96), name


def test_every_decision_has_both_outcomes(report):
    for name, r in report.items():
        assert r["both"] and r["one"] and r["swaps"] and r["swaps"] < r["both"], name
        if name != "g0":                                  # g0's second box is all of space: never "none"
            assert r["none"], name


def test_one_leaf_tree_stages_its_empty_child_as_all_of_space(report):
    g0 = report["g0"]
    assert g0["b2nodes"] == 1 and g0["inverted_axes"] == 3 and g0["infinite_planes"] == 3
    assert all(r["inverted_axes"] == 0 and r["infinite_planes"] == 0 for n, r in report.items() if n != "g0")
