"""Which tree regime each regime world of tests/scenes_common.py REGIME_WORLDS lands in (CPU only).

The traversal code a world runs is picked by size thresholds: BVH2 staged whole in LDS or read
through L2 (om::plan_trees, om_world.h; kB2LdsBudget), direct leaf codes or the leaf table (fewer
than 2048 records and leaves of at most 15, om_bvh.cpp), the max-leaf fallback tree from 32768
primitives, the BVH4 cut (kB4LdsBudget) and the megakernel's staged SBVH (kLdsBudget).
tests/test_gpu_tree_regimes.py renders one world per regime against the oracle; this test pins,
from the host-only report of tests/cpp/tree_regimes.cpp, that each of those worlds still IS in
the regime it was chosen for.  Retuning OM_B2_NODE_STRIDE, a budget or the leaf caps makes it
fail and name the regime that lost its world, instead of the GPU coverage silently moving.
It asserts regimes, not node counts.
"""
import json
import os
import subprocess

import pytest

from scenes_common import REGIME_WORLDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.fixture(scope="module")
def report():
    subprocess.check_call(["make", "-s", "-C", CPP, "tree_regimes"])
    out = subprocess.run([os.path.join(CPP, "tree_regimes")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    budgets = [r for r in rows if "budgets" in r][0]
    return budgets, {r["world"]: r for r in rows if "world" in r}


def test_every_rendered_world_is_reported(report):
    _, worlds = report
    assert set(REGIME_WORLDS) <= set(worlds), sorted(set(REGIME_WORLDS) - set(worlds))


def test_python_cluster_worlds_hold_the_reported_primitives(report, om, oracle):
    """tests/scenes_common.py cluster_world adds what the program's cluster_world adds."""
    _, worlds = report
    for name in ("c7x17", "c7x18", "c8x17"):
        w, ow = REGIME_WORLDS[name][0](om, oracle)
        assert w.counts()["spheres"] == worlds[name]["prims"] == sum(ow.counts())


def test_ground_only_has_no_bvh2(report):
    _, w = report
    assert w["g0x"]["b2_ok"] == 0 and w["g0x"]["b2nodes"] == 0 and w["g0x"]["srecs"] == 0, "ground only: reference loop"


def test_single_leaf_tree(report):
    _, w = report
    g0 = w["g0"]
    assert g0["b2_ok"] == 1 and g0["b2nodes"] == 1 and g0["b2leaves"] == 2, "one node, a leaf and an empty second child"
    assert g0["leaf_hist"].get("0") == 1, "the second child is an empty leaf"


@pytest.mark.parametrize("name", ["g16", "c8x17"])
def test_bvh2_in_lds_at_the_budget_edge(report, name):
    b, w = report
    assert w[name]["b2_lds_bytes"] != 0, f"{name}: BVH2 no longer staged in LDS"
    assert w[name]["b2_lds_bytes"] >= 0.9 * b["kB2LdsBudget"], f"{name}: no longer at the edge of kB2LdsBudget"
    # the request of such a tree: nodes kB2Stride apart + leaf table + one lane stack per lane
    assert w[name]["staged_bytes"] == w[name]["b2nodes"] * b["kB2Stride"] + w[name]["b2leaves"] * 4
    assert w[name]["wf_lds_request"] <= 160 * 1024


def test_first_l2_tree_has_direct_codes(report):
    _, w = report
    assert w["g17"]["b2_ok"] == 1 and w["g17"]["b2_lds_bytes"] == 0 and w["g17"]["b2_direct"] == 1


def test_l2_direct_codes_near_the_11_bit_limit(report):
    _, w = report
    assert w["g22"]["b2_ok"] == 1 and w["g22"]["b2_lds_bytes"] == 0
    assert w["g22"]["b2_direct"] == 1 and w["g22"]["max_first"] >= 1024, "top bit of the direct code's `first` unused"


def test_first_l2_tree_with_a_leaf_table(report):
    _, w = report
    assert w["g23"]["b2_ok"] == 1 and w["g23"]["b2_direct"] == 0 and w["g23"]["b2_lds_bytes"] == 0


def test_lds_direct_codes_with_full_leaves(report):
    _, w = report
    c = w["c7x17"]
    assert c["b2_ok"] == 1 and c["b2_lds_bytes"] != 0 and c["b2_direct"] == 1
    assert c["max_leaf"] >= 7 and any(int(k) >= 7 for k in c["leaf_hist"]), "no leaf of >= 7 records"
    assert c["max_first"] >= 1024, "top bit of the direct code's `first` unused"


def test_lds_with_a_leaf_table(report):
    _, w = report
    c = w["c7x18"]
    assert c["b2_ok"] == 1 and c["b2_direct"] == 0 and c["b2_lds_bytes"] != 0
    assert c["max_first"] >= 2048
    assert w["c8x17"]["b2_direct"] == 0, "c8x17: LDS + table at the budget edge"


def test_fallback_tree_from_32768_primitives(report):
    _, w = report
    g = w["g91x"]
    assert g["prims"] >= 32768
    assert g["b2_ok"] == 1 and g["b2nodes"] < 32768 and g["b2leaves"] < 32768
    assert g["max_leaf"] > 1, "one-record leaves: not the max-leaf fallback tree"
    assert g["b2_lds_bytes"] == 0 and g["b2_direct"] == 0


def test_tested_scenes_keep_their_regimes(report):
    """S-traced: LDS + direct; S-10k: L2 + table."""
    _, w = report
    assert w["g11"]["b2_lds_bytes"] != 0 and w["g11"]["b2_direct"] == 1
    assert w["g50x"]["b2_ok"] == 1 and w["g50x"]["b2_lds_bytes"] == 0 and w["g50x"]["b2_direct"] == 0


def test_bvh4_cut_has_a_world_on_each_side(report):
    b, w = report
    rendered = [w[n] for n in REGIME_WORLDS]
    near = [r["world"] for r in rendered if r["b4_lds_bytes"] >= 0.9 * b["kB4LdsBudget"]]
    assert {"g16", "c8x17"} <= set(near), f"BVH4 in LDS at >= 90 % of its budget: only {near}"
    assert w["g17"]["b4_ok"] == 1 and w["g17"]["b4_lds_bytes"] == 0, "g17: BVH4 expected past its LDS cut"
    assert all(r["b4_ok"] == 1 for r in rendered if r["b2_ok"]), "a regime world lost its BVH4"


def test_megakernel_staging_cut_has_a_world_on_each_side(report):
    """g15 / g16 straddle kLdsBudget: the pair test_gpu_tree_regimes.py renders under sbvh / culled."""
    b, w = report
    assert w["g15"]["lds_bytes"] != 0 and w["g15"]["lds_bytes"] >= 0.9 * b["kLdsBudget"]
    assert w["g16"]["lds_bytes"] == 0 and w["g16"]["srecs"] != 0


def test_scaled_child_codes_stay_node_codes(report):
    """stage_scene multiplies a child index by kB2Stride / 16: for every world staged in LDS the
    largest scaled index stays below OM_LEAF (0x8000)."""
    b, w = report
    for r in w.values():
        if r["b2_lds_bytes"]:
            assert (r["b2nodes"] - 1) * (b["kB2Stride"] // 16) < 0x8000, r["world"]


def test_largest_admitted_lds_request_fits_a_workgroup(report):
    """The budget counts 64 B per node, the wavefront stages kB2Stride: the largest tree the budget
    admits, with the deepest lane stack (24 entries of 2 B per lane), must fit the 160 KiB of LDS a
    gfx950 workgroup can use; and no reported world asks for more than that bound."""
    b, w = report
    bound = b["kB2LdsBudget"] * b["kB2Stride"] // 64 + 24 * 2 * b["wf_block"]
    assert bound <= 160 * 1024
    assert all(r["wf_lds_request"] <= bound for r in w.values())


def test_builder_depth_bound_holds_on_a_geometric_line(report):
    """4000 spheres on a line with geometrically growing gaps and radii: SAH peels the far end off
    level after level, the builder's switch to median splits at depth 10 must keep the tree within
    the 24-entry lane stack -- otherwise the wavefront drops to the scratch-stack BVH.  (The line spans
    e^6, radii 0.094 to 38: what the builder keeps in its trees; it spanned e^16 before thin spheres left them.)"""
    _, w = report
    ln = w["line4000"]
    assert ln["srecs"] == 4000
    assert ln["b2_ok"] == 1, "BVH2 refused: the wavefront would fall back to the global-memory BVH"
    assert ln["b2_depth"] <= 24
