"""The refit of om_update_triangles, on the CPU (no GPU): tests/cpp/refit_check.cpp loops the
OM_HD functions of csrc/om_refit.h, the ones the kernels of om_refit.hip run one thread per
element, over frozen worlds of tests/mesh_common.py and their refit tables.

Per world, from the same numpy arrays as every other mesh test (mesh_common.dump):
  (a) an update with the original vertices leaves every array of every layout byte-identical;
  (b) after the displacement of tests/refit_common.py every rewritten OmBary equals the record of a
      fresh freeze of the moved world byte for byte, every box of every layout contains the boxes of
      all records beneath it, each half plane lies outside the f32 plane it was rounded from;
  (c) a collapsed face takes the all-covering box and no plane anywhere is NaN;
  (d) a NaN vertex: its faces are counted and take the covering box in the leaf-record tree, records
      and primitive boxes equal a fresh freeze's of the same world, no plane is NaN.
ico2x2 moves its second mesh only (first = 320).
"""
import json
import os
import subprocess

import pytest

import mesh_common as MC
import refit_common as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def _run(om, tmp_path_factory, target):
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "Makefile.refit", target])
    d = tmp_path_factory.mktemp("refit_worlds")
    args = []
    for name in RC.WORLDS:
        items, moved, first, _, _ = RC.moved_spec(om, name)
        a, b = str(d / f"{name}.bin"), str(d / f"{name}_moved.bin")
        MC.dump(items, a)
        MC.dump(moved, b)
        args += [name, a, b, str(first)]
    return subprocess.run([os.path.join(CPP, target)] + args, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def report(om, tmp_path_factory):
    out = _run(om, tmp_path_factory, "refit_check")
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    return out, {r["world"]: r for r in rows}


def test_every_check_of_every_world_passes(report):
    out, rows = report
    fails = [l for l in out.stdout.splitlines() if l.startswith("FAIL")]
    assert out.returncode == 0 and not fails, "\n".join(fails[:20]) + out.stderr[-2000:]
    assert set(rows) == set(RC.WORLDS)


def test_the_worlds_are_the_cases_they_stand_for(report, om):
    _, rows = report
    assert rows["ico2x2"]["first"] == 320 and rows["ico2x2"]["triangles"] == 320, "the second copy only"
    assert rows["ico2"]["in_tree"] == 1 and rows["hf48"]["in_tree"] == 1 and rows["degen"]["in_tree"] == 1
    assert rows["below"]["in_tree"] == 0, "under OM_BARY_TREE_MIN the triangles stay outside with their boxes"
    assert rows["degen"]["unbounded_identity"] == 1 and rows["degen"]["unbounded_moved"] == 1, "its own repeated-index face"
    for name in ("ico2", "hf48", "below", "ico2x2"):
        assert rows[name]["unbounded_moved"] == 0 and rows[name]["unbounded_collapsed"] == 1
    assert rows["hf48"]["boxes_checked"] >= 4 * 4608 and rows["hf48"]["halves_checked"] >= 12 * 4608
    assert rows["hf48"]["levels"] >= 12
    assert all(rows[n]["nan_vertex_faces"] >= 1 for n in RC.WORLDS)


def test_the_same_checks_under_the_sanitizers(om, tmp_path_factory):
    """refit_check built with ASan + UBSan as its own executable: host code only."""
    out = _run(om, tmp_path_factory, "refit_check_san")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
