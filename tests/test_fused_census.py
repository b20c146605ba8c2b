"""The census behind the fused bounce-0/1 launch, on the host (CPU only).

tests/cpp/fused_census.cpp counts, with the oracle's ray_color, how many paths of each of bounce 0's
64-sample blocks (om_deal.h's numbering: one wave iteration of k_bounce<FIRST>) go on to bounce 1:
the share of blocks with no survivor (their waves skip the fused second trace), the survivors per
non-empty block and the lane occupancy of the fused trace.  The benchmark-shaped run (1920x1080, one
16-spp batch, every 7th block) is recorded in profiles/fused_b01/census.jsonl.

Here, at 480x270 and 2 spp over every block, the test pins only that the tool runs, that its numbers
are consistent with each other, and that its survivors are the paths tests/cpp/segment_census.cpp
counts at bounce 1 for the same frame (both from the bit-exact oracle, so the integers are equal).
"""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def _run(makefile, target, *args):
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", makefile, target])
    out = subprocess.run([os.path.join(CPP, target), *args], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]


@pytest.fixture(scope="module")
def fused():
    return _run("Makefile.fused", "fused_census", "480", "270", "2", "1")


def test_fused_census_is_consistent(fused):
    head, row = fused
    assert head["frame"] == [480, 270] and head["paths"] == 480 * 270 * 2
    assert head["blocks"] == head["counted_blocks"] == (head["paths"] + 63) // 64
    assert row["empty_blocks"] + row["nonempty_blocks"] == head["counted_blocks"]
    assert sum(row["survivors_hist_by_8"]) == row["nonempty_blocks"]
    assert row["full_blocks"] <= row["survivors_hist_by_8"][-1]
    assert row["nonempty_blocks"] <= head["survivors"] <= 64 * row["nonempty_blocks"]
    print(f"empty blocks {row['empty_share']}, survivors per non-empty block {row['mean_survivors']}, "
          f"fused lane occupancy {row['fused_lane_occupancy']}")
    assert abs(row["fused_lane_occupancy"] - head["survivors"] / (64 * row["nonempty_blocks"])) < 1e-4


def test_survivors_are_segment_census_bounce_1(fused):
    head, _ = fused
    rows = _run("Makefile.deal", "segment_census", "480", "270", "2", "1", "1")
    bounce1 = next(r for r in rows[1:] if r["bounce"] == 1)
    assert rows[0]["paths"] == head["paths"]
    assert head["survivors"] == bounce1["paths"]
    assert abs(head["survivor_share"] - bounce1["paths"] / rows[0]["paths"]) < 1e-4
