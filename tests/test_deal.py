"""Bounce 0's deal of the camera samples over the workgroups (csrc/om_deal.h), on the
host (CPU only).

* tests/cpp/deal_bijection.cpp checks the helper the kernels and the host sizing share, exhaustively
  over paths in {0, 1, 63, 64, 65, 64 nseg - 1, 64 nseg, 64 nseg + 1, 64 (3 nseg + 5) + 17}, nseg in
  {1, 2, 48} and D in {1, 2, 4, 8} (and the shipped D): every sample index is produced exactly once
  over all (workgroup, block), each workgroup's share fits the capacity the host sizes the segments
  with, and a workgroup's blocks rise.
* tests/cpp/segment_census.cpp counts, with the oracle's ray_color, how many paths each queue segment
  holds per bounce when bounce 0 fills the segments with contiguous sample ranges and when it deals
  64-sample blocks round-robin.  Here at 480x270, 2 spp, with the library's own batch and segment
  formulas (a 2-spp call on the default two streams is two 1-spp batches of 254 segments): the dealt
  order's max / mean must be below the contiguous order's at bounces 1-4.  Both tables are recorded in
  profiles/even_deal/census_480x270.jsonl; the counts are integers of a bit-exact oracle, so the
  record is the same on every machine, and the test compares it when the file exists.
"""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
RECORD = os.path.join(ROOT, "profiles", "even_deal", "census_480x270.jsonl")


def _run(target, *args):
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "Makefile.deal", target])
    out = subprocess.run([os.path.join(CPP, target), *args], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


def test_deal_helper_is_a_bijection_within_capacity():
    out = _run("deal_bijection")
    lines = out.splitlines()
    assert lines[-1] == "all ok", out[-2000:]
    # 3 nseg x 9 path counts x (4 + the shipped D) cases, each reported
    assert sum(1 for l in lines if l.endswith(" ok") and l.startswith("paths ")) == 3 * 9 * 5


@pytest.fixture(scope="module")
def census():
    out = _run("segment_census", "480", "270", "2", "1", "1")      # every pixel, blocks dealt one by one, two streams
    rows = [json.loads(l) for l in out.splitlines() if l.startswith("{")]
    head, bounces = rows[0], {r["bounce"]: r for r in rows[1:]}
    os.makedirs(os.path.dirname(RECORD), exist_ok=True)
    if os.path.exists(RECORD):
        with open(RECORD) as f:
            assert [json.loads(l) for l in f if l.startswith("{")] == rows, "the census no longer gives the recorded tables"
    else:
        with open(RECORD, "w") as f:
            f.write(out)
    return head, bounces


def test_census_runs_the_library_shapes(census):
    head, bounces = census
    assert head["batches"] == 2 and head["batch_spp"] == 1 and head["nseg"] == 254 and head["segcap"] == 512
    assert bounces[1]["paths"] > bounces[2]["paths"] > bounces[4]["paths"] > 0


@pytest.mark.parametrize("bounce", [1, 2, 3, 4])
def test_dealt_segments_are_more_even(census, bounce):
    _, bounces = census
    r = bounces[bounce]
    print(f"bounce {bounce}: contiguous {r['contiguous']}, dealt {r['dealt']}")
    assert r["dealt"]["max_mean"] < r["contiguous"]["max_mean"]
    assert r["dealt"]["nonempty"] >= r["contiguous"]["nonempty"]
