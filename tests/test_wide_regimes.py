"""Which worlds get the wide BVH2 (32-bit child codes), and that it is the same
tree as the 16-bit one (CPU only; the counterpart of test_mesh_regimes.py around the 15-bit limit).

tests/cpp/wide_regimes.cpp freezes the worlds of tests/wide_common.py and the small mesh worlds of
tests/mesh_common.py on the host, walks b2h and the wide nodes in lockstep, checks every wide tree
(each record in exactly one leaf, every decoded child box around the records below it, no non-finite
plane) and prints one JSON line per world; this test pins the regimes by name and checks that
om_world_tree_info, through the library, reports the same.
"""
import ctypes as C
import json
import os
import shutil
import subprocess

import pytest

import mesh_common as MC
import wide_common as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
SMALL = ["ico2", "hf48", "degen"]
LARGE = ["W15", "W15P", "W16P"]
NONE, LDS, L2, WIDE, FALLBACK = range(5)                      # OM_TREE_*
INFO_FIELDS = ["records", "always_tested", "b2_nodes", "b2_leaves", "b2_depth", "b2_max_leaf", "regime", "lds_bytes"]


def _spec(om, name):
    return MC.spec(om, name) if name in SMALL else WC.spec(om, name)


@pytest.fixture(scope="module")
def report(om, tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "Makefile.wide", "wide_regimes"])
    d = tmp_path_factory.mktemp("wide_worlds")
    args = []
    for name in SMALL + LARGE:
        path = str(d / f"{name}.bin")
        MC.dump(_spec(om, name), path)
        args += [name, path]
    out = subprocess.run([os.path.join(CPP, "wide_regimes")] + args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    return {r["world"]: r for r in rows}


def test_every_world_is_reported_and_walked(report):
    assert set(SMALL + LARGE) == set(report)
    for name, r in report.items():
        assert r["b2w_ok"] == 1 and r["b2w_nodes"] == r["b2nodes"], f"{name}: wide nodes for every world with a BVH2"
        assert r["records_once"] == r["srecs"], f"{name}: each record in exactly one leaf"
        assert r["bad_planes"] == 0 and r["bad_boxes"] == 0, name
        assert r["max_leaf"] <= 15 and r["b2w_depth"] == r["b2w_stack"] <= r["wide_stack_bound"], name
        if r["b2_ok"]:
            assert r["lockstep_nodes"] == r["b2nodes"], f"{name}: b2h and the wide nodes are one tree"


def test_small_worlds_keep_their_regime(report):
    assert report["ico2"]["b2_ok"] == 1 and report["ico2"]["b2_lds_bytes"] != 0 and report["ico2"]["regime"] == LDS
    assert report["degen"]["b2_ok"] == 1 and report["degen"]["b2_lds_bytes"] != 0 and report["degen"]["regime"] == LDS
    r = report["hf48"]
    assert r["b2_ok"] == 1 and r["b2_lds_bytes"] == 0 and r["b2_direct"] == 0 and r["regime"] == L2


def test_w15_is_the_last_world_within_the_15_bit_codes(report):
    r = report["W15"]
    assert r["triangles"] == 2 * WC.N["W15"] ** 2
    assert r["b2_ok"] == 1 and r["b2_lds_bytes"] == 0 and r["regime"] == L2
    assert 32768 - 200 < r["b2leaves"] < 32768, "chosen at the limit"
    assert r["b2w_ok"] == 1, "wide nodes present too"


def test_w15p_is_past_the_15_bit_codes_and_wide(report):
    """Fails without the wide regime: such a world had b2_ok 0 and nothing else."""
    r = report["W15P"]
    assert r["triangles"] == 2 * WC.N["W15P"] ** 2
    assert r["b2_ok"] == 0 and 32768 <= r["b2leaves"] < 32768 + 400, "just past the limit"
    assert r["b2w_ok"] == 1 and r["regime"] == WIDE
    assert r["walk_leaves"] == r["b2leaves"]
    # the u32 lane stack of 512 lanes, no node prefix (OM_WF_HYBW_BYTES = 0, measured: DESIGN.md §5.18)
    assert r["lds_bytes"] == 512 * 4 * r["b2w_stack"]


def test_w16p_is_past_16_bits(report):
    r = report["W16P"]
    assert r["b2nodes"] > 65536 and r["srecs"] > 65536, "a u16 stack entry or record index would truncate"
    assert r["b2_ok"] == 0 and r["b2w_ok"] == 1 and r["regime"] == WIDE
    assert r["info_depth"] == r["b2w_depth"], "the depth reported is the wide emission's (16-bit codes collide here)"


def test_library_reports_the_same(report, om):
    """om_world_tree_info through libottomarcher.so == the host driver's, for one world of each regime."""
    for name in ["ico2", "hf48", "W15P"]:
        w = WC.build_product(om, _spec(om, name))
        ti, r = w.tree_info(), report[name]
        assert ti["records"] == r["srecs"] and ti["always_tested"] == r["always2"]
        assert ti["b2_nodes"] == r["b2nodes"] and ti["b2_leaves"] == r["b2leaves"]
        assert ti["b2_depth"] == r["info_depth"] and ti["b2_max_leaf"] == r["max_leaf"]
        assert ti["regime"] == ("none", "lds", "l2", "wide", "fallback_bvh")[r["regime"]]
        assert ti["lds_bytes"] == r["lds_bytes"]
    assert om.HittableList.new().tree_info()["regime"] == "none"


def test_tree_info_layout_and_enums_match_the_header(om, tmp_path):
    from raytracingoneweekend_amd import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is part of the build environment"
    enums = ["OM_KERNEL_BVH2W", "OM_TREE_NONE", "OM_TREE_LDS", "OM_TREE_L2", "OM_TREE_WIDE", "OM_TREE_FALLBACK_BVH", "OM_ABI_VERSION"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "ottomarcher.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(om_tree_info));']
    lines += [f'printf("{f} %zu\\n", offsetof(om_tree_info, {f}));' for f in INFO_FIELDS]
    lines += [f'printf("{e} %d\\n", (int)({e}));' for e in enums]
    lines += ["return 0; }"]
    (tmp_path / "ti.c").write_text("\n".join(lines))
    subprocess.check_call([cc, "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(tmp_path / "ti.c"), "-o", str(tmp_path / "ti")])
    got = dict((k, int(v)) for k, v in (l.split() for l in subprocess.check_output([str(tmp_path / "ti")], text=True).splitlines()))
    assert C.sizeof(_lib.om_tree_info) == got["size"] == 32
    assert [n for n, _ in _lib.om_tree_info._fields_] == INFO_FIELDS
    for f in INFO_FIELDS:
        assert getattr(_lib.om_tree_info, f).offset == got[f], f
    assert _lib.KERNELS["bvh2w"] == got["OM_KERNEL_BVH2W"] == 7
    assert [got[f"OM_TREE_{n.upper()}"] for n in _lib.TREE_REGIMES] == list(range(5))
    assert got["OM_ABI_VERSION"] == 2, "the ABI version stays"
