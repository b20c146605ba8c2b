"""Are the tree culls conservative with respect to the float32 exact tests, away from the scene scale?
(CPU only: the oracle, numpy float64 and the host-only report of tests/cpp/leaf_boxes.cpp.)

A tree kernel gives the reference loop's answer only if every primitive that the loop's float32
test accepts sits in a leaf whose box, and every box above it, the ray's slab test passes.  The
boxes are inflated by an ABSOLUTE margin, 1e-3 * (1 + extent) + 1e-5 * max|coord| (om_bvh.cpp
inflate), and the slab window is [tmin / 2 - 1e-3, closest * 1.0001 + 1e-3]; the error of the exact
tests grows with the distance of the ray origin and with 1 / size.  The worlds and
ray sets of tests/scale_common.py leave the scale of every other test; this module checks, without a GPU,

  1. that the sets can tell: enough rays whose oracle winner is a tree-resident primitive although
     the ray's float64 line misses that primitive's un-inflated bound by more than the margin
     (test_sets_discriminate; a condition on the inputs, from the oracle alone), and
  2. that the build routes no such ray past the winner: for every ray that the product sends
     through a tree and the oracle answers with a tree-resident primitive at root t, the float64
     segment of the float32 ray over the loose window passes through the primitive's leaf box and
     through every box above it in every tree layout (test_winner_boxes_are_on_the_ray).

The answer of this commit: YES for the tiny and the sliver world and for every set from D = 1e4 on, because
a sphere or ellipsoid whose margin cannot cover the worst case of its test's rounding from 16 away stays
outside the trees (om_bvh.cpp thin_sphere; the tiny world holds radii on both sides of that, 1e-3 .. 0.2) and a
query ray beyond the slab test's reach (OM_SLAB_REACH) takes the reference loop; still NO for
spheres of radius 0.14 .. 1 seen from 1e2 or 1e3 away (scale_common.NOT_CONSERVATIVE), which fail check 2
and are strict expected failures here and, set for set, in tests/test_gpu_scale.py.  The figures the tests
print are in DESIGN.md §5.3.  Only Sphere::hit over-accepts below D = 1e4 (every winner found past its box is
a sphere or an ellipsoid); at D = 1e5 cubes and triangles do too (facets), where no ray is routed through a
tree any more.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import scale_common as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
F = np.float32
ALL = SC.WORLDS + [SC.L2_WORLD]
MIN_DISCRIMINATING = 32
# (world, D) sets that must discriminate.  Chosen from the error model, not from the product: the
# silhouette of a sphere of radius r, in a world whose coordinates reach C, seen from D away moves by
# about 6e-8 * (D^2 + C * D) / (2 r) (the rounding of c = |w2l o|^2 - 1 and of w2l o itself).  With
# r <= 1 and C <= 15 that passes the margin of 1.4e-3 .. 3e-3 from D = 1e3 on, and at D = 13 for
# r <= 5e-3 (tiny); at C = 3.6e4 / 1.4e5 the margin's 1e-5 * C term is 0.36 / 1.4, passed from
# D = 1e3 on as well; a scale of 1e-3 or 1e-4 on one axis (sliver) passes its margin at every D.
# Cube::hit and the barycentric test have no such cancellation; what moves them is the rounding of the
# hit point o + t d, about 6e-8 * (|o| + t) = 1.2e-2 at D = 1e5, against margins of 1.6e-3 .. 3e-3
# (facets at 1e5).  At D = 1e2 the model gives 6e-8 * 1e4 / (2 * 0.2) = 1.5e-3 for the cluster's smallest
# spheres, just past their margin of 1.4e-3: few rays, so that set is enlarged (scale_common.PER_DIR).
# "Tree-resident" is meant as on the parent commit, whose margin the count is about: every bounded
# primitive (Prim.bounded), whether or not this build keeps it in its trees.
MUST_DISCRIMINATE = [("tiny", 13.0), ("cluster", 1e2)] + [(w, D) for w in ("cluster", "cluster_a", "cluster_b", SC.L2_WORLD) for D in SC.FAR] + \
                    [("sliver", D) for D in SC.DISTANCES] + [("facets", 1e5)]
# The controls: the scene-scale set (cluster at D = 13), the displaced clusters at 13 and 1e2, whose margin
# of 0.36 / 1.4 the error passes from 1e3 on only, and the sphere-free world below 1e5.  They hold none, and
# the test says so: a control that starts to discriminate is a changed input, not a pass.
CONTROLS = [("cluster", 13.0)] + [(w, D) for w in ("cluster_a", "cluster_b") for D in (13.0, 1e2)] + \
           [("facets", D) for D in SC.DISTANCES[:-1]]


class _Data:
    """worlds, ray sets and oracle answers: built once per module and never changed"""

    def __init__(self, om, O):
        self.om, self.O, self.d = om, O, {}

    def world(self, name):
        if name not in self.d:
            items, w, ow = SC.world(self.om, self.O, name)
            self.d[name] = (items, ow, SC.ray_sets(self.om, self.O, name, items))
        return self.d[name]

    def answers(self, name, D, win):
        items, ow, sets = self.world(name)
        return SC.oracle_answers(self.om, self.O, name, D, ow, sets[D][0], *win)


@pytest.fixture(scope="module")
def data(om, oracle):
    return _Data(om, oracle)


@pytest.fixture(scope="module")
def report(data, tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", CPP, "leaf_boxes"])
    d = tmp_path_factory.mktemp("scale_worlds")
    args = []
    for name in ALL:
        path = str(d / f"{name}.bin")
        SC.dump(data.world(name)[0], path)
        args += [name, path]
    out = subprocess.run([os.path.join(CPP, "leaf_boxes")] + args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rep = {n: {"leaf": {}, "chains": {}} for n in ALL}
    for line in out.stdout.splitlines():
        if not line.startswith("{"):
            continue
        r = json.loads(line)
        w = rep[r["world"]]
        if "leaf" in r:
            w["leaf"][r["leaf"]] = np.array(r["box"], dtype=np.float64)
        elif "layout" in r:
            w["chains"].setdefault(r["layout"], {})[r["gi"]] = np.array(r["chain"], dtype=np.float64).reshape(-1, 6)
        else:
            w["info"] = r
    return rep


def _window(name, D):
    return SC.windows(name, D if D else 13.0)[0]


# ------------------------------------------------------------------ the report itself
@pytest.mark.parametrize("name", ALL)
def test_report_matches_the_python_geometry(data, report, name):
    """The program's world is the Python side's: the same primitives are tree-resident, and each
    f32 leaf box is the float64 bound inflated by the margin scale_common computes (to a few ulp)."""
    items = data.world(name)[0]
    rep = report[name]
    prims = SC.prims(items)
    assert rep["info"]["prims"] == len(prims)
    in_tree = {p.gi for p in prims if p.in_tree}
    boxed = set(rep["leaf"]) | set(rep["chains"].get("always2", {}))
    assert boxed == in_tree, (sorted(boxed - in_tree)[:5], sorted(in_tree - boxed)[:5])
    if name != SC.L2_WORLD:
        assert set(rep["leaf"]) == in_tree and len([p for p in prims if p.kind in ("tri", "para")]) >= 16
    for p in prims:
        if p.gi in rep["leaf"]:
            b = rep["leaf"][p.gi]
            want = np.concatenate([p.lo - p.margin, p.hi + p.margin])
            tol = 4.0 * np.spacing(np.abs(want).astype(F)).astype(np.float64) + 1e-6 * p.margin.max()
            assert (np.abs(b - want) <= np.concatenate([tol[:3] + tol[3:], tol[:3] + tol[3:]])).all(), (p.gi, b, want)
    if name == "tiny":
        # the eviction predicate is checked on both sides: of the spheres of radius 1e-2 .. 0.2 some stay outside
        # the trees and some are leaves (whose boxes test_winner_boxes_are_on_the_ray then holds to the rays)
        ring = [p for p in prims if p.kind == "sphere" and 9.99e-3 <= p.A[0, 0] <= 0.2 + 1e-6]   # (float32(1e-2) < 1e-2)
        assert len(ring) >= 12 and any(p.thin for p in ring) and sum(not p.thin for p in ring) >= 3, [p.thin for p in ring]
        assert all(p.thin for p in prims if p.kind == "sphere" and p.A[0, 0] < 9.99e-3)
    layouts = set(rep["chains"]) - {"always2"}
    assert {"bvh", "sbvh", "bvh2", "bvh2h", "bvh2w", "bvh4", "bvh4h"} <= layouts, layouts
    for lay in layouts:
        want = in_tree if lay == "bvh" else set(rep["leaf"])
        assert set(rep["chains"][lay]) == want, lay


def test_the_l2_world_reads_half_planes_and_the_far_worlds_lose_them(report):
    """g17 is past the LDS budget (its BVH2 is read through L2 with half-precision planes); at
    FAR_A a half plane has ulp 16, at FAR_B the x and z planes leave the half range."""
    assert report[SC.L2_WORLD]["info"]["b2_ok"] == 1 and report[SC.L2_WORLD]["info"]["b2_lds_bytes"] == 0
    a = np.concatenate(list(report["cluster_a"]["chains"]["bvh2h"].values()))
    b = np.concatenate(list(report["cluster_b"]["chains"]["bvh2h"].values()))
    assert np.isfinite(a).all() and (np.abs(a[:, 0]) % 16 == 0).all()
    # x and z planes at 1e5 are beyond the half range: lo is the largest finite half, hi is +inf
    assert (b[:, [0, 2]] == 65504.0).all() and np.isinf(b[:, [3, 5]]).all()


@pytest.mark.parametrize("name", ALL)
def test_every_box_contains_the_boxes_below_it(report, name):
    """Ray-independent: in every layout each box of a chain contains the next one, and the last one
    the primitive's leaf box (a half plane rounded outward still contains the f32 plane)."""
    rep = report[name]
    for lay, chains in rep["chains"].items():
        for gi, ch in chains.items():
            if lay == "always2":
                continue
            boxes = list(ch)
            if gi in rep["leaf"]:
                boxes.append(rep["leaf"][gi])
            for up, dn in zip(boxes[:-1], boxes[1:]):
                assert (up[:3] <= dn[:3]).all() and (up[3:] >= dn[3:]).all(), (lay, gi, up, dn)


# ------------------------------------------------------------------ 1. discriminating power
def _tree_winner(data, name, D, tree_gi):
    """-> rays, winner gi per ray (-1: no tree-resident winner), root t; the first window of the set"""
    items, ow, sets = data.world(name)
    rays = sets[D][0]
    exp = data.answers(name, D, _window(name, D))
    gi = exp["obj"].astype(np.int64) - 1
    ok = np.isin(gi, np.fromiter(tree_gi, dtype=np.int64)) & np.isfinite(exp["t"])
    return rays, np.where(ok, gi, -1), exp["t"]


def _prim_arrays(items):
    prims = SC.prims(items)
    lo = np.array([p.lo for p in prims]); hi = np.array([p.hi for p in prims]); m = np.array([p.margin for p in prims])
    return prims, lo, hi, m


@pytest.mark.parametrize("name", ALL)
def test_sets_discriminate(data, report, name):
    """Per (world, D): rays whose oracle winner is a tree-resident primitive although the ray's
    float64 line misses the winner's un-inflated bound by more than the builder's margin.
    Measured (rays / winners in the tree / of which beyond the margin):
      tiny      13: 5760 / 803 / 82
      cluster   13: 2688 / 1608 / 0,  1e2: 4992 rays / 3186 / 44 (28 of 2688 with 4 rays per direction),  1e3: 1951 / 478,  1e4: 2604 / 2405,  1e5: 2688 / 2597
      cluster_a 13: 566 / 0,  1e2: 578 / 0,  1e3: 682 / 51,  1e4: 2242 / 2115,  1e5: 2688 / 2610
      cluster_b 13: 264 / 0,  1e2: 270 / 0,  1e3: 18816 rays / 2139 / 47,  1e4: 1200 / 1003,  1e5: 2688 / 2591
      sliver    13: 1600 / 1563 / 1061,  1e2: 1590 / 1318,  1e3: 1600 / 1467,  1e4: 1600 / 1496,  1e5: 1599 / 1462
      g17       1e3: 3488 / 1738 / 886,  1e4: 2046 / 1979,  1e5: 2277 / 2264
      facets    13 .. 1e4: 1408 / 392 .. 403 / 0,  1e5: 20864 / 7824 / 51"""
    items, ow, sets = data.world(name)
    prims, lo, hi, m = _prim_arrays(items)
    tree_gi = {p.gi for p in prims if p.bounded}
    assert set(report[name]["leaf"]) <= tree_gi
    for D in SC.WORLD_DISTANCES[name]:
        assert ((name, D) in MUST_DISCRIMINATE) != ((name, D) in CONTROLS), (name, D)
        rays, win, _ = _tree_winner(data, name, D, tree_gi)
        sel = win >= 0
        g = win[sel]
        miss = SC.line_misses_box(rays[sel], lo[g] - m[g], hi[g] + m[g])
        n = int(miss.sum())
        print(f"{name} D={D:g}: {len(rays)} rays, {int(sel.sum())} tree winners, {n} beyond the margin")
        if (name, D) in MUST_DISCRIMINATE:
            assert n >= MIN_DISCRIMINATING, f"{name} D={D:g}: only {n} discriminating rays"
        else:
            assert n == 0, f"{name} D={D:g} is a control (measured: 0 discriminating rays) and holds {n}"


def test_far_answers_go_both_ways(data):
    """From the oracle alone: in each window the answers of a world's far sets contain hits and
    misses and at least 3 distinct objects.  (Set by set they need not: from D = 1e5 the float32
    sphere test of the cluster accepts every ray of the band.)"""
    for name in ALL:
        for k in range(len(SC.windows(name, 13.0))):
            ids = set()
            for D in SC.WORLD_DISTANCES[name]:
                ids |= set(int(x) for x in data.answers(name, D, SC.windows(name, D)[k])["obj"])
            assert 0 in ids and len(ids - {0}) >= 3, (name, k, len(ids))


# ------------------------------------------------------------------ 2. conservativeness of the build
def _slack(o, d, t_lo, t_hi, box, margin):
    """Per ray: the largest s such that the segment still meets the box shrunk by s * margin on
    every side (s = 1: the un-inflated bound; s < 0: the segment misses the box, which would have
    to GROW by -s margins).  Bisection on s in [-4096, 8]."""
    a = np.full(len(o), -4096.0); b = np.full(len(o), 8.0)
    for _ in range(48):
        s = 0.5 * (a + b)
        lo, hi = box[:, :3] + s[:, None] * margin, box[:, 3:] - s[:, None] * margin
        near, far = SC.slab(o, d, lo, hi)
        meets = (np.maximum(near, t_lo) <= np.minimum(far, t_hi)) & (lo <= hi).all(axis=1)
        a = np.where(meets, s, a); b = np.where(meets, b, s)
    return a


def routed_through_a_tree(rays, info):
    """The query rays a tree kernel does not hand to the reference loop: the finite ones that start
    within the build's far-origin distance of the root box (both from the program's report)."""
    assert info["slab_reach"] == SC.SLAB_REACH and info["sphere_reach"] == SC.SPHERE_REACH
    return np.isfinite(rays).all(axis=1) & ~SC.far_origin(rays, np.array(info["root"], dtype=np.float64))


def _cases():
    return [pytest.param(n, D, id=f"{n}-{D:g}", marks=SC.xfail_known((n, D) in SC.NOT_CONSERVATIVE)) for n in ALL for D in SC.sets_of(n)]


@pytest.mark.parametrize("name,D", _cases())
def test_winner_boxes_are_on_the_ray(data, report, name, D):
    """For every ray routed through a tree whose oracle answer is a tree-resident primitive at root
    t: the float64 segment over [tmin / 2 - 1e-3, t * 1.0001 + 1e-3] (the window of the slab tests
    when `closest` has come down to t itself) meets the leaf box and every box above it in every
    layout.  From D = 1e4 on no ray of a set is routed through a tree, and the test asserts that instead.
    The sets of scale_common.NOT_CONSERVATIVE are strict expected failures; measured
    (winners / past their leaf box / smallest slack in margins; half-extent of the failing winners):
    see DESIGN.md §5.3, which repeats this test's output."""
    items, ow, sets = data.world(name)
    prims, lo, hi, m = _prim_arrays(items)
    rep = report[name]
    tree_gi = set(rep["leaf"])
    leaf = rep["leaf"]
    rays, win, t = _tree_winner(data, name, D, tree_gi)
    routed = routed_through_a_tree(rays, rep["info"])
    if D >= 1e4:
        # 2 sqrt(3) * 1e4 / sqrt(3) > OM_SLAB_REACH: every ray of these sets starts beyond the slab test's reach
        assert not routed.any(), f"{name} D={D:g}: {int(routed.sum())} rays are still routed through a tree"
        print(f"{name} D={D:g}: no ray is routed through a tree (all start beyond the slab test's reach of {SC.SLAB_REACH:g})")
        return
    assert routed.all(), f"{name} D={D:g}: {int((~routed).sum())} rays take the reference loop"
    sel = (win >= 0) & routed
    assert sel.any(), "no ray of the set is answered by a tree-resident primitive"
    r, g, tt = rays[sel], win[sel], t[sel].astype(F)
    o, d = r[:, :3].astype(np.float64), r[:, 3:].astype(np.float64)
    tmin = F(_window(name, D)[0])
    t_lo = np.full(len(r), float(tmin * F(0.5) - F(1e-3)))
    t_hi = (tt * F(1.0001) + F(1e-3)).astype(np.float64)
    s = _slack(o, d, t_lo, t_hi, np.array([leaf[k] for k in g]), m[g])
    bad = s < 0
    above = 0
    for lay, chains in rep["chains"].items():
        if lay == "always2":
            continue
        for k in np.unique(g):
            pick = g == k
            for box in chains[int(k)]:
                near, far = SC.slab(o[pick], d[pick], box[:3], box[3:])
                above += int((np.maximum(near, t_lo[pick]) > np.minimum(far, t_hi[pick])).sum())
    half = 0.5 * (hi - lo).max(axis=1)
    sizes = f", half-extent of the failing winners {half[g[bad]].min():.3g} .. {half[g[bad]].max():.3g}" if bad.any() else ""
    kinds = sorted({prims[k].kind for k in g[bad]})
    print(f"{name} D={D:g}: {int(sel.sum())} winners, smallest slack {s.min():.3f} margins, {int(bad.sum())} miss the "
          f"leaf box {kinds}, {above} (ray, box) pairs missed above the leaves{sizes}")
    if bad.any() or above:
        # the pinned failure: leaf boxes of spheres and ellipsoids only (the thin ones have none)
        assert kinds == ["sphere"], kinds
        raise SC.KnownDisagreement(f"{name} D={D:g}: {int(bad.sum())} winners lie past their leaf box (smallest slack "
                                   f"{s.min():.3f} margins), {above} (ray, box) pairs are missed above the leaves")
