"""bench.py's host-side checks, on the CPU: the RCCL rank check the N>1 line depends on
 and the PMC fields the roofline copies from the committed summaries."""
import os

import pytest


@pytest.fixture(scope="module")
def bench():
    import bench as b
    return b


def test_comm_rank_check_passes_and_fails_loudly(bench):
    assert bench.check_comm_ranks((1, 0), 1, 0) == 1
    assert bench.check_comm_ranks((8, 5), 8, 5) == 8
    with pytest.raises(SystemExit, match=r"RCCL communicator has 1 ranks \(this is rank 0\), but WORLD_SIZE=2 RANK=1"):
        bench.check_comm_ranks((1, 0), 2, 1)
    with pytest.raises(SystemExit, match="WORLD_SIZE=8 RANK=3"):
        bench.check_comm_ranks((8, 2), 8, 3)


@pytest.mark.parametrize("cfg", ["C1", "C2", "C3"])
def test_pmc_fields_from_committed_summaries(bench, cfg):
    if not os.path.exists(bench.PMC_SUMMARY.format(cfg)):
        pytest.skip(f"no committed PMC summary for {cfg}")
    f = bench.pmc_fields(cfg)
    assert 0.0 < f["valu_lane_utilisation"] <= 1.0 and 0.0 <= f["wait_any_frac"] <= 1.0
    assert f["per_kernel"] and abs(sum(k["wave_cycle_share"] for k in f["per_kernel"].values()) - 1.0) < 1e-3
    assert bench.pmc_fields("C9") is None


@pytest.mark.parametrize("W,H", [(64, 48), (1024, 520)])       # a whole frame; one larger than the sample
def test_dump_outputs_fields_exact_and_repeatable(bench, tmp_path, W, H):
    """--dump-outputs: every Stats field of the frame (or of the fixed pixel sample of a frame
    larger than DUMP_PIXELS) comes back exactly from float32/float64 .npy files, the same pixels
    on every call, within the 64 MB the option allows; every value written is finite, the infinities
    (a sky pixel's avg_depth) and NaNs of the f32 fields carried by <field>_class.npy."""
    import numpy as np
    from raytracingoneweekend_amd import _lib as L
    rng = np.random.RandomState(3)
    fr = np.zeros(W * H, dtype=L.PIXEL_STATS_DTYPE)
    fr["bloom"] = rng.randint(0, 1 << 32, W * H).astype(np.uint64) << np.uint64(31) | np.uint64(1)
    fr["sum"] = rng.rand(W * H, 3).astype(np.float32) * 512
    fr["n"] = rng.randint(0, 1 << 31, W * H)
    fr["avg_depth"] = rng.rand(W * H).astype(np.float32) * 50
    fr["avg_depth"][::3] = np.inf
    fr["avg_depth"][5::7] = np.nan
    fr["sum"][1::5, 1] = -np.inf
    fr["sum"][2::11] = (np.nan, np.inf, 1.0)
    fr["bad_avgs"] = rng.randint(0, 6, W * H)
    fr["color"] = rng.randint(0, 256, (W * H, 3))
    fr["flags"] = rng.randint(0, 256, W * H)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, fr.view(np.uint8).reshape(-1), W, H)
    bench.dump_outputs(b, fr.view(np.uint8).reshape(-1).copy(), W, H)
    names = sorted(os.listdir(a))
    assert names == sorted(f + ".npy" for f in ("pixel", "sum", "sum_class", "n", "avg_depth", "avg_depth_class",
                                                  "bad_avgs", "color", "flags", "bloom"))
    got = {f[:-4]: np.load(os.path.join(a, f), allow_pickle=False) for f in names}
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 * 1000 * 1000
    for f in names:
        assert np.array_equal(got[f[:-4]], np.load(os.path.join(b, f), allow_pickle=False))
    pixel = got["pixel"].astype(np.int64)
    assert pixel.size == min(W * H, bench.DUMP_PIXELS) and np.all(np.diff(pixel) > 0) and pixel[-1] < W * H
    exp = fr[pixel]
    for f in ("n", "bad_avgs", "color", "flags"):
        assert np.array_equal(got[f], exp[f]), f
    for f in ("sum", "avg_depth"):
        cls = got[f + "_class"]
        assert (cls == 1).any() and (cls == 3).any() and (got[f][cls != 0] == 0).all()
        back = np.select([cls == 1, cls == 2, cls == 3], [np.inf, -np.inf, np.nan], got[f]).astype(np.float32)
        assert np.array_equal(back, exp[f], equal_nan=True), f
    bloom = got["bloom"].astype(np.uint64)
    assert np.array_equal(bloom[:, 0] | bloom[:, 1] << np.uint64(32), exp["bloom"])


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("cfg,ranks,steps", [("C1", 2, 2), ("C4", 2, 2), ("C3", 3, 1)])
def test_bench_multi_rank_harness_on_cpu(cfg, ranks, steps):
    """bench.py's N>1 control flow as the driver launches it (torch.distributed.run, one process per
    rank, gloo control plane), with RCCL replaced by a host transport (--host-rehearsal): the
    unique-id broadcast, check_comm_ranks on the group's real (size, rank), the weak/strong spp
    split, the shard capacities, the timed region's barriers and max over ranks, and the gather to
    rank 0 placed by om_shard_assemble_host (bench.py asserts every pixel's sample count and place).
    What stays unmeasured: RCCL itself with nranks > 1."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ranks}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(root, "bench.py"),
           "--gpus", str(ranks), "--host-rehearsal", "--config", cfg, "--steps", str(steps), "--warmup", "1"]
    env = dict(os.environ, OMP_NUM_THREADS="1")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout                                  # rank 0 only
    d = lines[0]
    import bench as b
    W, H = b.CONFIGS[cfg].get("size", (1920, 1080))
    assert d["host_rehearsal"] and d["n_ranks"] == ranks and d["nranks_seen"] == ranks
    assert (d["W"], d["H"]) == (W, H)
    # C4 renders the fixed frame (strong scaling); the others render spp x N on 1/N of the tiles
    assert d["spp_step"] == b.SPP_PER_STEP * (1 if cfg == "C4" else ranks)
    assert d["spp_total"] == d["spp_step"] * steps
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    assert d["shard_capacity"] == -(-tiles // ranks) * 64 and d["shard_pixels"] <= d["shard_capacity"]
