"""bench.py as the driver runs it, once, small: a plain run (no --full) times exactly --steps steps,
prints the headline line alone, and --dump-outputs writes the frame its timed steps produced."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP, PER_STEP = 2, 1, 16


def test_plain_run_is_lean_and_dumps_the_timed_frame(om, tmp_path):
    import torch
    import bench as b
    from raytracingoneweekend_amd import _lib as L
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--spp-per-step", str(PER_STEP), "--dump-outputs", out],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = lines[0]
    W, H, spp = 1920, 1080, STEPS * PER_STEP
    assert d["unit"] == "Msamples/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == STEPS and d["warmup"] == WARMUP and d["full"] is False
    # value and ms_per_step describe the same STEPS steps (both rounded in the line)
    assert d["value"] == pytest.approx(W * H * spp / (d["ms_per_step"] * STEPS) / 1e3, rel=1e-3)
    for k in ("window_parity", "hbm_gbs", "roofline", "work", "cpu_baseline", "configs"):
        assert d[k] is None, k                                   # measured under --full only

    got = {f[:-4]: np.load(os.path.join(out, f), allow_pickle=False) for f in os.listdir(out)}
    assert sum(v.nbytes for v in got.values()) <= 64 * 1000 * 1000
    pixel = got["pixel"].astype(np.int64)
    assert pixel.size == b.DUMP_PIXELS
    # the same frame through the single-GPU API: STEPS calls of PER_STEP samples, bench.py's seed
    world = om.random_scene(b.SCENE_SEED)
    cam = om.default_camera(W / H)
    fz = world.freeze(cam)
    frame = torch.zeros(W * H * 40, dtype=torch.uint8, device="cuda")
    p = om.make_params(b.MAX_DEPTH, b.TMIN, b.TMAX, spp, W, H, sample_count=PER_STEP, seed=b.SEED, march_steps=1024)
    for _ in range(STEPS):
        L.check(L.lib.om_render_device(fz.ctx, C.byref(cam.raw), C.byref(p), C.c_void_p(frame.data_ptr()), None), fz.ctx)
    torch.cuda.synchronize()
    fz.close()
    exp = frame.cpu().numpy().view(L.PIXEL_STATS_DTYPE)[pixel]
    assert (exp["n"] == spp).all() and (exp["bloom"] != 0).any()
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in got.values())
    for f in ("sum", "avg_depth"):                               # f32 as written; non-finite values by class
        cls = got[f + "_class"]
        back = np.select([cls == 1, cls == 2, cls == 3], [np.inf, -np.inf, np.nan], got[f]).astype(np.float32)
        assert np.array_equal(back, exp[f], equal_nan=True), f
    assert (got["avg_depth_class"] == 1).any(), "sky pixels carry an infinite avg_depth"
    for f in ("n", "bad_avgs", "color", "flags"):
        assert np.array_equal(got[f], exp[f]), f
    bloom = got["bloom"].astype(np.uint64)
    assert np.array_equal(bloom[:, 0] | bloom[:, 1] << np.uint64(32), exp["bloom"])
