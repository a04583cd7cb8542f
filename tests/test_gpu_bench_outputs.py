"""GPU: the plain bench.py run (the headline fields only: set-up, warm-up, the timed steps, one JSON line) and what
--dump-outputs writes after the timed steps -- a seeded sample of the result array, float64, the same from run to run with
the same arguments, and equal to the oracle applied once per launch (the keyswitch accumulates into `result`)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
BATCH, STEPS, WARMUP = 512, 2, 1


def _plain_run(dump_dir):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "HEXL_BENCH_ONE_GPU", "HEXL_BENCH_FORCE_DIST"):
        env.pop(k, None)
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--total-batch", str(BATCH), "--dump-outputs", str(dump_dir)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=str(ROOT))
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line"
    return json.loads(lines[0])


def test_plain_run_and_dumped_outputs(tmp_path, orc, hx, dev):
    import torch
    import bench
    from ks_util import KsCase
    a, b = _plain_run(tmp_path / "a"), _plain_run(tmp_path / "b")
    for d in (a, b):
        assert d["unit"] == "keyswitches/s" and d["higher_is_better"] is True and d["dtype"] == "u64"
        assert d["metric"].startswith("keyswitches/sec") and d["steps"] == STEPS and d["warmup"] == WARMUP
        assert abs(d["value"] - BATCH * STEPS / (d["ms_per_step"] * STEPS * 1e-3)) / d["value"] < 1e-6
        assert not {"roofline", "extra", "cpu_baseline", "verified_vs_oracle", "ntt_fwd_per_s"} & set(d)   # all of that is --full
    names = ["keyswitch_result.npy", "keyswitch_result_instances.npy"]
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == names
    assert sum((tmp_path / "a" / n).stat().st_size for n in names) <= 64 * 2**20
    res, rows = (np.load(tmp_path / "a" / n) for n in names)
    assert res.dtype == np.float64 and rows.dtype == np.float64
    assert res.shape == (len(rows), 2, 7, bench.N) and len(rows) >= 8
    for n in names:                                               # same arguments, same inputs, same outputs
        assert np.array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n))
    # the dumped words are the timed path's result: the oracle once per launch (the first launch, warm-up, timed steps)
    case = KsCase(orc, bench.N, 7, 8, seed=1)
    d_t, d_r = bench.device_inputs(hx, orc, case, BATCH, dev)
    for j in (0, len(rows) - 1):
        i = int(rows[j])
        t, r = hx.to_u64(d_t[i]).copy(), hx.to_u64(d_r[i]).copy()
        for _ in range(1 + WARMUP + STEPS):
            r = case.expected(orc, t, r)
        assert np.array_equal(res[j].reshape(-1), r.astype(np.float64)), f"instance {i}"
    del d_t, d_r
    torch.cuda.empty_cache()
