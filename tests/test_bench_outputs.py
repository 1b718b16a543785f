"""`bench.py` without --full: the result line carries the headline fields only, and --dump-outputs writes what the last timed pass
computed -- the same arrays from run to run, and the state and y_hat that the same passes give when made through the library
directly.  GPU only: `pytest -m gpu`."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, relerr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

D, R, T, STEPS, WARMUP = 8000, 32, 400, 3, 1


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(STEPS), "--warmup", str(WARMUP), "--rows", str(D),
           "--latent-rank", str(R), "--timesteps", str(T), "--dump-outputs", str(out_dir)]
    pr = subprocess.run(cmd, capture_output=True, text=True, timeout=280, env=dict(os.environ, OMP_NUM_THREADS="4"), cwd=ROOT)
    assert pr.returncode == 0, pr.stdout[-2000:] + pr.stderr[-3000:]
    lines = [ln for ln in pr.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, pr.stdout[-2000:]
    return json.loads(lines[0])


def _load(out_dir):
    return {n[:-4]: np.load(os.path.join(out_dir, n)) for n in sorted(os.listdir(out_dir))}


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    lines = [_plain_run(tmp_path / name) for name in ("a", "b")]
    for line in lines:
        assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["unit"] == "timesteps/s" and line["higher_is_better"] is True
        assert line["dtype"] == "f64" and line["value"] > 0
        assert abs(line["ms_per_step"] - 1e3 * T / line["value"]) < 1e-6 * line["ms_per_step"]
        for moved in ("cpu_baseline", "parity_vs_cpu_oracle", "roofline", "cold_pass_steps_per_s", "other_configs"):
            assert moved not in line, moved

    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == sorted(b)
    assert {"C", "V", "P", "Q", "mu", "rho", "lam", "eta", "N", "y_hat", "y_hat_timesteps"} <= set(a)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(os.path.getsize(tmp_path / "a" / (n + ".npy")) for n in a) <= 64_000_000
    assert a["C"].shape == (D, R) and a["y_hat"].dtype == np.float32 and a["y_hat"].shape == (a["y_hat_timesteps"].size, D)
    for n in a:
        assert a[n].shape == b[n].shape and relerr(a[n], b[n]) < 1e-6, n

    # the same passes through the library: reset + one pass (what bench.py makes before its warm-up), then warm-up and timed passes
    import bench
    from rpsmf_amd import _capi

    seed = 35853
    series = bench.Series(D, R, T, seed, 0, D, False)
    st0 = bench.init_state(D, R, seed)
    f = _capi.DeviceFilter(D, R, storage="f32")
    try:
        for t0, Yc in series.chunks():
            f.upload_series(Yc, t0=t0, T_total=T)
        f.set_state(st0["C"], st0["V"], st0["P"], st0["Q"], st0["mu"], rho=st0["rho"], lambda0=st0["lam"])
        for _ in range(1 + WARMUP + STEPS):
            f.run(0, T)
        s = f.get_state()
        yp = np.concatenate([f.y_pred(int(t), 1, dtype=np.float32) for t in a["y_hat_timesteps"]])
    finally:
        f.close()
    for n in ("C", "V", "P", "mu"):
        assert relerr(a[n], s[n]) < 1e-6, n
    assert relerr(a["y_hat"], yp) < 1e-6
