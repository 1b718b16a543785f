"""GPU-box probe: what the batched Bayesian online change-point detection (psmf_bocpd_run) takes at the change-point experiment's own
shape, ExperimentChange/main.m through MVBOCPD.m: 20 channels, the 801 samples from 400 on, 1000 independent series in one call.

    python tools/bocpd_timing.py [--batch 1000] [--T 801] [--dim 20] [--calls 3]

The series are N(2, 1) channels that move to N(-2, 1) at sample 201 (a change the detector declares, so the truncation runs).  One
warm-up call, then the median of `--calls` calls, device-event time of the two kernels (`elapsed_ms`) and the wall time of the call
(transfers, the host's finiteness scan and its table of log-gamma terms included).  Beside it the wall time of the Cholesky-factor,
log-domain numpy model (tests/bocpd_cases.py: stable_model) for ONE series on the same box, and the device's agreement with it on
that series.  Prints a table and one JSON line."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--T", type=int, default=801)
    ap.add_argument("--dim", type=int, default=20)
    ap.add_argument("--calls", type=int, default=3)
    a = ap.parse_args()
    import bocpd_cases as BC
    from rpsmf_amd.changepoint import mvbocpd_batch

    rng = np.random.default_rng(2024)
    X = rng.standard_normal((a.batch, a.dim, a.T)) + 2.0
    X[:, :, a.T // 4:] -= 4.0
    print(f"psmf_bocpd_run at dim = {a.dim}, T = {a.T}, batch = {a.batch}: one warm-up, then {a.calls} calls")
    mvbocpd_batch(X)
    ms, wall, res = [], [], None
    for _ in range(a.calls):
        t0 = time.perf_counter()
        res = mvbocpd_batch(X)
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(float(res["elapsed_ms"]))
    t0 = time.perf_counter()
    ref = BC.stable_model(X[0])
    host_s = time.perf_counter() - t0
    same = bool(np.array_equal(res["map_run"][0], ref["map_run"]) and list(res["changepoints"][0]) == ref["changepoints"])
    err = float(np.max(np.abs(res["R_last"][0] - ref["R_last"])) / np.max(np.abs(ref["R_last"])))
    med = float(np.median(ms))
    pairs = a.batch * a.T * (a.T + 1) / 2
    ok = bool(np.all(res["status"] == 0))
    found = np.bincount(res["n_changepoints"], minlength=3)
    print(f"  elapsed_ms {['%.3f' % v for v in ms]}  median {med:.3f} ms  ({med / a.batch * 1e3:.2f} us per series, "
          f"{pairs / (med * 1e-3):.4g} hypothesis-steps/s);  wall of the call {['%.1f' % v for v in wall]} ms")
    print(f"  stable_model, one series: {host_s:.3f} s wall, so {host_s * a.batch:.0f} s for the batch: {host_s * a.batch / (med * 1e-3):.0f} x the kernels;  "
          f"series 0 against it: map_run and change points equal: {same}, R_last {err:.2e};  all series OK: {ok};  "
          f"series by number of change points (0, 1, 2, ...): {found.tolist()}")
    print(json.dumps(dict(shape=dict(dim=a.dim, T=a.T, batch=a.batch), elapsed_ms=ms, median_ms=med, wall_ms=wall,
                          hypothesis_steps_per_s=pairs / (med * 1e-3), stable_model_one_series_s=host_s, series0_equal=same,
                          series0_R_last_relerr=err, ok=ok, series_by_changepoints=found.tolist())))


if __name__ == "__main__":
    main()
