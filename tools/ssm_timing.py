"""GPU-box probe: what the batched PSMF with linear-Gaussian dynamics and an observation map (psmf_ssm_run) takes at the
change-point experiment's own shape, ExperimentChange/main.m: d = 20, n = 1200, r = 10, p = 20 (Matern-3/2, lengthscale 0.1,
variance 0.1, dt = 1e-3, rho = 1e-3, V = I, P0 = I), 1000 independent series in one launch.

    python tools/ssm_timing.py [--batch 1000] [--n 1200] [--calls 5]

One warm-up call, then the median of `--calls` calls, device-event time of the kernel alone (`elapsed_ms`), for both carry_P values;
replica-steps per second = batch * n / median.  Beside it the wall time of the line-for-line numpy model (tests/ssm_cases.py:
literal_model) for ONE replica on the same box, and the device's error against it on that replica.  Prints a table and one JSON line."""

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
    ap.add_argument("--n", type=int, default=1200)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    import ssm_cases as SC
    from rpsmf_amd.ssm import linear_psmf_batch

    cs = dict(d=20, n=a.n, r=10, p=20, kind="matern", carry_P=1)
    pbs = [SC.problem(cs, seed=s) for s in range(a.batch)]
    pb = pbs[0]
    Y, C0, x0 = (np.stack([q[k] for q in pbs]) for k in ("Y", "C0", "x0"))
    out = {"shape": dict(d=20, n=a.n, r=10, p=20, batch=a.batch), "calls": a.calls}
    print(f"psmf_ssm_run at d = 20, n = {a.n}, r = 10, p = 20, batch = {a.batch}: one warm-up, then {a.calls} calls")
    for carry_P in (1, 0):
        run = lambda: linear_psmf_batch(Y, C0, x0, pb["V"], pb["P0"], pb["A"], pb["Q"], pb["H"], pb["rho"], carry_P=bool(carry_P))
        run()
        ms, res = [], None
        for _ in range(a.calls):
            res = run()
            ms.append(float(res["elapsed_ms"]))
        t0 = time.perf_counter()
        ref = SC.literal_model(pb, carry_P)
        host_s = time.perf_counter() - t0
        err = max(SC.relerr(res[k][0], ref[k]) for k in ("X", "C", "V", "P", "x", "scalars"))
        med = float(np.median(ms))
        rate = a.batch * a.n / (med * 1e-3)
        ok = bool(np.all(res["status"] == 0))
        print(f"  carry_P = {carry_P}: elapsed_ms {['%.3f' % v for v in ms]}  median {med:.3f} ms  {rate:.4g} replica-steps/s  "
              f"({med * 1e3 / a.n:.3f} us per step of the batch);  literal_model, one replica: {host_s:.3f} s wall "
              f"({a.n / host_s:.4g} steps/s);  device against it, replica 0: {err:.2e};  all replicas OK: {ok}")
        out[f"carry_P={carry_P}"] = dict(elapsed_ms=ms, median_ms=med, replica_steps_per_s=rate, literal_model_one_replica_s=host_s,
                                         relerr_replica0=err, ok=ok)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
