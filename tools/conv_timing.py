"""GPU-box probe: what the convergence experiment (psmf_conv_run, rpsmf_amd.convergence) takes at the reference's own shape -- d = 4,
r = 1, n = 1000, the data of tests/golden/convergence_expdata.npz -- for a batch of random starts.

    python tools/conv_timing.py --batch 16384 --iters 10000            # shared data: one Y and one Kalman path for all replicas
    python tools/conv_timing.py --batch 4096 --iters 1000 --own        # own data: every replica its own Y (the stored Y plus noise)
    python tools/conv_timing.py --baselines [--batch 16384]            # what else runs this step: the float64 numpy model of the
                                                                       # tests, and one sweep through linear_psmf_batch (A = I, H = I)

One call (no warm-up: a call of 10^7 serial steps is its own warm-up; `--calls` repeats it): the device-event time of the kernels
(`elapsed_ms`) and the wall time of the whole call, each also as time per replica-step and as replicas finished per second.  The
starts are main.m's: X0ps = 5 randn, C = 10 |randn|, P0 = 25 I, v = 1.  Prints a table and one JSON line."""

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
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10000)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--own", action="store_true")
    ap.add_argument("--moments", action="store_true")
    ap.add_argument("--baselines", action="store_true")
    a = ap.parse_args()
    from rpsmf_amd import convergence_batch

    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "convergence_expdata.npz")))
    Y, Ctrue, Q, Rd = g["Y"], g["Ctrue"], g["Q"], g["Rdiag"]
    d, n = Y.shape
    r = Ctrue.shape[1]
    rng = np.random.default_rng(2025)
    B = a.batch
    x0 = 5.0 * rng.standard_normal((B, r))
    C0 = 10.0 * np.abs(rng.standard_normal((B, d, r)))
    P0 = 25.0 * np.eye(r)
    if a.baselines:
        import conv_cases as CC
        from rpsmf_amd.ssm import linear_psmf_batch

        cs = dict(r=r, d=d, n=n, n_iter=1, B=1, own=False, Y=Y, Ctrue=Ctrue, Q=Q, Rdiag=Rd, x0k=g["X0k"][:, 0], P0k=g["P0k"], C0=C0[:1], x0=x0[:1],
                  P0=P0[None], v=np.ones(1), q_scale=np.ones(1), r_scale=np.ones(1))
        t0 = time.perf_counter()
        CC.model(cs)
        host_s = time.perf_counter() - t0
        Yb = np.broadcast_to(Y, (B, d, n))
        I = np.eye(r)
        args = (Yb, C0, x0, I, P0, I, Q, I, float(Rd[0]))
        linear_psmf_batch(*args, carry_P=True)
        t0 = time.perf_counter()
        res = linear_psmf_batch(*args, carry_P=True)
        wall = time.perf_counter() - t0
        ms = float(res["elapsed_ms"])
        print(f"float64 numpy model (tests/conv_cases.py), one replica, Kalman pass and one iteration: {host_s:.3f} s = {host_s / (2 * n) * 1e6:.1f} us per step")
        print(f"linear_psmf_batch, one sweep (A = I, H = I, carry_P), batch {B}: kernel {ms:.2f} ms = {ms * 1e6 / (B * n):.3f} ns per replica-step; "
              f"call {wall * 1e3:.0f} ms = {wall * 1e9 / (B * n):.3f} ns per replica-step;  all OK: {not res['status'].any()}")
        print(json.dumps(dict(baselines=True, batch=B, numpy_model_us_per_step=host_s / (2 * n) * 1e6, ssm_kernel_ms=ms, ssm_wall_ms=wall * 1e3,
                              ssm_kernel_ns_per_replica_step=ms * 1e6 / (B * n), ssm_wall_ns_per_replica_step=wall * 1e9 / (B * n))))
        return
    if a.own:
        Yin = Y[None] + 0.05 * rng.standard_normal((B, d, n))
        xk0 = 5.0 * rng.standard_normal((B, r))
    else:
        Yin, xk0 = Y, g["X0k"][:, 0]
    kms, wall, res = [], [], None
    for _ in range(a.calls):
        t0 = time.perf_counter()
        res = convergence_batch(Yin, Ctrue, C0, x0, P0, Q=Q, R=Rd, n_iter=a.iters, x0_kalman=xk0, P0_kalman=g["P0k"], want_moments=a.moments)
        wall.append(time.perf_counter() - t0)
        kms.append(float(res["elapsed_ms"]))
    steps = B * n * a.iters
    k, w = float(np.median(kms)) * 1e-3, float(np.median(wall))
    ok = int(np.sum(res["status"] == 0))
    print(f"psmf_conv_run, {'own' if a.own else 'shared'} data, d = {d}, r = {r}, n = {n}, {a.iters} iterations, batch {B}"
          f"{', moments' if a.moments else ''}: kernels {k:.3f} s = {k / steps * 1e9:.4f} ns per replica-step, {B / k:.1f} replicas/s;  "
          f"call {w:.3f} s = {w / steps * 1e9:.4f} ns per replica-step, {B / w:.1f} replicas/s;  one lane's step: {k / (n * a.iters) * 1e6:.3f} us;  "
          f"replicas OK: {ok} of {B};  median avW of the last iteration {np.median(res['avW'][:, -1]):.4f}, CerrI {np.median(res['CerrI'][:, -1]):.4f}")
    print(json.dumps(dict(own=a.own, moments=a.moments, d=d, r=r, n=n, iters=a.iters, batch=B, kernel_s=[v * 1e-3 for v in kms], wall_s=wall,
                          kernel_ns_per_replica_step=k / steps * 1e9, wall_ns_per_replica_step=w / steps * 1e9, replicas_per_s_kernel=B / k,
                          replicas_per_s_call=B / w, replicas_ok=ok)))


if __name__ == "__main__":
    main()
