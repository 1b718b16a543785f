"""GPU-box probe, the sibling of tools/ssm_timing.py: what the robust (rPSMF), the masked and the robust + masked instance of the batched
PSMF with linear-Gaussian dynamics and an observation map (psmf_ssm_run_ex) take beside the plain one (psmf_ssm_run), at the
change-point experiment's own shape, ExperimentChange/main.m: d = 20, n = 1200, r = 10, p = 20 (Matern-3/2, lengthscale 0.1,
variance 0.1, dt = 1e-3, rho = 1e-3, V = I, P0 = I), 1000 independent series in one launch.

    python tools/ssm_robust_timing.py [--batch 1000] [--n 1200] [--calls 5]

Y carries a Student-t draw (3 degrees of freedom) on 5 % of its entries, the mask observes 80 % (tests/ssm_robust_cases.py: problem);
robust is lambda0 = 1.8, growing by d per step (the first variant of the tests).  Per form and carry_P: one warm-up call, then
the median and the spread (max - min) of `--calls` calls, device-event time of the kernel alone (`elapsed_ms`); the four forms are
visited in turn inside every round, so a drift of the box shows in all of them.  Prints a table and one JSON line."""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FORMS = {"plain": dict(), "robust": dict(robust=True), "masked": dict(masked=True), "robust+masked": dict(robust=True, masked=True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--n", type=int, default=1200)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    import ssm_robust_cases as RC
    from rpsmf_amd.ssm import linear_psmf_batch

    cs = dict(d=20, n=a.n, r=10, p=20, kind="matern", carry_P=1, masked=True)
    pbs = [RC.problem(cs, seed=s) for s in range(a.batch)]
    pb = pbs[0]
    Y, C0, x0, M = (np.stack([q[k] for q in pbs]) for k in ("Y", "C0", "x0", "mask"))
    out = {"shape": dict(d=20, n=a.n, r=10, p=20, batch=a.batch), "calls": a.calls}
    print(f"psmf_ssm_run and psmf_ssm_run_ex at d = 20, n = {a.n}, r = 10, p = 20, batch = {a.batch}: one warm-up, then {a.calls} calls per form")

    def run(form, carry_P):
        kw = dict(carry_P=bool(carry_P))
        if FORMS[form].get("robust"):
            kw.update(robust=True, lambda0=1.8)
        if FORMS[form].get("masked"):
            kw.update(mask=M)
        return linear_psmf_batch(Y, C0, x0, pb["V"], pb["P0"], pb["A"], pb["Q"], pb["H"], pb["rho"], **kw)

    for carry_P in (1, 0):
        ms = {f: [] for f in FORMS}
        ok = {}
        for f in FORMS:
            run(f, carry_P)
        for _ in range(a.calls):
            for f in FORMS:
                res = run(f, carry_P)
                ms[f].append(float(res["elapsed_ms"]))
                ok[f] = int(np.sum(res["status"] == 0))
        for f in FORMS:
            med, spread = float(np.median(ms[f])), max(ms[f]) - min(ms[f])
            print(f"  carry_P = {carry_P}  {f:14s} elapsed_ms {['%.3f' % v for v in ms[f]]}  median {med:.3f} ms  spread {spread:.3f} ms  "
                  f"{a.batch * a.n / (med * 1e-3):.4g} replica-steps/s  ({med / float(np.median(ms['plain'])):.3f} x plain);  "
                  f"replicas OK: {ok[f]} of {a.batch}")
            out[f"carry_P={carry_P} {f}"] = dict(elapsed_ms=ms[f], median_ms=med, spread_ms=spread, replicas_ok=ok[f])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
