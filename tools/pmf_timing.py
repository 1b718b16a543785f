"""GPU-box probe: what the batched PMF baseline (psmf_pmf_run, rpsmf_amd/pmf.py) takes at the imputation experiment's largest shape,
19 x 295 719 (the shape the masked engine's headline is quoted at), and at the S&P 500's row count, 505 x 1259 -- r = 10, 2 epochs,
9 batches, 100 replicas in one call, as PMF.py runs its 100 repeats.

    python tools/pmf_timing.py [--shape 19x295719 --shape 505x1259] [--batch 100] [--calls 3]

Synthetic data like the datasets (40 + a rank-3 signal of standard deviation 6 + unit noise, a tenth natively missing, a fifth of the
rest held out per replica); the permutations are drawn once, outside the timing.  Per shape one warm-up call, then the median of
`--calls` calls of: the host work in front of the launch (means, batch maps, layouts), the wall time of psmf_pmf_run (transfers
included), their sum = the wall time of pmf_batch, and the device-event time of the kernels (`elapsed_ms`).  Beside it the wall time of
the numpy model (tests/pmf_model.py) for ONE replica on the same box, and the device's agreement with it on that replica.  Prints a
table and one JSON line per shape."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

R, EPOCHS, NB = 10, 2, 9


def problem(d, n, B, seed=7):
    rng = np.random.default_rng([seed, d, n])
    sig = rng.standard_normal((d, 3)) @ rng.standard_normal((3, n))
    sig *= 6.0 / float(sig.std())
    native = rng.random((d, n)) < 0.1
    Y = np.where(native, 0.0, 40.0 + sig + rng.standard_normal((d, n)))
    M = np.zeros((B, d, n), dtype=np.uint8)
    Mm = np.zeros((B, d, n), dtype=np.uint8)
    perms = []
    for b in range(B):
        held = (rng.random((d, n)) < 0.2) & ~native
        M[b], Mm[b] = ~native & ~held, held
        N = int(M[b].sum())
        perms.append([rng.permutation(N) for _ in range(EPOCHS)])
    return Y, M, Mm, rng.random((B, d, R)), rng.random((B, R, n)), perms


def relerr(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", default=None, help="dxn, may be repeated")
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--calls", type=int, default=3)
    a = ap.parse_args()
    import pmf_model
    from rpsmf_amd import pmf as P

    for shape in a.shape or ["19x295719", "505x1259"]:
        d, n = (int(v) for v in shape.split("x"))
        Y, M, Mm, C0, X0, perms = problem(d, n, a.batch)
        print(f"psmf_pmf_run at d = {d}, n = {n}, r = {R}, {EPOCHS} epochs of {NB} batches, {a.batch} replicas: one warm-up, then {a.calls} calls", flush=True)
        host, call, dev, res = [], [], [], None
        for k in range(a.calls + 1):
            t0 = time.perf_counter()
            h = P._prepare(Y, M, Mm, C0, X0, perms, EPOCHS, NB)
            t1 = time.perf_counter()
            res = P._launch(h, 50, 0.01, 0.8, 0, False)
            t2 = time.perf_counter()
            del h
            print(f"  call {k}: host {(t1 - t0) * 1e3:.0f} ms, psmf_pmf_run {(t2 - t1) * 1e3:.0f} ms, kernels {res['elapsed_ms']:.1f} ms", flush=True)
            if k:
                host.append((t1 - t0) * 1e3)
                call.append((t2 - t1) * 1e3)
                dev.append(float(res["elapsed_ms"]))
        t0 = time.perf_counter()
        ref = pmf_model.pmf_model(Y, M[0], Mm[0], C0[0], X0[0], perms[0], epochs=EPOCHS, num_batches=NB)
        model_s = time.perf_counter() - t0
        err = dict(Efull=float(np.max(np.abs(res["Efull"][0] - ref["Efull"]) / np.abs(ref["Efull"]))), C=relerr(res["C"][0], ref["P"]),
                   X=relerr(res["X"][0], ref["W"].T))
        ok = bool(np.all(res["status"] == 0))
        med = {k: float(np.median(v)) for k, v in (("host", host), ("call", call), ("dev", dev))}
        entries = float(M.sum()) * EPOCHS
        print(f"  kernels {['%.1f' % v for v in dev]} ms, median {med['dev']:.1f} ms ({med['dev'] / a.batch:.3f} ms per replica, "
              f"{entries / (med['dev'] * 1e-3):.4g} training entries/s);  psmf_pmf_run wall {['%.0f' % v for v in call]} ms;  "
              f"host work in front of it {['%.0f' % v for v in host]} ms;  pmf_batch = both: median {med['host'] + med['call']:.0f} ms")
        print(f"  pmf_model, one replica: {model_s:.2f} s wall, so {model_s * a.batch:.0f} s for the batch: {model_s * a.batch / ((med['host'] + med['call']) * 1e-3):.1f} x pmf_batch, "
              f"{model_s * a.batch / (med['dev'] * 1e-3):.0f} x the kernels;  replica 0 against it: {err};  all replicas OK: {ok}", flush=True)
        print(json.dumps(dict(shape=dict(d=d, n=n, r=R, epochs=EPOCHS, num_batches=NB, batch=a.batch), kernels_ms=dev, call_wall_ms=call, host_ms=host,
                              median=med, model_one_replica_s=model_s, replica0_err=err, ok=ok)), flush=True)
        del Y, M, Mm, C0, X0, perms, res


if __name__ == "__main__":
    main()
