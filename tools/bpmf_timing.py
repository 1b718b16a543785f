"""GPU-box probe: what the batched BPMF baseline (psmf_bpmf_run, rpsmf_amd/bpmf.py) takes at LondonAir_PM25's shape, 27 x 4393 with 100
replicas, as BPMF.py runs its 100 repeats, and at the imputation experiment's largest shape, 19 x 295 719, with as many replicas as
one chunk of the native call holds (its budget is 16 GiB of device memory; the normals alone are 95 MB a replica there) -- r = 10,
2 epochs.

    python tools/bpmf_timing.py [--shape 27x4393:100 --shape 19x295719:0] [--calls 3]        (dxn:replicas, 0 = one chunk's worth)

Synthetic data like the datasets (40 + a rank-3 signal of standard deviation 6 + unit noise, a tenth natively missing, a fifth of the
rest held out per replica).  The draws of all replicas are made once and timed on their own (`draw_bpmf`, the global numpy RNG).  Per
shape one warm-up call, then the median of `--calls` calls of: the host work in front of the warm start (means, batch maps, layouts),
the wall time of the warm start's native call and of the sweeps' (transfers and the stacking of the draws included), and the
device-event time of the kernels of each.  Beside it the wall time of the line-for-line numpy model (tests/bpmf_model.py) for ONE
replica on the same box, and the device's agreement with it on that replica.  Prints a table and one JSON line per shape."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

R, EPOCHS, BETA = 10, 2, 2
BUDGET = 16 << 30      # psmf_bpmf_run's cap on the device memory of a chunk


def one_chunk(d, n):
    """the replicas psmf_bpmf_run takes in one chunk at this shape (the sizes of bpmf_run in rpsmf_amd/csrc/psmf_bpmf.hip)"""
    cols = min(-(-max(64, -(-n // 64)) // 4) * 4, -(-n // 4) * 4)
    nwg = -(-n // cols)
    doubles = EPOCHS * 2 * (n + d) * R + EPOCHS * 2 * R * R + EPOCHS * 2 * R + n * R + d * R + nwg * d * 272 + nwg * 16 + nwg * 256 + 2 * 272 + n * d + EPOCHS + 2
    return (BUDGET - 8 * n * d) // (2 * n * d + 4 + 8 * doubles)


def problem(d, n, B, seed=7):
    rng = np.random.default_rng([seed, d, n])
    sig = rng.standard_normal((d, 3)) @ rng.standard_normal((3, n))
    sig *= 6.0 / float(sig.std())
    native = rng.random((d, n)) < 0.1
    Y = np.where(native, 0.0, 40.0 + sig + rng.standard_normal((d, n)))
    M = np.zeros((B, d, n), dtype=np.uint8)
    Mm = np.zeros((B, d, n), dtype=np.uint8)
    for b in range(B):
        held = (rng.random((d, n)) < 0.2) & ~native
        M[b], Mm[b] = ~native & ~held, held
    return Y, M, Mm, rng.random((B, d, R)), rng.random((B, R, n))


def relerr(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", default=None, help="dxn:replicas, may be repeated; 0 replicas = what one chunk holds")
    ap.add_argument("--calls", type=int, default=3)
    a = ap.parse_args()
    import bpmf_model
    from rpsmf_amd import bpmf as BP
    from rpsmf_amd import pmf as P

    for shape in a.shape or ["27x4393:100", "19x295719:0"]:
        dn, B = shape.split(":")
        d, n = (int(v) for v in dn.split("x"))
        B = int(B) or int(one_chunk(d, n))
        Y, M, Mm, C0, X0 = problem(d, n, B)
        np.random.seed(11)
        t0 = time.perf_counter()
        draws = [BP.draw_bpmf(d, n, R, int(M[b].sum()), EPOCHS) for b in range(B)]
        draw_ms = (time.perf_counter() - t0) * 1e3
        print(f"bpmf_batch at d = {d}, n = {n}, r = {R}, {EPOCHS} epochs, {B} replicas: the draws {draw_ms:.0f} ms ({draw_ms / B:.1f} ms a replica); "
              f"one warm-up, then {a.calls} calls", flush=True)
        keys = ("host", "warm_call", "sweep_call", "warm_dev", "sweep_dev")
        t = {k: [] for k in keys}
        res = None
        for k in range(a.calls + 1):
            t0 = time.perf_counter()
            h = P._prepare(Y, M, Mm, C0, X0, [dr["perms"] for dr in draws], EPOCHS, BP.WARM_START["num_batches"])
            h["Mt"] = np.ascontiguousarray(np.transpose(M != 0, (0, 2, 1)).astype(np.uint8))
            t1 = time.perf_counter()
            warm = P._launch(h, BP.WARM_START["epsilon"], BP.WARM_START["lmd"], BP.WARM_START["momentum"], 0, False)
            warm_dev = float(warm["elapsed_ms"])
            t2 = time.perf_counter()
            res = BP._sweeps(h, warm, draws, BETA, 0, False)
            t3 = time.perf_counter()
            del h, warm
            now = dict(host=(t1 - t0) * 1e3, warm_call=(t2 - t1) * 1e3, sweep_call=(t3 - t2) * 1e3, warm_dev=warm_dev, sweep_dev=float(res["elapsed_ms"]) - warm_dev)
            print(f"  call {k}: host {now['host']:.0f} ms, psmf_pmf_run {now['warm_call']:.0f} ms (kernels {now['warm_dev']:.1f} ms), "
                  f"psmf_bpmf_run with the stacking of the draws {now['sweep_call']:.0f} ms (kernels {now['sweep_dev']:.1f} ms)", flush=True)
            if k:
                for key in keys:
                    t[key].append(now[key])
        med = {k: float(np.median(v)) for k, v in t.items()}
        whole = med["host"] + med["warm_call"] + med["sweep_call"]
        t0 = time.perf_counter()
        ref = bpmf_model.bpmf_model(Y, M[0], Mm[0], C0[0], X0[0], draws[0], epochs=EPOCHS, beta=BETA)
        model_s = time.perf_counter() - t0
        err = dict(Efull=float(np.max(np.abs(res["Efull"][0] - ref["Efull"]) / np.abs(ref["Efull"]))), C=relerr(res["C"][0], ref["P"]),
                   X=relerr(res["X"][0], ref["W"].T))
        ok = bool(np.all(res["status"] == 0))
        print(f"  medians: kernels of the warm start {med['warm_dev']:.1f} ms, of the sweeps {med['sweep_dev']:.1f} ms ({med['sweep_dev'] / B:.3f} ms a replica); "
              f"host work in front {med['host']:.0f} ms, psmf_pmf_run {med['warm_call']:.0f} ms, psmf_bpmf_run {med['sweep_call']:.0f} ms: "
              f"bpmf_batch with the draws handed in {whole:.0f} ms, with its own draws {whole + draw_ms:.0f} ms")
        print(f"  bpmf_model, one replica: {model_s:.2f} s wall, so {model_s * B:.0f} s for the batch: {model_s * B / ((whole + draw_ms) * 1e-3):.1f} x bpmf_batch with its draws, "
              f"{model_s * B / ((med['warm_dev'] + med['sweep_dev']) * 1e-3):.0f} x the kernels;  replica 0 against it: {err};  all replicas OK: {ok}", flush=True)
        print(json.dumps(dict(shape=dict(d=d, n=n, r=R, epochs=EPOCHS, batch=B), draws_ms=draw_ms, times_ms=t, median=med, bpmf_batch_ms=whole,
                              model_one_replica_s=model_s, replica0_err=err, ok=ok)), flush=True)
        del Y, M, Mm, C0, X0, draws, res


if __name__ == "__main__":
    main()
