"""GPU-box probe: what per-row observation noise costs in the masked batched engine, and that the scalar path costs what it did.

    python tools/row_noise_timing.py --parent-lib PATH/libpsmf_hip.so [--rounds 6] [--control] [--seeds 50] [--n 295719]

Three legs at the experiment's size (19 x 295 719, r = 10, 2 passes, 50 replicas; inputs as bench.py:run_impute_config draws them),
PSMF and rPSMF, device-event times (`elapsed_ms` of impute_batch):
  (a) scalar R on the PARENT commit's library (built beforehand, --parent-lib),   (b) scalar R on this tree's library,
  (c) a (d,) vector R (log-uniform over a factor 100 around 10) on this tree's library.
One worker process per library, each with its own copy of the inputs, all alive for the whole call; the legs alternate after one
warm-up run of each, in an order that rotates from round to round (a b c, b c a, c a b, ...), so that neither a drift of the box nor
what ran just before shows in one leg only.  --control adds (a') a SECOND process of the parent's library: how far two processes
running the same code lie apart (own allocations, own code-object load address) is the scale on which (b) against (a) can be read.
Prints a table and one JSON line."""

import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def worker(lib_path, seeds, n, d=19, r=10):
    from rpsmf_amd import _capi

    if lib_path:
        _capi.LIB_PATH = lib_path
        _capi.SIGNATURES.pop("psmf_impute_run_rows", None)      # the parent's library has no such entry point
    from rpsmf_amd import impute, impute_harness as H

    rng = np.random.default_rng(20160930)
    Yorig = np.cumsum(0.05 * rng.standard_normal((d, n)), axis=1) + 10.0 * rng.random((d, 1))
    Yorig[rng.random((d, n)) < 0.01] = np.nan
    Yint = np.nan_to_num(Yorig, nan=0.0)
    np.random.seed(123)
    M, Mm, C0, X0 = [], [], [], []
    for _ in range(seeds):
        p = H.draw_problem(Yorig, 40, r)
        M.append(p["M"].astype(np.uint8)); Mm.append(p["Mmiss"].astype(np.uint8)); C0.append(p["C"]); X0.append(p["X"])
    M, Mm, C0, X0 = np.stack(M), np.stack(Mm), np.stack(C0), np.stack(X0)
    V, Q, P = 2 * np.eye(r), 0.1 * np.eye(r), np.eye(r)
    rho = 10.0 * 100.0 ** (np.random.default_rng(d + 1).random(d) - 0.5)
    print("ready", flush=True)
    for line in sys.stdin:
        robust, vector = (int(v) for v in line.split())
        res = impute.impute_batch(Yint, M, Mm, C0, X0, V, Q, rho if vector else 10.0, P, 2, 2, robust=bool(robust), lambda0=1.8)
        print(json.dumps({"ms": res["elapsed_ms"], "kernel": res["kernel"], "Epred": float(res["Epred"][0, -1]),
                          "ok": bool(np.all(res["status"] == 0))}), flush=True)


class Worker:
    def __init__(self, lib, seeds, n):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", lib or "", "--seeds", str(seeds), "--n", str(n)],
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def wait_ready(self):
        line = self.p.stdout.readline()
        if line.strip() != "ready":
            raise SystemExit(f"worker did not start: {line!r}")

    def run(self, robust, vector):
        self.p.stdin.write(f"{int(robust)} {int(vector)}\n")
        self.p.stdin.flush()
        line = self.p.stdout.readline()
        if not line:
            raise SystemExit(f"worker ended (exit status {self.p.wait()})")     # nothing more is started on the device
        return json.loads(line)

    def close(self):
        self.p.stdin.close()
        self.p.wait(timeout=120)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--worker", default=None)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--control", action="store_true")
    ap.add_argument("--seeds", type=int, default=50)
    ap.add_argument("--n", type=int, default=295_719)
    a = ap.parse_args()
    if a.worker is not None:
        return worker(a.worker, a.seeds, a.n)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("--parent-lib: the parent commit's libpsmf_hip.so")
    wa, wb = Worker(os.path.abspath(a.parent_lib), a.seeds, a.n), Worker("", a.seeds, a.n)
    wc = Worker(os.path.abspath(a.parent_lib), a.seeds, a.n) if a.control else None
    wa.wait_ready(), wb.wait_ready()
    legs = [("a", wa, 0), ("b", wb, 0), ("c", wb, 1)]
    if wc:
        wc.wait_ready()
        legs.append(("a'", wc, 0))
    times = {(leg, rb): [] for leg, _, _ in legs for rb in (0, 1)}
    kernels, answers = {}, {}
    for rnd in range(a.rounds + 1):          # round 0: warm-up, not recorded
        for rb in (0, 1):
            for leg, w, vec in legs[rnd % len(legs):] + legs[:rnd % len(legs)]:
                res = w.run(rb, vec)
                if not res["ok"]:
                    raise SystemExit(f"leg {leg}: a replica failed")
                kernels[leg] = res["kernel"]
                answers[(leg, rb)] = res["Epred"]
                if rnd:
                    times[(leg, rb)].append(res["ms"])
    for w in (wa, wb, wc):
        if w:
            w.close()
    cols = 2 * a.n
    out = {"shape": [19, a.n, 10], "seeds": a.seeds, "rounds": a.rounds, "kernels": kernels}
    print(f"masked batched engine, 19 x {a.n}, r = 10, 2 passes, {a.seeds} replicas; ms per launch (device events), {a.rounds} alternating rounds")
    print(f"{'':8s}{'leg':46s}{'runs (ms)':56s}{'median':>9s}{'us/col':>8s}")
    for rb in (0, 1):
        name = "rPSMF" if rb else "PSMF"
        assert answers[("a", rb)] == answers[("b", rb)], "scalar R: the two libraries disagree"
        med = {}
        for leg, label in (("a", "scalar R, parent library"), ("a'", "the same, second process"), ("b", "scalar R, this library"),
                           ("c", "vector R, this library")):
            if (leg, rb) not in times:
                continue
            t = times[(leg, rb)]
            med[leg] = float(np.median(t))
            print(f"{name:8s}{'(' + leg + ') ' + label + ' ' + kernels[leg][12:]:46s}{' '.join(f'{v:8.2f}' for v in t):56s}{med[leg]:9.2f}{1e3 * med[leg] / cols:8.3f}")
        ta = times[("a", rb)] + times.get(("a'", rb), [])
        inside = min(ta) <= med["b"] <= max(ta)
        print(f"{name:8s}(b) median inside the spread of the parent library's runs [{min(ta):.2f}, {max(ta):.2f}]: {inside};  (b)/(a) = {med['b'] / med['a']:.4f};  "
              f"(c)/(b) = {med['c'] / med['b']:.3f}")
        out[name] = {"a_ms": times[("a", rb)], "a2_ms": times.get(("a'", rb), []), "b_ms": times[("b", rb)], "c_ms": times[("c", rb)], "b_inside_a_spread": inside,
                     "b_over_a": med["b"] / med["a"], "c_over_b": med["c"] / med["b"], "us_per_column": {k: 1e3 * v / cols for k, v in med.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
