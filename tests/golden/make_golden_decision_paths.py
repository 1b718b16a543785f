"""Records tests/golden/filter3_decision_paths.npz: what the library in rpsmf_amd/lib leaves for every case of
tests/decision_path_cases.py (counters of both passes, blake2b digests of every array; tests/test_hip_filter3_decision_paths.py).
Run once, on an MI355X, on the build of the commit whose results are to be kept:

    python tests/golden/make_golden_decision_paths.py tests/golden/filter3_decision_paths.npz

Prints, per case, the counters per timestep, whether the second pass took the path the case is named for, and the worst error
against the float64 oracle as a fraction of the bar.  `--probe` records nothing: it runs every problem under a grid of tolerance /
problem settings and prints the counters, which is how decision_path_cases.SETTINGS were chosen."""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import blocked_cases as BC                      # noqa: E402
import decision_path_cases as DP                # noqa: E402
import test_hip_filter3_decision_paths as TD    # noqa: E402


def _worst(cs, passes, ref):
    tol, worst = BC.bar(cs), 0.0
    for p, want in zip(passes, ref):
        for k in ("C", "V", "mu", "P"):
            worst = max(worst, BC.relerr(p["state"][k], want[k]) / tol)
        worst = max(worst, BC.relerr(p["y_pred"], want["y_pred"]) / tol)
    return worst


def _line(cs, passes, ref):
    T = cs["T"]
    per = " | ".join(f"it {p['counters']['ns_iterations'] / T:.3f} sw {p['counters']['sweep_steps'] / T:.3f} fl {p['counters']['ns_failed'] / T:.3f}" for p in passes)
    return f"{cs['name']:36s} env={cs['env']} :: {per} :: err/bar {_worst(cs, passes, ref):.3g}"


def main():
    from rpsmf_amd import _capi as c

    if sys.argv[1] == "--probe":
        tols = ("1e-2", "1e-3", "1e-4", "1e-5", "1e-6", "1e-8")
        grid = [{}] + [{"PSMF_NS_TOL": t} for t in tols]
        for r in DP.SHAPES:
            for robust in (False, True):
                for storage in ("f64", "f32"):
                    for rho, q in ((1.0, 1e-2), (1.0, 1e-3), (1e3, 1e-3), (1e6, 1e-3), (1e6, 1e-4)):
                        for env in grid:
                            cs = DP.make(f"r{r}-{int(robust)}-{storage}-rho{rho:g}-q{q:g}", r, robust, "f64", "more", rho=rho, q=q, env=env)
                            cs["storage"], cs["v0"] = storage, 0.02 if storage == "f32" else 0.1
                            pb, ref = TD._reference(cs)
                            print(_line(cs, TD.drive(c, cs, pb), ref), flush=True)
        return
    rec = {}
    for cs in DP.cases():
        pb, ref = TD._reference(cs)
        passes = TD.drive(c, cs, pb)
        print(_line(cs, passes, ref), "::", DP.expect(cs, [p["counters"] for p in passes]) or "path ok", flush=True)
        for k, v in TD.record_of(passes).items():
            rec[f"{cs['name']}/{k}"] = v
    np.savez_compressed(sys.argv[1], **rec)


if __name__ == "__main__":
    main()
