"""GPU-box tool: the three accuracies of the change-point experiment (ExperimentChange/main.m) for N series at one contamination
level, end to end through this library.

    python tools/change_experiment.py [--series 1000] [--dof 1.5] [--seed 0]

The data are this file's own numpy restatement of the experiment's generator: a two-mass spring system stepped by explicit Euler
(dt = 0.1, spring constants 5, 5), observed through a random 20 x 4 map with unit Gaussian noise, 1200 samples; from sample 601 on
three random rows follow a second system (spring constants 1, 1); every entry is hit by Student-t noise of `--dof` degrees of freedom
with probability 0.05.  Per series, as main.m does:
    PSMF + search   the Matern-3/2 filter (rpsmf_amd.ssm.linear_psmf_batch, r = 10, rho = 1e-3), then find_changepoint on the ten
                    position states from sample 400 on; a hit when it lands within 30 samples of 601
    search alone    find_changepoint on the raw series from sample 400 on; the same rule
    BOCPD           mvbocpd_batch on the samples from 400 on; a hit when a declared change point lies strictly between 570 and 630
Prints the three accuracies with the time each stage took, and one JSON line.  Not a test: random draws differ from Matlab's."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spring_states(L, k, k2):
    """(4, L) states of the two damped masses, explicit Euler with dt = 0.1 and a unit input"""
    m, b, m2, b2, dt = 4.0, 0.5, 2.0, 0.5, 0.1
    A = np.zeros((4, 4))
    A[:2, :2] = [[0.0, 1.0], [-k / m, -b / m]]
    A[2:, 2:] = [[0.0, 1.0], [-k2 / m2, -b2 / m2]]
    Bu = np.array([0.0, 1.0 / m, 0.0, 1.0 / m2])
    step = np.eye(4) + dt * A
    x = np.array([1.0, 0.0, 0.0, -1.0])
    xs = np.empty((4, L))
    for i in range(L):
        xs[:, i] = x
        x = step @ (x + Bu)
    return xs


def make_series(rng, dof, m=20, L=1200, m2=3, L2=600, cont=0.05):
    Y = rng.standard_normal((m, 4)) @ spring_states(L, 5.0, 5.0) + rng.standard_normal((m, L))
    Y2 = rng.standard_normal((m2, 4)) @ spring_states(L2, 1.0, 1.0) + rng.standard_normal((m2, L2))
    Y[rng.choice(m, m2, replace=False), L - L2:] = Y2
    hit = rng.random((m, L)) < cont
    Y[hit] += rng.standard_t(dof, size=int(hit.sum()))
    return Y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=1000)
    ap.add_argument("--dof", type=float, default=1.5)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from rpsmf_amd.changepoint import find_changepoint, mvbocpd_batch
    from rpsmf_amd.ssm import linear_psmf_batch, matern32_state_space

    rng = np.random.default_rng(a.seed)
    N, m, L, r, st, SP = a.series, 20, 1200, 10, 400, 601
    Y = np.stack([make_series(rng, a.dof) for _ in range(N)])
    A, Q, H = matern32_state_space(0.1, 0.1, 1e-3, r)
    C0 = rng.standard_normal((N, m, r))
    x0 = rng.standard_normal((N, 2 * r)) @ np.linalg.cholesky(Q).T
    t0 = time.perf_counter()
    X = linear_psmf_batch(Y, C0, x0, np.eye(r), np.eye(2 * r), A, Q, H, 1e-3, carry_P=False)["X"]
    t1 = time.perf_counter()
    k_f = find_changepoint(X[:, :r, st - 1:])            # the positions come first (matern32_state_space)
    k_raw = find_changepoint(Y[:, :, st - 1:])
    t2 = time.perf_counter()
    res = mvbocpd_batch(Y[:, :, st - 1:], max_changepoints=64)
    t3 = time.perf_counter()
    acc_f = float(np.mean(np.abs(k_f + (st - 1) - SP) < 30))
    acc_raw = float(np.mean(np.abs(k_raw + (st - 1) - SP) < 30))
    acc_b = float(np.mean([np.any((st + c > 570) & (st + c < 630)) for c in res["changepoints"]]))
    print(f"{N} series, 5 % contamination with t({a.dof}) noise, change at sample {SP}:")
    print(f"  PSMF + search  accuracy {acc_f:.3f}   (filter {1e3 * (t1 - t0):.0f} ms)")
    print(f"  search alone   accuracy {acc_raw:.3f}   (both searches {1e3 * (t2 - t1):.0f} ms on the host)")
    print(f"  BOCPD          accuracy {acc_b:.3f}   ({1e3 * (t3 - t2):.0f} ms, kernels {res['elapsed_ms']:.0f} ms; "
          f"{int((res['status'] != 0).sum())} series failed)")
    print(json.dumps(dict(series=N, dof=a.dof, psmf_search=acc_f, search=acc_raw, bocpd=acc_b, filter_ms=1e3 * (t1 - t0),
                          search_ms=1e3 * (t2 - t1), bocpd_ms=1e3 * (t3 - t2), bocpd_kernel_ms=float(res["elapsed_ms"]))))


if __name__ == "__main__":
    main()
