"""The cases of the masked per-step engine with per-row observation noise (cfg.masked with cfg.nonuniform_R: the masked weighted
Gram psmf_mwgram_mfma, rpsmf_amd/csrc/psmf_masked.hip), the problem each one runs and the float64 oracle of it.  Pure Python:
tests/test_masked_noise_cases_cpu.py checks the list without a GPU, tests/test_hip_masked_row_noise.py runs it on the device.

One builder for every case (`problem`, in the style of tests/test_hip_masked_large.py::_problem):
    series   Yorig = cumsum(0.3 N(0, 1)) + 3 U(0, 1) per row
    mask     60 % observed, row 3 never observed, column 5 empty (not for MLE-SMF: it divides by eta = 0 there, MLESMF.py:79)
    noise    rho_i = 10 * 100^(u_i - 1/2): diag(R) over a 100 x spread
    state    V = 2 I, Q = 0.1 I, P = I, lambda0 = 1.8, sig = 2
The weighted Gram kernel runs 256 workgroups of NW = 8 waves, one slab of 16 rows per wave and trip: a wave makes a second trip
beyond 16 * 256 * 8 = 32 768 rows.  The big case is one row past that bound; its column SECOND_TRIP_COLUMN has observations only
in the slabs of a second trip (as gram_cases.mask_of's column 4): a Gram that drops them solves with G = 0 there.
Reference: ExperimentImpute/PSMF.py:40-95 (R row by row: 70-72), rPSMF.py:40-148 (91-98), MLESMF.py:40-92 (70-76)."""

from functools import lru_cache

import numpy as np

from netlib import f32_round, relerr  # noqa: F401  (the tests take relerr from here)
from oracle.impute_oracle import impute_filter, mle_smf_filter

N_WG, SLAB, WGRAM_NW = 256, 16, 8           # kMGramWG and wgram_inst (psmf_step.hip), mgram_body's slab (psmf_masked.hip)
BOUND = SLAB * N_WG * WGRAM_NW              # rows up to which every wave of the weighted Gram takes one slab
SECOND_TRIP_COLUMN = 7
SIG, LAMBDA0 = 2.0, 1.8
METHOD_CODE = {"psmf": 1, "rpsmf": 1, "mle_smf": 2}          # cfg.masked (include/psmf_hip.h)

# (d, n, r, passes, storage, methods)
SHAPES = [
    (700, 60, 3, 2, "f64", ("psmf", "rpsmf", "mle_smf")),
    (40, 90, 24, 2, "f64", ("psmf", "rpsmf", "mle_smf")),          # fewer slabs than waves, NT = 2
    (2001, 50, 20, 2, "f64", ("psmf", "rpsmf")),                    # also on two uneven shards
    (1041, 40, 40, 2, "f64", ("psmf", "rpsmf")),                    # NT = 3, the masked solve beyond r = 32
    (530, 30, 64, 2, "f64", ("psmf", "rpsmf")),                     # NT = 4
    (BOUND + 1, 24, 10, 1, "f64", ("psmf", "rpsmf")),               # a second trip of one row
    (700, 60, 3, 2, "f32", ("psmf", "rpsmf", "mle_smf")),
    (2001, 50, 20, 2, "f32", ("psmf", "rpsmf")),
]
CASES = [dict(d=d, n=n, r=r, passes=p, storage=s, method=m, robust=m == "rpsmf", masked=True) for d, n, r, p, s, ms in SHAPES for m in ms]
IDS = [f"{c['d']}x{c['n']}r{c['r']}-{c['method']}-{c['storage']}" for c in CASES]


def find(d, r, method, storage="f64"):
    return next(c for c in CASES if (c["d"], c["r"], c["method"], c["storage"]) == (d, r, method, storage))


def trips(d_local):
    """the most slabs one wave of the weighted Gram takes"""
    return -(-((d_local + SLAB - 1) // SLAB) // (N_WG * WGRAM_NW))


def problem(cs, perturb=None):
    """dict(Yorig, M, Mmiss, C0, X0, rho, V, Q, P) of a case, (d, n) as the reference takes them.  `perturb` = (seed, eps): C0 and
    X0 times (1 + eps u), u uniform in [-1, 1] (the oracle's own arithmetic is float64 whatever the device stores)."""
    d, n, r = cs["d"], cs["n"], cs["r"]
    rng = np.random.default_rng(7000 + d + r)
    Yorig = np.cumsum(0.3 * rng.standard_normal((d, n)), axis=1) + 3.0 * rng.random((d, 1))
    M = (rng.random((d, n)) > 0.4).astype(int)
    if trips(d) >= 2:
        M[:, SECOND_TRIP_COLUMN] = 0
        M[BOUND:, SECOND_TRIP_COLUMN] = 1
    M[3] = 0
    if cs["method"] != "mle_smf":
        M[:, 5] = 0
    Mmiss = ((1 - M) * (rng.random((d, n)) > 0.1)).astype(float)
    C0, X0 = rng.random((d, r)), rng.random((r, n))
    rho = 10.0 * 100.0 ** (rng.random(d) - 0.5)
    if cs["storage"] == "f32":
        Yorig, C0 = f32_round(Yorig), f32_round(C0)
    if perturb is not None:
        prng = np.random.default_rng(perturb[0])
        C0 = C0 * (1.0 + perturb[1] * prng.uniform(-1, 1, C0.shape))
        X0 = X0 * (1.0 + perturb[1] * prng.uniform(-1, 1, X0.shape))
    return dict(Yorig=Yorig, M=M, Mmiss=Mmiss, C0=C0, X0=X0, rho=rho, V=2 * np.eye(r), Q=0.1 * np.eye(r), P=np.eye(r))


def run_oracle(cs, pb, rho):
    """the reference's filter over the case's passes with R = diag(rho) (a vector) or rho I (a scalar) ->
    dict(C, X (n, r), Yrec, YrecL, YrecH (n, d), Epred, Efull (passes,), coverage)"""
    Y, M, X = pb["Yorig"], pb["M"], pb["X0"].copy()
    with np.errstate(all="ignore"):
        if cs["method"] == "mle_smf":
            ep, ef, inside, st = mle_smf_filter(Y * M, pb["C0"], X, M, pb["Mmiss"], pb["Q"], rho, pb["P"], SIG, cs["passes"], Y, 0.0, return_state=True)
        else:
            ep, ef, inside, st = impute_filter(Y * M, pb["C0"], X, M, pb["Mmiss"], pb["V"], pb["Q"], rho, pb["P"], SIG, cs["passes"], Y, 0.0,
                                               robust=cs["robust"], lambda0=LAMBDA0, return_state=True)
    return dict(C=st["C"], X=st["X"].T.copy(), Yrec=st["Yrec"].T.copy(), YrecL=st["YrecL"].T.copy(), YrecH=st["YrecH"].T.copy(),
                Epred=ep[0, 1:].copy(), Efull=ef[0, 1:].copy(), coverage=float(inside))


@lru_cache(maxsize=None)
def _cached(i):
    pb = problem(CASES[i])
    return pb, run_oracle(CASES[i], pb, pb["rho"])


def reference(cs):
    """(problem, oracle result) of a case, computed once and shared by the tests that need it: do not modify either"""
    return _cached(CASES.index(cs))


COMPARED = ("C", "X", "Yrec", "YrecL", "YrecH")
