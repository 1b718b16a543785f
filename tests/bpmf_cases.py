"""The cases of the batched BPMF baseline (psmf_bpmf_run, rpsmf_amd/bpmf.py), the problem each one runs and its answer by the numpy
model of tests/bpmf_model.py.  Pure Python: tests/test_bpmf_cases_cpu.py checks the list without a GPU, tests/test_hip_bpmf.py runs it
on the device.

Data as in tests/pmf_cases.py: positive with a mean far above its spread -- 40 + a rank-3 signal of standard deviation 6 + unit noise
-- a tenth natively missing (shared by the replicas) and a fifth of the rest held out per replica.  Every case with n > 5 has, in
every replica, a column without a training entry but with a probe entry (its precision matrix is alpha alone), every case with d > 2
a row without one; the masks, factors and draws of the replicas differ.  The tiny shapes (fewer than 1000 entries) run the warm
start at epsilon = 2 with fewer batches, as pmf_cases does: at the reference's 50 they diverge, and 2 x 5 has fewer than 9 training
entries.

The kernels have one instance each (d, n and r are run-time values), so the shapes are chosen for the paths inside them: d that is
no multiple of the 4 rows of a matrix-core product (2, 3, 19, 27, 505, 17) and d that is; n below, at and above the 4 columns a
wave takes at a time and the 16 a workgroup's four waves do (5, 16, 17, 33); r from 2 to the full tile of 16, with 15 one short of
it; more than one workgroup per replica (700, 3000 columns; the row partials are then added across workgroups) and exactly one.

ADMISSION, by the model alone: a case is admitted when the model is finite in every replica and its two algebras and two summation
orders -- four runs -- agree to 1e-13 (conftest.relerr) in Efull, P, W and Yrec.  Every listed case is admitted --
tests/test_bpmf_cases_cpu.py asserts it -- and none may be left out: data and seeds are chosen so."""

import functools

import numpy as np

import bpmf_model
from conftest import relerr

# (d, n, r, epochs, batch)
SHAPES = (
    (2, 5, 2, 1, 1),
    (3, 23, 2, 2, 2),
    (19, 700, 10, 2, 3),
    (27, 257, 10, 2, 2),
    (80, 130, 16, 3, 2),
    (200, 70, 7, 2, 2),
    (505, 96, 10, 2, 2),
    (512, 33, 16, 1, 1),
    (17, 3000, 5, 2, 4),
    (21, 16, 15, 1, 1),
    (21, 17, 15, 1, 1),
    (21, 33, 15, 2, 2),
)
TINY = 1000                      # entries below which the warm start runs at epsilon = 2
CASES = tuple(dict(i=i, d=d, n=n, r=r, epochs=ep, batch=B, name=f"{d}x{n}_r{r}_e{ep}_b{B}",
                   warm_start=dict(epsilon=2, num_batches=1 if n <= 5 else 4) if d * n < TINY else None)
              for i, (d, n, r, ep, B) in enumerate(SHAPES))
COLS_CASES = (2, 8)              # 19 x 700 and 17 x 3000: run again under PSMF_BPMF_COLS
ADMIT_TOL = 1e-13
# Device against model.  The rule: the larger of 1e-12 (PMF's bar) and 50 x the largest disagreement the CPU model shows between its
# two algebras and its two summation orders, over all cases and the known-answer repeats the device tests replay (the first five of
# the nine files).  MEASURED is that disagreement -- a property of the reference arithmetic, taken without a device: 9.7e-14, in P of
# the fourth repeat of LondonAir_PM25 at 20 % (profiles/bpmf_model_kat.txt; Efull parts by at most 7e-16 there, and the cases stay
# below 2.2e-15).  tests/test_bpmf_cases_cpu.py measures it again on the cases and three of those repeats (8.1e-14).
MEASURED = 9.7e-14
TOL = max(1e-12, 50 * MEASURED)
BETA = 2
VARIANTS = (("reference", "reversed"), ("device", "reference"), ("device", "reversed"))      # beside ("reference", "reference")


def by_name(name):
    return [c for c in CASES if c["name"] == name][0]


def draw_seeded(seed, d, n, r, N, epochs):
    """rpsmf_amd.bpmf.draw_bpmf from a seeded global RNG, whose state is put back"""
    from rpsmf_amd.bpmf import draw_bpmf

    keep = np.random.get_state()
    np.random.seed(seed)
    try:
        return draw_bpmf(d, n, r, N, epochs)
    finally:
        np.random.set_state(keep)


@functools.lru_cache(maxsize=None)
def problem(i, seed=2026):
    """dict(YorgInt (d, n), M, Mmiss (batch, d, n) uint8, C0, X0, draws: per replica the record of draw_bpmf)"""
    cs = CASES[i]
    d, n, r, B = cs["d"], cs["n"], cs["r"], cs["batch"]
    rng = np.random.default_rng([seed, i])
    sig = rng.standard_normal((d, 3)) @ rng.standard_normal((3, n))
    sig *= 6.0 / max(float(sig.std()), 1e-12)
    Y = 40.0 + sig + rng.standard_normal((d, n))
    native = rng.random((d, n)) < 0.1
    if n > 5:
        native[0, n // 2:n // 2 + B] = False          # the probe entries of the columns without a training entry
    else:
        native[0, 0] = False
    YorgInt = np.where(native, 0.0, Y)
    M = np.zeros((B, d, n), dtype=np.uint8)
    Mmiss = np.zeros((B, d, n), dtype=np.uint8)
    draws = []
    for b in range(B):
        held = (rng.random((d, n)) < 0.2) & ~native
        if n <= 5:
            held[0, 0] = True                         # (a probe entry, whatever the draw)
        m = ~native & ~held
        if n > 5:
            c = n // 2 + b                            # a column without a training entry, but with a probe entry
            m[:, c] = False
            held[0, c] = True
        if d > 2:
            m[d - 1 - (b % 2), :] = False             # a row without a training entry (it may hold probe entries)
        M[b], Mmiss[b] = m, held
        draws.append(draw_seeded([seed, i, b], d, n, r, int(m.sum()), cs["epochs"]))
    return dict(YorgInt=YorgInt, M=M, Mmiss=Mmiss, C0=rng.random((B, d, r)), X0=rng.random((B, r, n)), draws=draws)


def run_model(pb, b, cs, algebra="reference", order="reference", draws=None):
    return bpmf_model.bpmf_model(pb["YorgInt"], pb["M"][b], pb["Mmiss"][b], pb["C0"][b], pb["X0"][b], pb["draws"][b] if draws is None else draws,
                                 epochs=cs["epochs"], beta=BETA, algebra=algebra, order=order, warm_start=cs["warm_start"])


@functools.lru_cache(maxsize=None)
def reference(i):
    """the model's answer for every replica of case i: a tuple of dicts (computed once, shared by the tests, not to be modified)"""
    pb = problem(i)
    return tuple(run_model(pb, b, CASES[i]) for b in range(CASES[i]["batch"]))


KEYS = ("Efull", "P", "W", "Yrec")


def disagreement(ref, others):
    """the largest conftest.relerr between a model answer and its variants, over KEYS"""
    return max(relerr(o[k], ref[k]) for o in others for k in KEYS)


@functools.lru_cache(maxsize=None)
def admission(i):
    """(admitted, text, disagreement): the rule of the module docstring, replica by replica"""
    pb, ref = problem(i), reference(i)
    worst = 0.0
    for b in range(CASES[i]["batch"]):
        others = [run_model(pb, b, CASES[i], algebra=a, order=o) for a, o in VARIANTS]
        if not all(np.all(np.isfinite(res[k])) for res in [ref[b]] + others for k in KEYS):
            return False, f"{CASES[i]['name']}: replica {b} is not finite in the model", np.inf
        worst = max(worst, disagreement(ref[b], others))
    return worst <= ADMIT_TOL, f"{CASES[i]['name']}: algebras and summation orders part by {worst:.2e} (<= {ADMIT_TOL})", worst


def device_args(pb):
    return pb["YorgInt"], pb["M"], pb["Mmiss"], pb["C0"], pb["X0"], pb["draws"]


def device_kwargs(cs):
    return dict(epochs=cs["epochs"], beta=BETA, warm_start=cs["warm_start"])


# ---- the reference's stored answers (tests/golden/impute_kat_bpmf.npz)
KAT_FILES = tuple((ds, pct) for ds in ("pm25", "pm10", "sp500") for pct in (20, 30, 40))
KAT_EPOCHS, KAT_R = 2, 10        # BPMF.py:325-326


@functools.lru_cache(maxsize=None)
def kat_inputs(ds, pct, n_rep):
    """The inputs of the first n_rep repeats behind <ds>_<pct>_BPMF.json, as BPMF.py:336-375 draws them: per repeat the mask and the
    factors (kat_replay.draws) and then, from the RNG state those leave, the draws of bpmf() -- the script restores that state after
    the call, so the next repeat's inputs do not depend on them.  A list of dicts: YorigInt, M, Mmiss, C, X, draws, hY / hC / hX.
    The caller's RNG state is put back."""
    import kat_replay
    from rpsmf_amd.bpmf import draw_bpmf

    keep = np.random.get_state()
    Yorig = kat_replay.fixture(ds)["Yorig"]
    YorigInt = np.nan_to_num(Yorig, nan=0.0)
    d, n = Yorig.shape
    out = []
    for k in range(n_rep):
        dr = kat_replay.draws(ds, pct, k + 1, r=KAT_R, want={k})[0]      # seeds the RNG and leaves it behind repeat k's inputs
        dr["draws"] = draw_bpmf(d, n, KAT_R, int(dr["M"].sum()), KAT_EPOCHS)
        dr["YorigInt"] = YorigInt
        out.append(dr)
    np.random.set_state(keep)
    return out


def kat_model(dr, algebra="reference", order="reference"):
    return bpmf_model.bpmf_model(dr["YorigInt"], dr["M"], dr["Mmiss"], dr["C"], dr["X"], dr["draws"], epochs=KAT_EPOCHS, beta=BETA, algebra=algebra,
                                 order=order)


# ---- a replica whose precision matrix is not positive definite, next to a healthy one
NONSPD_CASE = "27x257_r10_e2_b2"


@functools.lru_cache(maxsize=None)
def nonspd():
    """The 27 x 257 case with the Bartlett factors of replica 0 set to zero -- their diagonals are zero, and so is everything else, so
    alpha = 0 exactly and (b0 + N) alpha has no Cholesky factor: the reference raises numpy.linalg.LinAlgError from inv() there, and
    the model says so.  Replica 1 is the case's own, healthy one.  Returns (problem, case)."""
    cs = by_name(NONSPD_CASE)
    pb = dict(problem(cs["i"]))
    bad = dict(pb["draws"][0])
    bad["bartlett"] = np.zeros_like(bad["bartlett"])
    pb["draws"] = [bad, pb["draws"][1]]
    return pb, cs
