"""The cases of the batched PMF baseline (psmf_pmf_run, rpsmf_amd/pmf.py), the problem each one runs and its answer by the numpy model
of tests/pmf_model.py.  Pure Python: tests/test_pmf_cases_cpu.py checks the list without a GPU, tests/test_hip_pmf.py runs it on the
device.

Data like the experiment's datasets: positive with a mean far above its spread -- 40 + a rank-3 signal of standard deviation 6 + unit
noise -- a tenth natively missing (shared by the replicas, as the dataset's own gaps are) and a fifth of the rest held out per replica.
Every case with n > 5 has, in every replica, a column without a training entry but with a probe entry (it moves by its momentum alone
and is still predicted), every case with d > 2 a row without a training entry; the masks of the replicas differ, so their N differ, and
no N is a multiple of num_batches (the batches of an epoch differ in size).  The first replica of the 19 x 700 case has a probe entry
that is also a training entry.

ADMISSION, by the model alone: a case is admitted when the model is finite, max |W|, |P| <= 10 and its two summation orders agree to
1e-13 (conftest.relerr) in Efull, P, W and Yrec.  Every listed case is admitted -- tests/test_pmf_cases_cpu.py asserts it -- and none
may be left out: data and seeds are chosen so.  The tiny shape, 3 x 23 with 4 batches of about 8 entries, diverges at the reference's
epsilon = 50 (|W| about 1e12 after two epochs), so it runs at epsilon = 2.  `diverging()` is the status test's pair of replicas."""

import functools

import numpy as np

import pmf_model
from conftest import relerr

# (d, n, r, num_batches, epochs, batch, epsilon)
SHAPES = (
    (1, 40, 1, 1, 1, 1, 50),
    (3, 23, 2, 4, 2, 2, 2),
    (19, 700, 10, 9, 2, 3, 50),
    (27, 257, 10, 9, 2, 2, 50),
    (80, 130, 16, 9, 3, 2, 50),
    (505, 96, 10, 9, 2, 2, 50),
    (512, 33, 16, 5, 1, 1, 50),
    (17, 3000, 5, 9, 2, 4, 50),
    (200, 70, 7, 6, 2, 2, 50),       # not on the issue's list: the instance of 129 <= d <= 256 (16 row tiles in registers), which none of its shapes reaches
)
CASES = tuple(dict(i=i, d=d, n=n, r=r, nb=nb, epochs=ep, batch=B, epsilon=eps, name=f"{d}x{n}_r{r}_nb{nb}_e{ep}_b{B}")
              for i, (d, n, r, nb, ep, B, eps) in enumerate(SHAPES))
COLS_CASES = (2, 7)              # 19 x 700 and 17 x 3000: run again under PSMF_PMF_COLS
BOTH_CASE = 2                    # its first replica has a probe entry that is also a training entry
ADMIT_TOL = 1e-13
ADMIT_MAX = 10.0
TOL = 1e-12                      # device against model: about 400 x the order sensitivity measured on the CPU (2.8e-15)
LMD, MOMENTUM = 0.01, 0.8


def by_name(name):
    return [c for c in CASES if c["name"] == name][0]


@functools.lru_cache(maxsize=None)
def problem(i, seed=2025):
    """dict(YorgInt (d, n), M, Mmiss (batch, d, n) uint8, C0, X0, perms: per replica a list of `epochs` permutations)"""
    cs = CASES[i]
    d, n, r, nb, B = cs["d"], cs["n"], cs["r"], cs["nb"], cs["batch"]
    rng = np.random.default_rng([seed, i])
    sig = rng.standard_normal((d, 3)) @ rng.standard_normal((3, n))
    sig *= 6.0 / max(float(sig.std()), 1e-12)
    Y = 40.0 + sig + rng.standard_normal((d, n))
    native = rng.random((d, n)) < 0.1
    if n > 5:
        native[0, n // 2:n // 2 + B] = False          # the probe entries of the columns without a training entry
    YorgInt = np.where(native, 0.0, Y)
    M = np.zeros((B, d, n), dtype=np.uint8)
    Mmiss = np.zeros((B, d, n), dtype=np.uint8)
    perms = []
    for b in range(B):
        held = (rng.random((d, n)) < 0.2) & ~native
        m = ~native & ~held
        if n > 5:
            c = n // 2 + b                            # a column without a training entry, but with a probe entry
            m[:, c] = False
            held[0, c] = True
        if d > 2:
            m[d - 1 - (b % 2), :] = False             # a row without a training entry (it may hold probe entries)
        if i == BOTH_CASE and b == 0:
            ii, jj = np.nonzero(m)
            held[ii[5], jj[5]] = True                 # a probe entry that is also a training entry
        while (nb > 1 and int(m.sum()) % nb == 0) or any(int(m.sum()) == int(M[k].sum()) for k in range(b)):
            ii, jj = np.nonzero(m)
            m[ii[-1], jj[-1]] = False                 # N is no multiple of num_batches and differs between the replicas
        M[b], Mmiss[b] = m, held
        N = int(m.sum())
        perms.append([rng.permutation(N) for _ in range(cs["epochs"])])
    return dict(YorgInt=YorgInt, M=M, Mmiss=Mmiss, C0=rng.random((B, d, r)), X0=rng.random((B, r, n)), perms=perms)


def run_model(pb, b, cs, order="reference", epochs=None, epsilon=None):
    return pmf_model.pmf_model(pb["YorgInt"], pb["M"][b], pb["Mmiss"][b], pb["C0"][b], pb["X0"][b], pb["perms"][b],
                               epochs=cs["epochs"] if epochs is None else epochs, epsilon=cs["epsilon"] if epsilon is None else epsilon,
                               lmd=LMD, momentum=MOMENTUM, num_batches=cs["nb"], order=order)


@functools.lru_cache(maxsize=None)
def reference(i):
    """the model's answer for every replica of case i: a tuple of dicts (computed once, shared by the tests, not to be modified)"""
    pb = problem(i)
    return tuple(run_model(pb, b, CASES[i]) for b in range(CASES[i]["batch"]))


KEYS = ("Efull", "P", "W", "Yrec")


def admission(i):
    """(admitted, text): the rule of the module docstring, replica by replica"""
    pb, ref = problem(i), reference(i)
    worst, size = 0.0, 0.0
    for b in range(CASES[i]["batch"]):
        other = run_model(pb, b, CASES[i], order="sorted")
        if not all(np.all(np.isfinite(ref[b][k])) and np.all(np.isfinite(other[k])) for k in KEYS):
            return False, f"{CASES[i]['name']}: replica {b} is not finite in the model"
        size = max(size, float(np.max(np.abs(ref[b]["W"]))), float(np.max(np.abs(ref[b]["P"]))))
        worst = max([worst] + [relerr(other[k], ref[b][k]) for k in KEYS])
    ok = size <= ADMIT_MAX and worst <= ADMIT_TOL
    return ok, f"{CASES[i]['name']}: max |W|, |P| = {size:.3g} (<= {ADMIT_MAX}), summation orders part by {worst:.2e} (<= {ADMIT_TOL})"


def device_args(pb):
    return pb["YorgInt"], pb["M"], pb["Mmiss"], pb["C0"], pb["X0"], pb["perms"]


def device_kwargs(cs):
    return dict(epochs=cs["epochs"], epsilon=cs["epsilon"], lmd=LMD, momentum=MOMENTUM, num_batches=cs["nb"])


# ---- the reference's stored answers (tests/golden/impute_kat_pmf.npz)
KAT_FILES = tuple((ds, pct) for ds in ("pm25", "pm10", "sp500") for pct in (20, 30, 40))
KAT_EPOCHS, KAT_R = 2, 10        # PMF.py:190-191


@functools.lru_cache(maxsize=None)
def kat_inputs(ds, pct, n_rep):
    """The inputs of the first n_rep repeats behind <ds>_<pct>_PMF.json, as PMF.py:193-224 draws them: per repeat the mask and the
    factors (kat_replay.draws) and then, from the RNG state those leave, the permutations of pmf() -- the script restores that state
    after the call, so the next repeat's inputs do not depend on them.  A list of dicts: YorigInt, M, Mmiss, C, X, perms, hY / hC / hX.
    The caller's RNG state is put back."""
    import kat_replay

    keep = np.random.get_state()
    Yorig = kat_replay.fixture(ds)["Yorig"]
    YorigInt = np.nan_to_num(Yorig, nan=0.0)
    out = []
    for k in range(n_rep):
        dr = kat_replay.draws(ds, pct, k + 1, r=KAT_R, want={k})[0]      # seeds the RNG and leaves it behind repeat k's inputs
        dr["perms"] = pmf_model.draw_perms(int(dr["M"].sum()), KAT_EPOCHS)
        dr["YorigInt"] = YorigInt
        out.append(dr)
    np.random.set_state(keep)
    return out


# ---- a replica that diverges, next to a healthy one
DIVERGING_CASE, DIVERGING_SCALE = "27x257_r10_nb9_e2_b2", 30.0


@functools.lru_cache(maxsize=None)
def diverging():
    """The 27 x 257 case with the C0 of replica 0 thirty times as large: its first predictions are off by three orders of magnitude
    and the steps of epsilon = 50 leave the finite range within the first epoch -- the model says so -- while replica 1 is the
    case's own, healthy one.  Returns (problem, case, the model's answers)."""
    cs = by_name(DIVERGING_CASE)
    pb = dict(problem(cs["i"]))
    pb["C0"] = pb["C0"].copy()
    pb["C0"][0] *= DIVERGING_SCALE
    return pb, cs, tuple(run_model(pb, b, cs) for b in range(2))
