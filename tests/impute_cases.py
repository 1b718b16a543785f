"""Seeded random configurations of the masked, batched one-workgroup engine (psmf_impute_run / psmf_impute_run_rows: the twelve
kernels psmf_impute_kernel3<3|5|8|12|20>, their row-noise twins psmf_impute_kernel3w<...>, psmf_impute_kernel2 and
psmf_impute_kernel2w), the problem each one runs and the float64 oracle of every replica.  Pure Python:
tests/test_impute_cases_cpu.py checks the list's coverage and the conditioning of every case without a GPU,
tests/test_hip_impute_engine_net.py runs the same list on the device.

The draw is stratified: case i is aimed at the pair (kernel instance, method) number i mod len(TARGETS) and the axes are redrawn
until `expected_kernel` names that instance.  Two axes are dealt rather than drawn, because 126 cases are too few for chance to
cover them: the 21 cases of an instance and its row-noise twin ("slots": 4 + 3 methods x 3 visits) take their row count from the
instance's edge list on every other slot (kernel2: from a fixed recipe that holds all twelve row edges, r = 15 / 16 at small and
large d and the small shapes that only PSMF_IMPUTE_V3=0 sends there) and walk the list of series lengths, so that every
instance sees every n; a general Q falls on one visit of every target, dense V0 / P0 on one or two.  Everything else -- rank,
passes, band factor, lambda0, noise, observed fraction, batch, PSMF_IMPUTE_PAR, and the uniform row counts -- is drawn.

`expected_kernel` restates impute_select as a table in the words of psmf_impute_kernel_id's description (include/psmf_hip.h);
the device test asserts that the call reports the same name.
Reference: ExperimentImpute/PSMF.py:40-95, rPSMF.py:40-148, MLESMF.py:40-92, TMF.py:30-73, common.py:79-94 (through
oracle/impute_oracle.py)."""

import numpy as np

import netlib
from netlib import relerr  # noqa: F401  (the device test takes it from here)
from oracle.impute_oracle import impute_filter, mle_smf_filter, tmf_filter

METHODS = ("psmf", "rpsmf", "mle_smf", "tmf")
BAND_METHODS = ("psmf", "rpsmf", "mle_smf")          # TMF has no bands and no coverage
GROUPS = ((12, 3), (20, 5), (32, 8), (48, 12), (80, 20))      # d <= 12 / 20 / 32 / 48 / 80 -> NG four-row groups
UNIFORM = tuple(f"psmf_impute_kernel3<{ng}>" for _, ng in GROUPS) + ("psmf_impute_kernel2",)
ROW_NOISE = tuple(f"psmf_impute_kernel3w<{ng}>" for _, ng in GROUPS) + ("psmf_impute_kernel2w",)
INSTANCES = UNIFORM + ROW_NOISE
# a target is (kernel instance, method); TMF ignores R, so the row-noise instances have three methods
TARGETS = [(k, m) for k in UNIFORM for m in METHODS] + [(k, m) for k in ROW_NOISE for m in BAND_METHODS]
N_CASES = 126            # 3 x len(TARGETS)

R_LIST = (1, 2, 3, 7, 10, 13, 14)
N_LIST = (2, 3, 17, 40, 90, 255, 256, 257, 300)
N_ITER, SIGS, LAMBDAS, FRACTIONS, RHOS = (1, 2, 3), (0.5, 1.0, 2.0, 3.0), (0.5, 1.8, 5.0), (0.3, 0.6, 0.8), (1.0, 10.0, 50.0)
D_EDGES3 = (1, 2, 3, 12, 13, 20, 21, 32, 33, 48, 49, 64, 65, 80)
D_EDGES2 = (81, 191, 192, 193, 255, 256, 257, 447, 448, 449, 511, 512)
# kernel2 / kernel2w, slot -> (d, r, PSMF_IMPUTE_V3=0); None = drawn.  Slots 0 .. 11: kernel2 (psmf, rpsmf, mle_smf, tmf x 3
# visits), 12 .. 20: kernel2w.  192 / 193: wave 0 starts owning rows; 256 / 257: second row round; 448 / 449: wave 0's second row.
RECIPE2 = {0: (81, None, False), 1: (14, 15, False), 2: (192, None, False), 3: (257, 16, False), 4: (16, 16, False), 5: (448, 15, False),
           6: ("small", "small", True), 7: (511, None, False), 8: (255, None, False), 9: (191, None, False), 10: (512, None, False),
           11: (None, None, False),
           12: (16, 15, False), 13: (449, 16, False), 14: (193, None, False), 15: (34, 16, False), 16: (447, 15, False),
           17: (256, None, False), 18: ("small", "small", True), 19: (None, None, False), 20: (None, None, False)}


def d_range(instance):
    """the row counts an instance serves by default"""
    if "kernel2" in instance:
        return 81, 512
    ng = int(instance[instance.index("<") + 1:-1])
    hi = [h for h, g in GROUPS if g == ng][0]
    lo = 1 + max([h for h, g in GROUPS if h < hi], default=0)
    return lo, hi


def slot_of(i):
    """(group 0 .. 5 = position of the instance among its kind, slot 0 .. 20 within the instance and its twin)"""
    t = i % len(TARGETS)
    v = i // len(TARGETS)
    if t < 4 * len(UNIFORM):
        return t // 4, (t % 4) * 3 + v
    t -= 4 * len(UNIFORM)
    return t // 3, 12 + (t % 3) * 3 + v


# ---- the dispatch, as psmf_impute_kernel_id describes it
def noise(cs):
    """diag(R) as the caller passes it: a float, or a (d,) vector"""
    d, kind = cs["d"], cs["R_kind"]
    rng = np.random.default_rng([cs["seed"], 77])
    if kind == "scalar":
        return float(cs["rho"])
    if kind == "const_vector":
        return np.full(d, float(cs["rho"]))
    if kind == "vector":
        return 10.0 * 100.0 ** (rng.random(d) - 0.5)
    assert kind == "one_off"          # constant except one entry: first row, last row or one in between; a last-bit or a plain difference
    v = np.full(d, float(cs["rho"]))
    j = (0, d - 1, int(rng.integers(0, d)))[int(rng.integers(0, 3))]
    v[j] *= (1.0 + 2.0 ** -52, 3.0)[int(rng.integers(0, 2))]
    return v


def facts(cs):
    R = noise(cs)
    return dict(small_shape=cs["d"] <= 80 and cs["r"] <= 14,
                sw_v3=cs["env"].get("PSMF_IMPUTE_V3") != "0",
                row_noise=np.ndim(R) == 1 and bool(np.any(R != R[0])) and cs["method"] != "tmf")


# first row whose conditions all hold names the column loop (psmf_impute_kernel_id: 300 + NG, else 2)
KERNEL_TABLE = [
    ("psmf_impute_kernel3", [("small_shape", True), ("sw_v3", True)]),      # d <= 80 and r <= 14: every wave its own Gram
    ("psmf_impute_kernel2", []),                                               # d <= 512, r <= 16; PSMF_IMPUTE_V3=0: the small shapes too
]


def expected_kernel(cs):
    assert 1 <= cs["d"] <= 512 and 1 <= cs["r"] <= 16          # beyond: the masked per-step engine, not this net's
    f = facts(cs)
    name = next(n for n, conds in KERNEL_TABLE if all(f[k] == v for k, v in conds))
    w = "w" if f["row_noise"] else ""      # unequal entries of diag(R), and a method that reads R
    if name == "psmf_impute_kernel3":
        return f"{name}{w}<{next(g for h, g in GROUPS if cs['d'] <= h)}>"
    return name + w


# ---- the draw
def _draw(rng, i):
    instance, method = TARGETS[i % len(TARGETS)]
    g, k = slot_of(i)
    v = i // len(TARGETS)
    w = instance in ROW_NOISE
    lo, hi = d_range(instance)
    cs = dict(instance=instance, method=method, env={})
    if "kernel2" in instance:
        d, r, v3off = RECIPE2[k]
        if d == "small":
            d = int(rng.integers(2, 81))
            r = int(rng.choice(R_LIST))
        if d is None:
            d = int(rng.integers(lo, hi + 1))
        if r is None:
            r = int(rng.choice(R_LIST + (15, 16)))
        if v3off:
            cs["env"]["PSMF_IMPUTE_V3"] = "0"
    else:
        # one row: every noise vector is constant; and a held-out entry is then a column with no observation, where MLE-SMF's
        # reference divides by eta = 0 (MLESMF.py:79)
        lo = max(lo, 2) if (w or method == "mle_smf") else lo
        edges = [e for e in D_EDGES3 if lo <= e <= hi]
        d = edges[(k // 2) % len(edges)] if k % 2 == 0 else int(rng.integers(lo, hi + 1))
        r = int(rng.choice(R_LIST))
        if d <= 15 and rng.random() < 0.3:          # the rank next to the row count
            r = int(np.clip(d + int(rng.integers(-1, 2)), 1, 14))
    cs.update(d=d, r=r, n=N_LIST[(4 * k + g) % len(N_LIST)])
    cs["n_iter"] = int(rng.choice(N_ITER))
    cs["sig"] = float(rng.choice(SIGS))
    cs["lambda0"] = float(rng.choice(LAMBDAS))
    cs["general_Q"] = v == g % 3
    cs["dense"] = (v + i % len(TARGETS)) % 2 == 0
    cs["rho"] = float(rng.choice(RHOS))
    if w:
        cs["R_kind"] = "vector" if rng.random() < 0.6 else "one_off"
    elif method == "tmf":            # TMF ignores R: whatever it is given, the scalar kernel runs
        cs["R_kind"] = str(rng.choice(["scalar", "const_vector", "vector", "one_off"], p=[0.5, 0.1, 0.2, 0.2]))
    else:
        cs["R_kind"] = "scalar" if rng.random() < 0.75 else "const_vector"
    cs["frac"] = float(rng.choice(FRACTIONS))
    cs["batch"] = int(rng.integers(1, 4))
    if not cs["general_Q"] and rng.random() < 0.3:
        cs["env"]["PSMF_IMPUTE_PAR"] = "0"
    cs["seed"] = int(rng.integers(1 << 30))
    return cs


def case(i, salt=0):
    """Configuration number i; `salt` > 0 gives the replacements the conditioning check may ask for."""
    rng = np.random.default_rng([7300 + i, salt])
    for _ in range(2000):
        cs = _draw(rng, i)
        if expected_kernel(cs) == cs["instance"]:
            break
    else:
        raise AssertionError(f"no draw reaches {TARGETS[i % len(TARGETS)]}")
    cs["i"], cs["salt"], cs["shortened"] = i, salt, 0
    return cs


def shorten(cs):
    """The same case over half the series (not below n = 2, the ABI's minimum); None when it cannot be halved."""
    n = max(cs["n"] // 2, 2)
    if n >= cs["n"] or cs["shortened"] >= 2:
        return None
    return dict(cs, n=n, shortened=cs["shortened"] + 1)


# ---- tolerances: the bars the suite already holds this engine to on random draws (test_small_shapes_drawn_at_random; the
# docstring of test_hip_impute_row_noise.py for kernel2)
def bar(cs):
    if cs["method"] == "rpsmf" or cs["r"] >= cs["d"]:
        return 1e-7
    if cs["method"] in ("mle_smf", "tmf") or "kernel2" in cs["instance"]:
        return 1e-8
    return 1e-9


ERR_BAR, INSIDE_BAR = 1e-8, 1e-12          # Epred / Efull (relative), coverage (absolute)


# ---- the problem of a case
def empty_column(cs):
    """Does every replica of the case have a column with no observation?  d >= 12, n >= 4, not MLE-SMF (its reference divides by
    eta = 0 there, MLESMF.py:79), and r >= 3: in such a column eta = 0, N = s, and V - w w^T / s loses the direction x_p for good, so
    by the r-th pass over the column V has no direction left and N = s is a rounding residue of either sign -- a NaN band on one
    side, a 1e-9 one on the other, for no fault of either (r = 2, three passes: 1.9e-18 in the oracle where the device took the
    square root of a negative number; r = 1: the oracle's own Epred is not finite).  With r >= 3 the three passes leave a direction."""
    return cs["d"] >= 12 and cs["n"] >= 4 and cs["method"] != "mle_smf" and cs["r"] >= 3


def _mask(rng, cs):
    """One replica's M and Mmiss (d, n).  A row that is never observed (d > 3), a column observed on every other row (n >= 6), a
    column with no observation (`empty_column`), every other column with at least one observation, at least one held-out entry."""
    d, n = cs["d"], cs["n"]
    M = (rng.random((d, n)) < cs["frac"]).astype(int)
    dead = int(rng.integers(0, d)) if d > 3 else None
    if dead is not None:
        M[dead] = 0
    alive = [j for j in range(d) if j != dead]
    for t in np.flatnonzero(M.sum(axis=0) == 0):
        M[alive[int(rng.integers(0, len(alive)))], t] = 1
    cols = rng.permutation(n)
    if n >= 6:
        M[alive, cols[0]] = 1
    if empty_column(cs):
        M[:, cols[1]] = 0
    Mmiss = ((1 - M) * (rng.random((d, n)) > 0.2)).astype(float)
    if not Mmiss.any():
        free = np.argwhere(M == 0)
        if len(free) == 0:              # (d <= 3 and every entry observed: give one up, from the fullest column)
            t = int(np.argmax(M.sum(axis=0)))
            M[int(rng.integers(0, d)), t] = 0
            free = np.argwhere(M == 0)
        j, t = free[int(rng.integers(0, len(free)))]
        Mmiss[j, t] = 1.0
    return M, Mmiss


def problem(cs, perturb=None):
    """Inputs of a case: Yorig (d, n) shared by the replicas, M, Mmiss (batch, d, n), C0 (batch, d, r), X0 (batch, r, n) -- every
    replica its own -- and the shared V, P, Q, R.  `perturb` = (seed, eps): C0, X0 and Yorig times (1 + eps u), u uniform in [-1, 1]."""
    d, n, r, B = cs["d"], cs["n"], cs["r"], cs["batch"]
    rng = np.random.default_rng([cs["seed"], n])
    Yorig = np.cumsum(0.3 * rng.standard_normal((d, n)), axis=1)
    masks = [_mask(rng, cs) for _ in range(B)]
    C0 = rng.random((B, d, r))
    X0 = rng.random((B, r, n))
    Q = netlib.spd(rng, r, 0.05) if cs["general_Q"] else 0.1 * np.eye(r)
    V, P = (netlib.spd(rng, r, 2.0), netlib.spd(rng, r, 1.0)) if cs["dense"] else (2.0 * np.eye(r), np.eye(r))
    if perturb is not None:
        Yorig, C0, X0 = netlib.perturbed(dict(Yorig=Yorig, C0=C0, X0=X0), *perturb).values()
    return dict(Yorig=Yorig, M=np.stack([m for m, _ in masks]), Mmiss=np.stack([mm for _, mm in masks]), C0=C0, X0=X0, V=V, P=P, Q=Q,
                R=noise(cs))


OUTPUTS = ("C", "X", "Yrec", "YrecL", "YrecH")


def oracle(cs, pb):
    """The float64 oracle on every replica of the case: a list of dicts Epred, Efull (n_iter,), inside (None for TMF), C, X, Yrec
    and, for the methods with bands, YrecL, YrecH."""
    out = []
    for b in range(cs["batch"]):
        M, Mmiss, Yorig = pb["M"][b], pb["Mmiss"][b], pb["Yorig"]
        Y, C0, X0 = Yorig * M, pb["C0"][b], pb["X0"][b].copy()
        with np.errstate(all="ignore"):
            if cs["method"] in ("psmf", "rpsmf"):
                ep, ef, ib, st = impute_filter(Y, C0, X0, M, Mmiss, pb["V"], pb["Q"], pb["R"], pb["P"], cs["sig"], cs["n_iter"], Yorig, 0.0,
                                               robust=cs["method"] == "rpsmf", lambda0=cs["lambda0"], return_state=True)
            elif cs["method"] == "mle_smf":
                ep, ef, ib, st = mle_smf_filter(Y, C0, X0, M, Mmiss, pb["Q"], pb["R"], pb["P"], cs["sig"], cs["n_iter"], Yorig, 0.0,
                                                return_state=True)
            else:
                ep, ef, st = tmf_filter(Y, C0, X0, M, Mmiss, cs["n_iter"], Yorig, 0.0, return_state=True)
                ib = None
        rec = dict(Epred=ep[0, 1:], Efull=ef[0, 1:], inside=ib, C=st["C"], X=st["X"], Yrec=st["Yrec"])
        if ib is not None:
            rec.update(YrecL=st["YrecL"], YrecH=st["YrecH"])
        out.append(rec)
    return out


def sensitivity(cs):
    """(relerr between the oracle on the case's inputs and on inputs moved by a relative 2^-50: the worst over C, X, Yrec, YrecL,
    YrecH of every replica; the same for Epred, Efull; the smallest distance of a held-out entry from a band edge, in units of
    max(1, |y|)).  Raises what the oracle raises, and FloatingPointError for an output that is not finite."""
    pb = problem(cs)
    ref0 = oracle(cs, pb)
    ref1 = oracle(cs, problem(cs, perturb=(cs["seed"] ^ 0x5EED, 2.0 ** -50)))
    state = errs = 0.0
    margin = np.inf
    for b, (r0, r1) in enumerate(zip(ref0, ref1)):
        netlib.require_finite(r0, list(r0), f"case {cs['i']}, replica {b}")
        state = max(state, netlib.response(r0, r1, [k for k in OUTPUTS if k in r0]))
        errs = max(errs, netlib.response(r0, r1, ("Epred", "Efull")))
        if r0["inside"] is not None:
            sel = pb["Mmiss"][b] == 1
            y = pb["Yorig"][sel]
            gap = np.minimum(np.abs(y - r0["YrecL"][sel]), np.abs(y - r0["YrecH"][sel])) / np.maximum(1.0, np.abs(y))
            margin = min(margin, float(np.min(gap)))
    return state, errs, margin


BAND_MARGIN = 1e-6


def admissible(cs):
    try:
        state, errs, margin = sensitivity(cs)
    except (np.linalg.LinAlgError, FloatingPointError, ZeroDivisionError) as e:
        return False, f"{type(e).__name__}: {e}"
    ok = state <= bar(cs) / 16 and errs <= min(bar(cs), ERR_BAR) / 16 and margin >= BAND_MARGIN
    return ok, f"sensitivity {state:.2e} (bar {bar(cs):.0e}), errors {errs:.2e}, band margin {margin:.2e}"


def describe(cs):
    return f"{cs['instance']} {cs['method']} d={cs['d']} r={cs['r']} n={cs['n']}"


# What `resolve` answers for the cases it does not leave alone, {i: (salt, times shortened)}: recorded here so that the device
# test need not run the oracle three times per case; tests/test_impute_cases_cpu.py recomputes every entry (and every absence).
RESOLUTION = {42: (1, 1)}


def resolve(i):
    """netlib.resolve on this net (halving the series, not below n = 2; admitted: finite, the response to a last-bit change 16 x
    inside the bars, no held-out entry within 1e-6 of a band edge): ((salt, times shortened), log)"""
    return netlib.resolve(i, case, shorten, admissible, describe)


def device_case(i):
    return netlib.device_case(i, case, shorten, RESOLUTION.get(i, (0, 0)))
