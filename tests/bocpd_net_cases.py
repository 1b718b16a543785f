"""A seeded net of configurations for the batched Bayesian online change-point detection (psmf_bocpd_run), judged against the
extended-precision model of tests/bocpd_cases.py (extended_model: np.longdouble, lgamma from mpmath).  Pure Python:
tests/test_bocpd_net_cases_cpu.py admits the list without a GPU, tests/test_hip_bocpd_net.py runs it on the device.

WALKED, so that the coverage holds for any seed (`walk`):
    every dim 1 .. 32 -- the chain kernel is one separately compiled instance per dim
    the six dims on either side of a change of the chain kernel's lanes per workgroup NL (12 | 13: 256 -> 128, 17 | 18: 128 -> 64,
        24 | 25: 64 -> 32) with T = NL - 1, NL, NL + 1 and 2 NL + 1 each: one block short of full, exactly full, a last block with a
        single birth, three blocks
    every dim with a T > NL(dim) at least: every instance crosses a block edge (t0 = blockIdx.x * NL, the b > t skip)
    T = 63, 64, 65 (a wave of the post kernel) and 255, 256, 257 (its workgroup) at dims <= 12
DRAWN per case (`draw`): batch 1 .. 5, every replica its own series; lam log-uniform on [1.5, 1000]; kappa0 log-uniform on [0.05, 20];
    nu0 = dim - 1 + log-uniform [0.05, 10] (down to 0.05 above the bound); the data's scale s in {1e-3, 1, 1e3} with sigma0 = s^2 x
    log-uniform [0.25, 4] (the well-scaled family: the float64 model is itself good to 1e-11 there and not elsewhere, see
    tests/test_hip_bocpd_edges.py for the ill-scaled prior); drop, settle, confirm in 0 .. 12 (settle = 0 can never confirm);
    max_changepoints in {0, 1, 16}; the kind of series -- none, one shift, alternating shifts at 2 .. 5 places, a variance step.
    The segments' means are +-base, 1.5 s .. 3 s away from the prior's 0: at the larger dims a run only grows, and can only drop,
    there (the docstring of tests/bocpd_cases.py).
A few cases carry overrides (`FORCED`) so that what the heuristic must show -- a late truncation from more than 256 live hypotheses to
fewer than 64, a change point under confirm = 0 and under drop = 0, three change points or more, more than max_changepoints allows --
does not hang on the seed either.

A case that the references do not admit (tests/test_bocpd_net_cases_cpu.py) is redrawn from the next sub-seed and listed in REPLACED."""

from functools import lru_cache

import numpy as np

import bocpd_cases as BC

SEED = 4107
BOUNDARY_DIMS = (12, 13, 17, 18, 24, 25)
KINDS = ("none", "shift", "alt", "var")
SCALES = (1e-3, 1.0, 1e3)

# case number -> sub-seed of the admitted draw (sub-seed 0 failed the admission of tests/test_bocpd_net_cases_cpu.py)
REPLACED = {}


def lanes(dim):
    """bocpd_lanes of rpsmf_amd/csrc/psmf_bocpd.hip: the most of 256, 128, 64, 32 lanes whose packed factors fit 160 KiB of LDS"""
    lane_bytes = dim * (dim + 1) // 2 * 8
    return next(n for n in (256, 128, 64, 32) if n * lane_bytes <= 160 * 1024 or n == 32)


def walk():
    """the (dim, T) of every case, in order"""
    out = []
    for dim in BOUNDARY_DIMS:
        nl = lanes(dim)
        out += [(dim, nl - 1), (dim, nl), (dim, nl + 1), (dim, 2 * nl + 1)]
    for dim in range(1, 33):                             # every other dim: past one block edge at least
        if dim not in BOUNDARY_DIMS:
            nl = lanes(dim)
            out.append((dim, 2 * nl + 1 if dim in (2, 7, 15, 21, 29) else nl + 1))
    out += [(5, 63), (8, 64), (11, 65), (3, 255), (6, 256), (9, 257)]
    for k, dim in enumerate(d for d in range(1, 33) if d not in BOUNDARY_DIMS):      # and once more, at or under one block
        nl = lanes(dim)
        out.append((dim, (nl - 1, nl, nl + 1)[k % 3]))
    out += [(4, 513), (10, 513), (1, 64), (14, 257), (20, 129), (28, 65), (32, 65), (16, 129)]
    return out


# overrides by case number: (dim, T) is walk()'s, the rest replaces what was drawn
FORCED = {
    3: dict(kind="shift", at=(350,), lam=300.0, drop=5, settle=8, confirm=3, max_changepoints=16),      # dim 12, T 513: > 256 live -> < 64
    82: dict(kind="shift", at=(400,), lam=200.0, drop=8, settle=6, confirm=5, max_changepoints=1),      # dim 4, T 513: the same, later
    83: dict(kind="alt", at=(90, 180, 270, 360, 450), lam=100.0, drop=6, settle=5, confirm=2, max_changepoints=1),      # dim 10, T 513: shifts this prior never takes for one -- 513 live
    84: dict(kind="shift", at=(30,), lam=50.0, drop=4, settle=4, confirm=0, max_changepoints=16),       # dim 1, T 64: confirm = 0
    85: dict(kind="alt", at=(60, 120, 190), lam=100.0, drop=0, settle=12, confirm=4, max_changepoints=0),      # dim 14, T 257: drop = 0
    86: dict(kind="alt", at=(30, 60, 95), lam=60.0, drop=3, settle=6, confirm=1, max_changepoints=1),   # dim 20, T 129
    87: dict(kind="shift", at=(40,), lam=80.0, drop=5, settle=0, confirm=2),                            # dim 28, T 65: settle = 0 never confirms
    88: dict(kind="shift", at=(44,), lam=80.0, drop=2, settle=3, confirm=12, max_changepoints=16),      # dim 32, T 65: the confirmation is slow
    89: dict(kind="var", at=(70,), lam=150.0, drop=7, settle=7, confirm=4),                             # dim 16, T 129
}


def draw(no, dim, T, sub=0):
    rng = np.random.default_rng([SEED, no, sub])
    lu = lambda lo, hi: float(np.exp(rng.uniform(np.log(lo), np.log(hi))))
    cs = dict(no=no, name=f"net{no:03d}-dim{dim}-T{T}", dim=dim, T=T, sub=sub, batch=int(rng.integers(1, 6)))
    cs.update(lam=lu(1.5, 1000.0), kappa0=lu(0.05, 20.0), nu0=dim - 1 + lu(0.05, 10.0))
    cs["scale"] = SCALES[int(rng.integers(3))]
    cs["sigma0"] = cs["scale"] ** 2 * lu(0.25, 4.0)
    cs["drop"], cs["settle"], cs["confirm"] = (int(v) for v in rng.integers(0, 13, 3))
    cs["max_changepoints"] = (0, 1, 16)[int(rng.integers(3))]
    cs["kind"] = KINDS[int(rng.integers(4))]
    cs["base"] = float(rng.choice([-1.0, 1.0]) * rng.uniform(1.5, 3.0))      # in units of the scale
    cs["vscale"] = float(rng.uniform(4.0, 8.0))
    places = int(rng.integers(2, 6)) if cs["kind"] == "alt" else 1
    span = np.arange(max(T // 6, 1), max(T - T // 6, 2))
    cs["at"] = tuple(int(v) for v in np.sort(rng.choice(span, size=min(places, len(span)), replace=False)))
    cs.update(FORCED.get(no, {}))
    if cs["kind"] == "none":
        cs["at"] = ()
    return cs


CASES = [draw(no, dim, T, REPLACED.get(no, 0)) for no, (dim, T) in enumerate(walk())]
IDS = [c["name"] for c in CASES]
PARAMS = ("lam", "kappa0", "nu0", "sigma0", "drop", "settle", "confirm")


def params(cs):
    """the model's arguments of a case (the device takes max_changepoints besides)"""
    return {k: cs[k] for k in PARAMS}


def series(cs, b):
    """X (dim, T) of replica b of a case"""
    rng = np.random.default_rng([SEED, cs["no"], cs["sub"], 1000 + b])
    Z = rng.standard_normal((cs["dim"], cs["T"]))
    mean = np.full(cs["T"], cs["base"])
    if cs["kind"] in ("shift", "alt"):
        for at in cs["at"]:
            mean[at:] = -mean[at:]                       # +base, -base, +base, ...
    elif cs["kind"] == "var":
        Z[:, cs["at"][0]:] *= cs["vscale"]
    return cs["scale"] * (Z + mean[None])


def batch(cs):
    return np.stack([series(cs, b) for b in range(cs["batch"])])


@lru_cache(maxsize=None)
def reference(no, b):
    """(X, extended_model's result) of replica b of case `no`, computed once per process"""
    cs = CASES[no]
    X = series(cs, b)
    X.setflags(write=False)
    return X, BC.extended_model(X, **params(cs))


@lru_cache(maxsize=None)
def stable_reference(no, b):
    cs = CASES[no]
    return BC.stable_model(series(cs, b), **params(cs))


def column_gap(R):
    return BC.column_gap(R)


def truncations(ref):
    """(step t 0-based, first live birth before, first live birth after) of every declared change point of a model's result: the
    discarded births are [before, after), and a declared cp IS the first birth that stays (cp = t - m_t + 2 = 0-based birth t - m_t + 2)"""
    out, lo = [], 0
    for t, cp in zip(ref["declared_at"], ref["changepoints"]):
        hi = max(lo, min(t + 1, cp))
        out.append((t, lo, hi))
        lo = hi
    return out
