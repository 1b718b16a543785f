"""The random-configuration net of the batched PSMF with linear-Gaussian dynamics and an observation map (psmf_ssm_run and
psmf_ssm_run_ex, rpsmf_amd/ssm.py; psmf_ssm_kernel<robust, masked>, rpsmf_amd/csrc/psmf_ssm.hip): the draw, the problem of every
case and its float64 references.  Pure numpy: tests/test_ssm_net_cases_cpu.py checks the net without a GPU,
tests/test_hip_ssm_net.py runs it on the device.

N_CASES cases from one seed; case i is a function of i alone (and of the sub-seed REPLACED records for it), so a failing case can
be rerun by number.  Case i targets kernel instance i % 4 (plain, robust, masked, robust+masked).  With j = i // 4 counting the
cases of one instance: even j takes r, p, d from the edge lists below (walked in turn), odd j draws them uniformly from the legal range; j // 2 even gives
every replica its own dense V0 and P0, (batch, r, r) and (batch, p, p), otherwise one dense V0 / P0 is broadcast; j % 5 picks the
mask shape of a masked case (MASK_KINDS).  Everything else is drawn:
    r       R_EDGES, else 1..16               p    {r, r + 1, 16, 17, 31, 32} kept >= r, else r..32
    d       D_EDGES, else 1..512              n    N_LIST, n <= 40 when d > 256 (the d x d reference stays cheap)
    batch   2 or 3 DIFFERENT replicas: own Y, contamination, C0, x0, mask (and V0, P0)
    carry_P {0, 1}   lambda0 LAMBDAS   fixed_lambda {False, True}   alpha ALPHAS   beta BETAS     (robust instances; else 1)
    rho     {1e-3, 0.05, 0.5, 3} for d <= 64, {0.05, 0.5, 3} above               observed fraction FRACTIONS (masked instances)
    A = 0.9 I + 0.05 N / sqrt(p) (not symmetric), Q = 0.05 I + 0.02 L L^T / p, H = W diag(sigma) U^T with U p x r orthonormal,
    W r x r orthogonal and sigma uniform in [0.5, 1.5]: the r x r algebra of the kernel forms P_z^-1 and its error grows with
    cond(P_z) ~ cond(H)^2 cond(Pbar) -- a plain Gaussian H at p = r = 15 / 16 makes two float64 models differ by 1e-9.
    V0 = 0.3 I + 0.4 L L^T / r, P0 = 0.5 I + 0.5 L L^T / p (dense, symmetric positive definite)
    Y, C0, x0 as ssm_cases.problem (min(4, r) sinusoids mixed by a normal matrix, the first scaled by 2.5 from n / 2 on, plus
    0.3 N(0, 1); C0 standard normal, x0 = 0.3 N(0, 1)) with the contamination of ssm_robust_cases.problem: a Student-t draw with
    3 degrees of freedom added to 5 % of the entries.
Masks (1 = observed; every column keeps an observed row):
    uniform     each entry observed with the case's fraction
    last-row    d >= 2: on about a third of the steps (at least one) only row d - 1 is observed -- with d > 256 it lies in the
                second row of its thread (u = 1 in phases 3 and 10 of the kernel)
    dark-wave   d >= 65: rows 64 k .. 64 k + 63 of one wave are unobserved for a run of steps
    full-steps  d >= 2, n >= 2: every second step is fully observed, the others are not (cnt == d switches the eta expression)
A structured mask whose condition on d or n fails is drawn uniform instead (cs["mask_kind"] says what was built).

The references are ssm_robust_cases.literal_model (d x d, line for line) and device_algebra_model (the kernel's r x r algebra),
one run per replica.  A case is in the net only if it passes `admission`: finite, V positive definite, the two models within
1e-11 on every compared array, and C0, x0 moved by 4 * 2^-52 move every compared array by at most 1e-11.  A draw that fails is
replaced by the next sub-seed of the same i: REPLACED holds the outcome, tests/test_ssm_net_cases_cpu.py recomputes it."""

from functools import lru_cache

import numpy as np

import netlib
import ssm_cases as SC
import ssm_robust_cases as RC

SEED = 9400
N_CASES = 240
INSTANCES = ("plain", "robust", "masked", "robust+masked")
R_EDGES = (1, 2, 3, 8, 15, 16)
D_EDGES = (1, 2, 3, 4, 5, 63, 64, 65, 127, 129, 255, 256, 257, 260, 383, 511, 512)
N_LIST = (1, 2, 3, 7, 25, 40, 60)
LAMBDAS = (0.7, 1.8, 10.0, 50.0)
ALPHAS = (1.0, 0.97, 1.02)
BETAS = (1.0, 0.95, 1.05)
RHOS = (1e-3, 0.05, 0.5, 3.0)
FRACTIONS = (0.1, 0.5, 0.9)
MASK_KINDS = ("uniform", "last-row", "uniform", "dark-wave", "full-steps")       # by j % 5
STRUCTURED = ("last-row", "dark-wave", "full-steps")
BAR = 5e-9            # the suite's float64 bar for the one-workgroup engines (tests/test_hip_ssm.py); not raised
ADMIT = 1e-11         # both admission bounds
EPS = 4 * 2.0 ** -52
relerr = SC.relerr


def p_edges(r):
    return (r, r + 1, 16, 17, 31, 32)


def case(i, sub=0):
    """the configuration of case i at sub-seed `sub`: a dict of plain Python values"""
    rng = np.random.default_rng([SEED, i, sub])
    inst, j = i % 4, i // 4
    robust, masked = bool(inst & 1), bool(inst & 2)
    edge, own = j % 2 == 0, (j // 2) % 2 == 0
    if edge:
        e = j // 2                                # the edge lists are walked, not drawn from: every value occurs, whatever the seed
        g = 4 * e + inst
        r = R_EDGES[(e + inst) % len(R_EDGES)]
        p = max(r, p_edges(r)[(e // len(R_EDGES) + g) % 6])
        d = D_EDGES[g % len(D_EDGES)]
    else:
        r = int(rng.integers(1, 17))
        p = int(rng.integers(r, 33))
        d = int(rng.integers(1, 513))
    n = int(rng.choice([v for v in N_LIST if d <= 256 or v <= 40]))
    batch = int(rng.integers(2, 4))
    carry_P = int(rng.integers(0, 2))
    lambda0, fixed = float(rng.choice(LAMBDAS)), bool(rng.integers(0, 2))
    alpha, beta = float(rng.choice(ALPHAS)), float(rng.choice(BETAS))
    rho = float(rng.choice(RHOS if d <= 64 else RHOS[1:]))
    frac = float(rng.choice(FRACTIONS))
    kind = MASK_KINDS[j % 5]
    if (kind == "last-row" and d < 2) or (kind == "dark-wave" and d < 65) or (kind == "full-steps" and (d < 2 or n < 2)):
        kind = "uniform"
    return dict(i=i, sub=sub, robust=robust, masked=masked, edge=edge, own_VP=own, d=d, n=n, r=r, p=p, batch=batch, carry_P=carry_P,
                lambda0=lambda0 if robust else None, fixed_lambda=fixed and robust, alpha=alpha if robust else 1.0,
                beta=beta if robust else 1.0, rho=rho, frac=frac if masked else 1.0, mask_kind=kind if masked else None)


def instance(cs):
    """the kernel instance a case runs on"""
    return INSTANCES[(1 if cs["robust"] else 0) + (2 if cs["masked"] else 0)]


def bar(cs):
    return BAR


def compared(cs):
    """what the device is compared on: the plain instance (psmf_ssm_run) returns no omega, phi, robust_state"""
    return RC.COMPARED if (cs["robust"] or cs["masked"]) else SC.COMPARED


def describe(cs):
    s = (f"{instance(cs)} d={cs['d']} r={cs['r']} p={cs['p']} n={cs['n']} batch={cs['batch']} carry_P={cs['carry_P']} rho={cs['rho']:g} "
         f"V0,P0={'per replica' if cs['own_VP'] else 'shared'} draw={'edges' if cs['edge'] else 'uniform'}")
    if cs["robust"]:
        s += f" lambda0={cs['lambda0']:g}{' fixed' if cs['fixed_lambda'] else ''} alpha={cs['alpha']:g} beta={cs['beta']:g}"
    if cs["masked"]:
        s += f" mask={cs['mask_kind']} observed={cs['frac']:g}"
    return s


def _spd(rng, k, base, spread):
    L = rng.standard_normal((k, k))
    M = base * np.eye(k) + spread * (L @ L.T) / k
    return 0.5 * (M + M.T)


def _mask(rng, cs):
    d, n, kind = cs["d"], cs["n"], cs["mask_kind"]
    if not cs["masked"]:
        return np.ones((d, n), dtype=np.uint8)
    m = rng.uniform(size=(d, n)) < cs["frac"]
    dark = np.zeros((d, n), dtype=bool)           # entries that must stay unobserved
    if kind == "last-row":
        steps = np.flatnonzero(rng.uniform(size=n) < 1.0 / 3.0)
        if len(steps) == 0:
            steps = np.array([min(1, n - 1)])
        m[:, steps] = False
        m[d - 1, steps] = True
        dark[:d - 1, steps] = True
    elif kind == "dark-wave":
        k = int(rng.integers(0, (d + 63) // 64))          # (d >= 65: there are rows outside any one wave)
        t0 = int(rng.integers(0, n))
        t1 = int(rng.integers(t0, n)) + 1
        m[64 * k:64 * k + 64, t0:t1] = False
        dark[64 * k:64 * k + 64, t0:t1] = True
    elif kind == "full-steps":
        par = int(rng.integers(0, 2))
        m[:, par::2] = True
        rest = np.arange(1 - par, n, 2)
        hole = rng.integers(0, d, size=len(rest))
        m[hole, rest] = False                      # a step that is not fully observed has a hole
        dark[hole, rest] = True
    for t in np.flatnonzero(m.sum(axis=0) == 0):   # every column keeps at least one row
        free = np.flatnonzero(~dark[:, t])
        m[free[int(rng.integers(0, len(free)))], t] = True
    return m.astype(np.uint8)


def problem(cs, perturb=None):
    """The replicas of a case: a list of dict(Y (d, n), C0 (d, r), x0 (p,), V (r, r), P0 (p, p), A, Q, H, rho, mask (d, n) uint8) --
    what ssm_robust_cases.literal_model takes; A, Q, H, rho are shared (the same arrays), V and P0 too unless cs["own_VP"].
    `perturb` = eps: C0 and x0 times (1 + eps u), u uniform in [-1, 1]."""
    i, sub, d, n, r, p = cs["i"], cs["sub"], cs["d"], cs["n"], cs["r"], cs["p"]
    mrng = np.random.default_rng([SEED, i, sub, 0])
    A = 0.9 * np.eye(p) + 0.05 * mrng.standard_normal((p, p)) / np.sqrt(p)
    Q = _spd(mrng, p, 0.05, 0.02)
    U, _ = np.linalg.qr(mrng.standard_normal((p, r)))
    W, _ = np.linalg.qr(mrng.standard_normal((r, r)))
    H = (W * mrng.uniform(0.5, 1.5, size=r)) @ U.T
    V, P0 = _spd(mrng, r, 0.3, 0.4), _spd(mrng, p, 0.5, 0.5)
    k = min(4, r)
    t = np.arange(n, dtype=float)
    S = np.stack([np.sin(0.07 * (j + 1) * t + j) for j in range(k)])
    S[0, n // 2:] *= 2.5
    pbs = []
    for b in range(cs["batch"]):
        rng = np.random.default_rng([SEED, i, sub, 1 + b])
        Y = rng.standard_normal((d, k)) @ S + 0.3 * rng.standard_normal((d, n))
        hit = rng.uniform(size=(d, n)) < 0.05
        Y = Y + np.where(hit, rng.standard_t(3, size=(d, n)), 0.0)
        C0, x0 = rng.standard_normal((d, r)), 0.3 * rng.standard_normal(p)
        Vb, Pb = (_spd(rng, r, 0.3, 0.4), _spd(rng, p, 0.5, 0.5)) if cs["own_VP"] else (V, P0)
        mask = _mask(rng, cs)
        if perturb is not None:
            C0, x0 = netlib.perturbed(dict(C0=C0, x0=x0), [SEED, i, sub, 100 + b], perturb).values()
        pbs.append(dict(Y=Y, C0=C0, x0=x0, V=Vb, P0=Pb, A=A, Q=Q, H=H, rho=cs["rho"], mask=mask))
    return pbs


def model_kw(cs):
    """the keywords of ssm_robust_cases.literal_model / device_algebra_model for a case"""
    return dict(robust=cs["robust"], lambda0=cs["lambda0"], fixed_lambda=cs["fixed_lambda"], alpha=cs["alpha"], beta=cs["beta"])


def device_kw(cs, pbs):
    """the keywords of rpsmf_amd.ssm.linear_psmf_batch for a case (none of the new ones on the plain instance: psmf_ssm_run)"""
    kw = dict(carry_P=bool(cs["carry_P"]))
    if cs["robust"]:
        kw.update(robust=True, lambda0=cs["lambda0"], fixed_lambda=cs["fixed_lambda"], alpha=cs["alpha"], beta=cs["beta"])
    if cs["masked"]:
        kw["mask"] = np.stack([q["mask"] for q in pbs])
    return kw


def device_args(cs, pbs):
    """the positional arguments of linear_psmf_batch: Y, C0, x0, V0, P0, A, Q, H, rho"""
    st = lambda k: np.stack([q[k] for q in pbs])
    V0, P0 = (st("V"), st("P0")) if cs["own_VP"] else (pbs[0]["V"], pbs[0]["P0"])
    return st("Y"), st("C0"), st("x0"), V0, P0, pbs[0]["A"], pbs[0]["Q"], pbs[0]["H"], cs["rho"]


def admission(cs):
    """(admitted, figures): every replica finite with V positive definite in the line-for-line model, the kernel's algebra within
    ADMIT of it, and its response to EPS on C0 and x0 within ADMIT, on every array of ssm_robust_cases.COMPARED"""
    pbs, pert = problem(cs), problem(cs, perturb=EPS)
    kw = model_kw(cs)
    algebra = cond = 0.0
    try:
        for pb, pp in zip(pbs, pert):
            ref = RC.literal_model(pb, cs["carry_P"], **kw)
            if not all(np.all(np.isfinite(v)) for v in ref.values()):
                return False, dict(why="not finite")
            if not np.linalg.eigvalsh(0.5 * (ref["V"] + ref["V"].T)).min() > 0:
                return False, dict(why="V not positive definite")
            alg = RC.device_algebra_model(pb, cs["carry_P"], **kw)
            moved = RC.literal_model(pp, cs["carry_P"], **kw)
            algebra = max([algebra] + [relerr(alg[k], ref[k]) for k in RC.COMPARED])
            cond = max([cond] + [relerr(moved[k], ref[k]) for k in RC.COMPARED])
    except np.linalg.LinAlgError as e:
        return False, dict(why=f"LinAlgError: {e}")
    ok = bool(algebra <= ADMIT and cond <= ADMIT)          # (a NaN in either fails)
    return ok, dict(algebra=algebra, cond=cond)


def resolve(i):
    """(sub-seed of the first admitted draw of case i, log of the draws it replaced): netlib.resolve without halving, the salt
    being the sub-seed"""
    def admissible(cs):
        ok, figures = admission(cs)
        return ok, str(figures)

    (sub, _), log = netlib.resolve(i, case, None, admissible, describe)
    return sub, log


# What `resolve` answers for the cases whose first draw it does not admit, {i: sub-seed}: recorded so that the device test need not
# run three models per replica; tests/test_ssm_net_cases_cpu.py recomputes every entry and every absence.
REPLACED = {47: 1, 177: 1, 230: 1}
N_REPLACED = sum(REPLACED.values())       # draws replaced at admission


def device_case(i):
    """case i as the net runs it"""
    return netlib.device_case(i, case, None, (REPLACED.get(i, 0), 0))


@lru_cache(maxsize=None)
def reference(i):
    """(case, replicas, literal_model result per replica) of case i, computed once and shared: do not modify any of it"""
    cs = device_case(i)
    pbs = problem(cs)
    return cs, pbs, [RC.literal_model(pb, cs["carry_P"], **model_kw(cs)) for pb in pbs]
