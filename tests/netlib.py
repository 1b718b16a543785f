"""What the random-configuration nets and the device tests share: the admission policy of the case modules (blocked_cases,
step_cases, impute_cases, gram_cases, ssm_net_cases) and the helpers of the test_hip_*.py files that drive a handle.  A plain
module: no fixtures, and nothing of rpsmf_amd is imported until a function that needs the library is called -- the case modules
are imported on machines without it.

Admission: a case is taken if the oracle's own response to a last-bit change of the inputs sits 16 x inside the bar (what that
means is the case module's `admissible`); otherwise the horizon is halved, at most twice (the module's `shorten`); otherwise the
next salt, at most 8.  The outcome is recorded in a table of the case module, which its CPU test recomputes with `resolve`."""

import os
import threading
from contextlib import contextmanager

import numpy as np


# ---- admission
def resolve(i, case, shorten, admissible, describe, salts=8):
    """Case i as the device runs it.  case(i, salt) draws, shorten(cs) halves (None: it cannot; shorten=None: the net does not
    halve), admissible(cs) -> (ok, text).  Returns ((salt, times shortened), log of the draws that were not admitted)."""
    log = []
    for salt in range(salts):
        cs, halved = case(i, salt), 0
        while cs is not None:
            ok, text = admissible(cs)
            if ok:
                return (salt, halved), log
            log.append(f"case {i} salt {salt} {describe(cs)}: {text}")
            cs, halved = (shorten(cs), halved + 1) if shorten else (None, halved)
    raise AssertionError(f"case {i}: no admissible configuration in {salts} salts: {log}")


def device_case(i, case, shorten, resolution):
    """the case that `resolution` = (salt, times shortened) names"""
    salt, n = resolution
    cs = case(i, salt)
    for _ in range(n):
        cs = shorten(cs)
    return cs


def perturbed(arrays, seed, eps, f32=()):
    """{name: a (1 + eps u)}, u uniform in [-1, 1], drawn in the order of `arrays` from one generator; the arrays named in `f32`
    are rounded through float32 afterwards"""
    prng = np.random.default_rng(seed)
    out = {k: a * (1.0 + eps * prng.uniform(-1, 1, a.shape)) for k, a in arrays.items()}
    return {k: f32_round(a) if k in f32 else a for k, a in out.items()}


def require_finite(record, keys, what):
    for k in keys:
        if record.get(k) is not None and not np.all(np.isfinite(record[k])):
            raise FloatingPointError(f"{what}: non-finite {k} in the oracle")


def relerr(a, b):
    """conftest.relerr, max |a - b| / max |b|; 0.0 for an empty array"""
    a = np.asarray(a, dtype=float)
    b = np.asarray(b, dtype=float)
    if a.size == 0:
        return 0.0
    den = max(float(np.max(np.abs(b))), 1e-300)
    return float(np.max(np.abs(a - b))) / den


def response(ref0, ref1, keys):
    """the worst relerr(ref1[k], ref0[k]) over `keys` -- and over the parts, where the records are lists; 0.0 over nothing"""
    if isinstance(ref0, dict):
        ref0, ref1 = [ref0], [ref1]
    return max([relerr(p1[k], p0[k]) for p0, p1 in zip(ref0, ref1) for k in keys] + [0.0])


# ---- problems
def f32_round(a):
    return a.astype(np.float32).astype(np.float64)


def spd(rng, r, base):
    B = rng.standard_normal((r, r))
    return base * (np.eye(r) + 0.3 * (B @ B.T) / r)


def ydict(Y):
    """the {k: column} series the filter classes take"""
    return {k + 1: Y[k][:, None].copy() for k in range(Y.shape[0])}


# ---- device tests
def capi():
    from rpsmf_amd import _capi

    return _capi


@contextmanager
def env(vars_):
    """The environment for the creation of one handle or for one batched call, restored afterwards."""
    old = {k: os.environ.get(k) for k in vars_}
    os.environ.update(vars_)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def open_filter(c, cs, pb, engine, **extra):
    """The DeviceFilter of an unmasked case of the block or the step net: hooks, dynamics, storage, the in-loop optimiser."""
    from blocked_cases import ADAM_LR, HOOKS, SGD_LR

    nl = pb["nl"]
    cu, ef, pp = HOOKS[cs["hooks"]]
    return c.DeviceFilter(cs["d"], cs["r"], robust=cs["robust"], coef_update=cu, eta_full=ef, pbar_predict=pp, fixed_lambda=cs["fixed_lambda"],
                          alpha=cs["alpha"], beta=cs["beta"], dyn_kind=nl.device_kind, dyn_flags=nl.device_flags, dyn_terms=nl.device_terms,
                          storage=cs["storage"], recursive=cs["recursive"], update_every=cs["update_every"],
                          adam_lr=SGD_LR if cs["recursive"] == 2 else ADAM_LR, engine=engine, **extra)


def start_pass(f, cs, pb, ep):
    """the top of pass `ep`: rPSMF's step_reset (rpsmf.py:106-114) from the second pass on, the gradient sum, Adam's moments"""
    n_theta = pb["nl"].n_params
    if ep and cs["robust"]:
        f.set_state(Q=pb["Q"], rho=pb["rho"], lambda0=pb["lam"])
    if n_theta:
        f.zero_gradsum()
    if cs["recursive"] == 1:
        f.set_adam(np.zeros(n_theta), np.zeros(n_theta))


def state_errors(cs, got, want, part, tol, gtol, y_pred=None, skip=()):
    """[(quantity, part, error, bound)] of get_state() `got` against the oracle's record `want` of a run part: C, V, mu, P;
    `y_pred` where the part is not empty; rho, lam, Q of rPSMF; theta and the gradient sum where the dynamics have parameters."""
    errs = [(k, part, relerr(got[k], want[k]), tol) for k in ("C", "V", "mu", "P")]
    if want["b"] > want["a"]:
        errs.append(("y_pred", part, relerr(y_pred, want["y_pred"]), tol))
    if cs["robust"]:
        errs += [(k, part, relerr(got[k], want[k]), tol) for k in ("rho", "lam", "Q") if k not in skip]
    if want["theta"].size:
        errs.append(("theta", part, relerr(got["theta"], want["theta"]), tol))          # after a recursive run: the stepped theta
        if np.max(np.abs(want["gradsum"])) > 0:
            errs.append(("gradsum", part, relerr(got["gradsum"], want["gradsum"]), gtol))
        else:                                # (the optimiser has just stepped and restarted the sum)
            errs.append(("gradsum", part, float(np.max(np.abs(got["gradsum"]))), 1e-300))
    return errs


def verdict(errs):
    """the worst (quantity, part, error, bound) by error / bound; an error that is not finite is the worst there is"""
    return max(errs, key=lambda e: (e[2] / e[3]) if np.isfinite(e[2]) else np.inf)


def assert_within(errs, cs):
    bad = [e for e in errs if not e[2] < e[3]]          # (`not <`: a NaN fails)
    assert not bad, (cs, bad)


def run_ranks(n, worker, join_timeout):
    """worker(rank, comm) on n threads over one HostGroup, comm = the arguments of comm_init_host.  Returns (group, results)."""
    from host_group import HostGroup

    grp = HostGroup(n)
    out, errs = [None] * n, []

    def run(rank):
        try:
            out[rank] = worker(rank, (n, rank, grp.allreduce(rank)))
        except BaseException as e:          # noqa: BLE001 -- reported by the main thread
            errs.append((rank, e))
            grp.barrier.abort()

    threads = [threading.Thread(target=run, args=(k,)) for k in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(join_timeout)
    assert not any(t.is_alive() for t in threads), "a shard thread is stuck"
    assert not errs, errs
    assert all(k == grp.calls[0] for k in grp.calls), grp.calls
    return grp, out
