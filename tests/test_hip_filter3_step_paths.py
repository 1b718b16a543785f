"""The paths through the step loop of psmf_blk_filter3 (rpsmf_amd/csrc/psmf_blk3.hip) that are NOT the steady one, and the steady
one itself.  psmf_blk_filter3's step loop is laid out for the path a converged step takes: phase 0 of the inversion waves fills W
from the dump and forms its trace in a straight line, with the refill from the sweep image in a block of its own
(F3_W_AND_TRACES_WIDE); the tracked-Gram update runs as independent chains with the contraction written out; the vector waves read
mu_bar as one group.  None of it changes an operation, so every comparison here is bit for bit -- and it can only go wrong where a
step leaves the steady path, so each case asserts from counters() that it drove the path it is named for:

    refill  the first steps from the initial state with rho_0 = 1, q = 0.1 (the random net's problem): the first step of pass 0 has
            nothing to start from and sweeps, and so do later ones; the step behind a sweep refills W from the sweep image
    one     rho_0 = 1e6, q <= 1e-3, float32 storage: accepted at the first check, one iteration per timestep -- the steady path
    two     the first check fails and the second iteration is the last one: it runs on the matrix M of phase 1, and the partner's
            final column is fetched late, in the next step's phase 0 (fetch_late) -- two per timestep
    more    a tolerance so tight that the third barrier and the loop behind it run: three or more per timestep

(settings: tests/decision_path_cases.py, where they were chosen from probes on an MI355X).  Shapes: d = 257 (d = 3 once); r = 32
(mask mode 0), 20 and 17 (mask mode 1; at r = 17 the second tile holds ONE row and column); T = 2 B + 1 and 3 B + 1 with
B = min(64 - r, 48); PSMF and rPSMF; float32 and float64 storage; chained and one launch per block.  Each case is compared with

  * the record of the PARENT commit's library, tests/golden/filter3_step_paths_parent.npz: per pass the integer counters and a
    blake2b digest of the bytes of every array (state, all of y_pred, the mean history; equal digests are np.array_equal and
    more: the sign of a zero counts).  Written on an MI355X by tests/golden/make_golden_step_paths.py on the parent's build;
  * the float64 oracle at the bars of the decision-path tests (blocked_cases.bar: float64 storage 1e-9, float32 storage 1e-5).

GPU only: `pytest -m gpu`; `-s` shows the counters and error figures of every case (each prints before it asserts)."""

import hashlib
import os

import numpy as np
import pytest

import blocked_cases as BC
import decision_path_cases as DP
import netlib

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

STATE_KEYS = ("C", "V", "P", "Q", "mu", "rho", "lam", "s", "eta", "N", "phi", "omega", "k")
COUNTER_KEYS = ("ns_steps", "sweep_steps", "ns_iterations", "ns_failed", "filter_launches", "filter_kernel_launches")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "filter3_step_paths_parent.npz")
KERNEL = "psmf_blk_filter3"
RANKS = (32, 20, 17)

# (robust, storage, path, blocks, chained): T = blocks * B + 1.  Every rank runs every row; between them the rows cover both
# lengths, both forms, both storages and both launch forms for every path that has them (`one` exists with float32 storage only).
ROWS = (
    (False, "f32", "one", 3, True),
    (True, "f32", "one", 2, True),
    (False, "f64", "two", 2, True),
    (True, "f64", "two", 3, True),
    (False, "f32", "two", 3, False),
    (False, "f64", "more", 2, True),
    (True, "f64", "more", 3, False),
    (False, "f64", "refill", 2, True),
    (True, "f32", "refill", 3, True),
)


def make(r, robust, storage, path, blocks, chain, d=DP.D_ROWS):
    """a case of tests/decision_path_cases.py (same fields, same problem generator, same settings per path) at this file's ranks
    and lengths; `refill` is the random net's problem at the default tolerances, looked at on the first pass"""
    B = BC.block_steps(r)
    T = blocks * B + 1
    pbkw, env, on_pass = ({}, {}, 0) if path == "refill" else DP.SETTINGS[(robust, storage, path)]
    env = dict(env)
    if not chain:
        env["PSMF_BLOCK_CHAIN"] = "0"           # one launch per block
    name = f"r{r}-{'rPSMF' if robust else 'PSMF'}-{storage}-{path}-{blocks}B" + ("-d3" if d == 3 else "") + ("" if chain else "-perblock")
    cs = dict(name=name, path=path, r=r, B=B, d=d, T=T, blocks=blocks, dyn="random_walk", robust=robust, storage=storage,
              v0=0.02 if storage == "f32" else 0.1, fixed_lambda=False, alpha=1.0, beta=1.0, general_Q=False, sched=False,
              hooks="full", recursive=0, update_every=1, env=env, second_pass=True, shards=None, parts=[(0, T)],
              # the series depends on (r, robust, storage, d, T) alone; the paths of one problem share its oracle run
              seed=880000 + 1000 * r + 100 * int(robust) + 10 * (storage == "f32") + (d != DP.D_ROWS) + 7 * blocks,
              i=name, salt=0, shortened=0, rho=float(pbkw.get("rho", 1.0)), q=float(pbkw.get("q", 0.1)), on_pass=on_pass)
    assert BC.expected_kernel(cs) == KERNEL, cs
    return cs


def cases():
    out = [make(r, *row) for r in RANKS for row in ROWS]
    out.append(make(32, False, "f64", "refill", 2, True, d=3))
    return out


CASES = cases()


def expect(cs, passes):
    """None, or what is wrong with the counters (one dict per pass) for the path of the case.  decision_path_cases.expect with the
    number of blocks of the case in place of its three: a block's first step starts without the predictor and may take up to two
    iterations more than a steady one, or, on the two-iteration path, one fewer."""
    T, nblk = cs["T"], cs["blocks"] + 1
    for ep, cnt in enumerate(passes):
        if cnt["ns_steps"] + cnt["sweep_steps"] != T:
            return f"pass {ep}: ns_steps + sweep_steps != T: {cnt}"
    cnt = passes[cs["on_pass"]]
    ns, sw, it, fl = cnt["ns_steps"], cnt["sweep_steps"], cnt["ns_iterations"], cnt["ns_failed"]
    first = 1 if cs["on_pass"] == 0 else 0          # the first step of the first pass sweeps: nothing to start from
    path = cs["path"]
    if path == "refill":
        # a sweep, and a step behind it that iterates (its phase 0 refilled W from the image)
        return None if sw >= 1 and ns >= 1 else f"refill: {cnt}"
    if path == "more":
        return None if it >= 3 * ns and 10 * fl <= T else f"more: {it / max(ns, 1):.3f} iterations per iterated timestep, {cnt}"
    if sw != first or fl:
        return f"{path}: sweeps or failed starts in pass {cs['on_pass']}: {cnt}"
    if path == "one":
        return None if ns <= it <= ns + 2 * nblk else f"one: {it} iterations in {ns} timesteps"
    return None if 2 * ns - nblk <= it <= 2 * ns + 2 * nblk else f"two: {it} iterations in {ns} timesteps"


def digest(a):
    a = np.ascontiguousarray(np.asarray(a))
    return np.frombuffer(hashlib.blake2b(a.tobytes(), digest_size=16).digest(), dtype=np.uint8).copy()


def drive(c, cs, pb):
    """The two passes of a case on one handle -> per pass: state, y_pred, mean history, integer counters"""
    r, d, T = cs["r"], cs["d"], cs["T"]
    with netlib.env(cs["env"]):
        f = c.DeviceFilter(d, r, robust=cs["robust"], storage=cs["storage"], engine="block")
    try:
        f.upload_series(np.ascontiguousarray(pb["Y"]))
        f.set_state(pb["C0"], pb["V0"], pb["P0"], pb["Q"], pb["mu0"], rho=pb["rho"], lambda0=pb["lam"])
        geo = f.geometry()
        assert geo["filter_kernel"] == KERNEL and geo["block_steps"] == cs["B"], geo
        out = []
        for ep in range(2):
            if ep and cs["robust"]:              # rPSMF's step_reset (rpsmf.py:106-114)
                f.set_state(Q=pb["Q"], rho=pb["rho"], lambda0=pb["lam"])
            f.counters(reset=True)
            f.run(0, T)
            cnt = f.counters()
            out.append(dict(state=f.get_state(), y_pred=f.y_pred(0, T), mu_hist=f.mu_history(1, T), counters={k: int(cnt[k]) for k in COUNTER_KEYS}))
        return out
    finally:
        f.close()


def record_of(passes):
    """what the golden file keeps of a case: {key: array}"""
    rec = {}
    for ep, p in enumerate(passes):
        rec[f"pass{ep}/counters"] = np.array([p["counters"][k] for k in COUNTER_KEYS], dtype=np.int64)
        for k in STATE_KEYS:
            rec[f"pass{ep}/{k}"] = digest(np.asarray(p["state"][k], dtype=np.float64))
        rec[f"pass{ep}/y_pred"] = digest(p["y_pred"])
        rec[f"pass{ep}/mu_hist"] = digest(p["mu_hist"])
    return rec


def problem_key(cs):
    return (cs["r"], cs["robust"], cs["storage"], cs["d"], cs["T"], cs["rho"], cs["q"])


_REF = {}


def reference(cs):
    """problem and oracle of a case, computed once per problem: the cases of one problem share both (read-only)"""
    key = problem_key(cs)
    if key not in _REF:
        pb = DP.problem(cs)
        ref, _ = BC.reference(cs, pb)
        _REF[key] = (pb, ref)
    return _REF[key]


def errors(cs, passes, ref):
    """[(quantity, pass, relative error against the oracle, bar)]"""
    tol, errs = BC.bar(cs), []
    for ep, (p, want) in enumerate(zip(passes, ref)):
        s = p["state"]
        for k in ("C", "V", "mu", "P"):
            errs.append((k, ep, BC.relerr(s[k], want[k]), tol))
        errs.append(("y_pred", ep, BC.relerr(p["y_pred"], want["y_pred"]), tol))
        if cs["robust"]:
            errs += [("rho", ep, BC.relerr(s["rho"], want["rho"]), tol), ("lam", ep, BC.relerr(s["lam"], want["lam"]), tol)]
        else:
            errs += [("eta", ep, BC.relerr(s["eta"], want["eta"]), tol), ("N", ep, BC.relerr(s["N"], want["N"]), tol)]
    return errs


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("cs", CASES, ids=[cs["name"] for cs in CASES])
def test_step_path(cs, golden):
    from rpsmf_amd import _capi as c

    pb, ref = reference(cs)
    passes = drive(c, cs, pb)
    T = cs["T"]
    for ep, p in enumerate(passes):
        n = p["counters"]
        print(f"\nSTEP-PATH case={cs['name']} pass={ep} per timestep: iterations {n['ns_iterations'] / T:.3f} sweeps {n['sweep_steps'] / T:.3f} "
              f"failed {n['ns_failed'] / T:.3f} | {n}")
    # the path, from the counters
    wrong = expect(cs, [p["counters"] for p in passes])
    assert wrong is None, (cs["name"], wrong)
    nblk = cs["blocks"] + 1
    for p in passes:
        assert p["counters"]["filter_launches"] == nblk
        assert p["counters"]["filter_kernel_launches"] == (nblk if cs["env"].get("PSMF_BLOCK_CHAIN") == "0" else 1), p["counters"]
        for k in STATE_KEYS:
            assert np.all(np.isfinite(np.asarray(p["state"][k], dtype=float))), (cs["name"], k)
    # the float64 oracle
    errs = errors(cs, passes, ref)
    worst = max(errs, key=lambda e: (e[2] / e[3]) if np.isfinite(e[2]) else np.inf)
    print(f"STEP-PATH case={cs['name']} bar={worst[3]:.0e} worst={worst[0]}@{worst[1]} err={worst[2]:.3e} ratio={worst[2] / worst[3]:.3g}")
    bad = [e for e in errs if not e[2] < e[3]]
    assert not bad, (cs["name"], bad)
    # the parent's record: same bits, same counters
    for k, v in record_of(passes).items():
        want = golden[f"{cs['name']}/{k}"]
        assert np.array_equal(v, want), (cs["name"], k, v, want)
