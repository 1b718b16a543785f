"""Every exit of the inversion decision of psmf_blk_filter3 / filter3s (F3_DECIDE, rpsmf_amd/csrc/psmf_blk3.hip), forced with the
diagnostic switches of DESIGN section 9 at d = 257 (and d = 3), r = 32 / 20 / 12, PSMF and rPSMF, T = 2 B + 1, chained and one
launch per block, float64 and float32 storage: the list of tests/decision_path_cases.py.  The step loop reads the decision's norms
and thresholds in one group with its other LDS operands and runs the Gram / rank-1 update IN FRONT of the decision; that can only
go wrong where the decision is not the steady one, so each case asserts from counters() that it took the path it is named for
(iterations, sweeps and failed starts of a pass against its timesteps: decision_path_cases.expect), and then compares

  * with the float64 oracle, at the bars of the random net of the blocked engine (blocked_cases.bar: float64 storage 1e-9,
    float32 storage 1e-5; tests/test_decision_path_cases_cpu.py has shown the oracle's own response to a last-bit change of the
    inputs to sit 16 x inside them for every case);
  * bit for bit with what the library of the commit BEFORE the reordering left for the same case: tests/golden/
    filter3_decision_paths.npz holds, per case, the integer counters of both passes and a blake2b digest of the bytes of every
    array (state after each pass, all of y_pred, the mean history) -- equal digests are np.array_equal and more (the sign of a
    zero counts).  Recorded on an MI355X with tests/golden/make_golden_decision_paths.py on that commit's build; the record binds
    the cases to the compiler that built both libraries.

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
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "filter3_decision_paths.npz")
CASES = DP.cases()


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
        assert geo["filter_kernel"] == DP.SHAPES[r] and geo["block_steps"] == cs["B"], geo
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


_REF = {}


def _reference(cs):
    """problem and oracle of a case, computed once per problem: the paths of one problem share both (read-only)"""
    key = DP.problem_key(cs)
    if key not in _REF:
        pb = DP.problem(cs)
        ref, _ = BC.reference(cs, pb)
        _REF[key] = (pb, ref)
    return _REF[key]


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("cs", CASES, ids=[cs["name"] for cs in CASES])
def test_decision_path(cs, golden):
    from rpsmf_amd import _capi as c

    pb, ref = _reference(cs)
    passes = drive(c, cs, pb)
    T, tol = cs["T"], BC.bar(cs)
    for ep, p in enumerate(passes):
        n = p["counters"]
        print(f"\nPATH case={cs['name']} pass={ep} per timestep: iterations {n['ns_iterations'] / T:.3f} sweeps {n['sweep_steps'] / T:.3f} "
              f"failed {n['ns_failed'] / T:.3f} | {n}")
    # the path, from the counters
    wrong = DP.expect(cs, [p["counters"] for p in passes])
    assert wrong is None, (cs["name"], wrong)
    nblk = -(-T // cs["B"])
    for p in passes:
        assert p["counters"]["filter_launches"] == nblk
        assert p["counters"]["filter_kernel_launches"] == (nblk if cs["env"].get("PSMF_BLOCK_CHAIN") == "0" else 1), p["counters"]
    # the float64 oracle
    errs = []
    for ep, (p, want) in enumerate(zip(passes, ref)):
        s = p["state"]
        for k in ("C", "V", "mu", "P"):
            errs.append((k, ep, BC.relerr(s[k], want[k]), tol))
        errs.append(("y_pred", ep, BC.relerr(p["y_pred"], want["y_pred"]), tol))
        if cs["robust"]:
            errs += [("rho", ep, BC.relerr(s["rho"], want["rho"]), tol), ("lam", ep, BC.relerr(s["lam"], want["lam"]), tol)]
        else:
            errs += [("eta", ep, BC.relerr(s["eta"], want["eta"]), tol), ("N", ep, BC.relerr(s["N"], want["N"]), tol)]
        for k in STATE_KEYS:
            assert np.all(np.isfinite(np.asarray(s[k], dtype=float))), (cs["name"], k)
    worst = max(errs, key=lambda e: (e[2] / e[3]) if np.isfinite(e[2]) else np.inf)
    print(f"PATH case={cs['name']} bar={tol:.0e} worst={worst[0]}@{worst[1]} err={worst[2]:.3e} ratio={worst[2] / worst[3]:.3g}")
    bad = [e for e in errs if not e[2] < e[3]]
    assert not bad, (cs["name"], bad)
    # the record of the commit before the reordering: same bits, same counters
    got = record_of(passes)
    for k, v in got.items():
        want = golden[f"{cs['name']}/{k}"]
        assert np.array_equal(v, want), (cs["name"], k, v, want)
