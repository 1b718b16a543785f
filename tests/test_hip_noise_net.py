"""The unmasked handle with a non-scalar observation noise R on seeded configurations (tests/noise_cases.py): 36 cases with a
per-row diagonal R = rho diag(rho_rows) (nonuniform_R + psmf_set_row_noise) against oracle.lowrank_step with a vector rho, and 24
with a dense symmetric PSD R (psmf_set_noise_rotation: the row path in the eigenbasis of R, psmf_rot_gemm at the boundary) against
oracle.literal_step with the d x d matrix -- the dense inverse the device never forms.  Rows from 2 to 700 around the GEMM's K slab,
its 64-tile and the Gram's 256 workgroups, every rank at which the weighted Gram or the solve changes instance, float32 / float64
storage crossed with the dtype of the upload, PSMF / rPSMF (fixed lambda, alpha / beta), R benign, spread over 1e6, with zero rows,
all equal but one -- dense: well conditioned, low rank plus diagonal, singular, block diagonal, a repeated eigenvalue -- the five
hook configurations, cos-phase and a dense-Jacobian kind, the in-loop Adam / SGD, rho_k / q_k schedules in front of R, a general Q,
one to three run parts, an empty run, a second pass, PSMF_WGRAM_MFMA 0 / 1; six row cases again as 2 and 3 row shards.

Every case asserts the dispatch (the per-step engine in its launched form, because of nonuniform_R) and state and y_hat against
the oracle after every run part.  A dense case also asserts the boundary of the rotation: an upload in pieces equals the whole
upload bit for bit, sub-range downloads are slices of the full one in both dtypes, get_state twice gives the same bits,
project(I_r) is C, and predict / predict_sq_error / sq_error match the oracle's roll-out and residual sums in original coordinates.
GPU only: `pytest -m gpu`; `-s` shows the error figures of every case (each prints before it asserts).

Bars: row cases step_cases.bar (float64 storage 1e-9, float32 1e-5), gradsum 1e-7 / 1e-5; dense cases the bars of
tests/test_hip_dense_R.py (1e-8, 1e-5).  tests/test_noise_cases_cpu.py has shown that the oracle's own response to a last-bit
change of the inputs sits 16 x inside them for every case.  The sums of squares take the bound that an elementwise error of
`bar` x max |y_hat| allows: 2 bar max|a| sum |a - y| (+ the second-order term).  Shards against the unsharded run: the bars of
tests/test_hip_multishard.py (1e-11, float32 storage 2e-6), replicated state bit-identical.
Measured on one MI355X: the whole file takes 2.0 s, its slowest case 0.32 s (profiles/noise_net_gpu_tests.txt); the limit below is per case.
Reference: pypsmf/psmf/psmf.py:85-188,287-304, rpsmf.py:116-184."""

import time

import numpy as np
import pytest

import netlib
import noise_cases as NC
import step_cases as SC
from conftest import relerr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(60)]


def _series(cs, Y):
    return Y.astype(np.float32) if cs["upload"] == "f32" else Y


def _open(c, cs, pb, rot=None, shard=None, comm=None, pieces=False):
    """A handle of the case with its noise, series and state.  shard = (row0, d_local); pieces: the series in two uploads split
    at a row count that is no multiple of the rotation's 64-row tile, and the first piece once more."""
    row0, dl = shard or (0, cs["d"])
    rows = slice(row0, row0 + dl)
    nl, T = pb["nl"], cs["T"]
    f = netlib.open_filter(c, cs, pb, "step", nonuniform_R=True, **(dict(row0=row0, d_local=dl) if shard else {}))
    try:
        if comm is not None:
            f.comm_init_host(*comm)
        if rot is not None:
            f.set_noise_rotation(rot[1], rot[0])
        else:
            f.set_row_noise(pb["rho_rows"][rows], rho_mean=float(pb["rho_rows"].sum()) / cs["d"])          # rho_mean: over ALL rows
        Y = _series(cs, np.ascontiguousarray(pb["Y"][:, rows]))
        if pieces:
            s = max(1, T // 3)
            f.upload_series(Y[:s], 0, T)
            f.upload_series(Y[s:], s, T)
            f.upload_series(Y[:s], 0, T)
        else:
            f.upload_series(Y)
        f.set_state(pb["C0"][rows], pb["V0"], pb["P0"], pb["Q"], pb["mu0"], rho=pb["rho"], lambda0=pb["lam"], theta=pb["theta"] if nl.n_params else None)
        if cs["sched"]:
            f.set_schedules(pb["rho_k"], pb["q_k"])
    except BaseException:
        f.close()
        raise
    return f


def _check_dispatch(f, cs):
    """the per-step engine, two launches per timestep, and nonuniform_R is why"""
    sp, g = f.step_plan(), f.geometry()
    assert g["engine"] == "step" and g["filter_kernel"] == "psmf_sweep_solve" == SC.expected_kernel(cs, sp["n_cu"]), (cs, g, sp)
    assert not sp["usable"] and not SC.facts(cs, sp["n_cu"])["uniform_R"], (cs, sp)
    if cs["r"] <= 48:          # (beyond 48 the rank alone keeps the launched form: the table names it first)
        assert SC.launched_reason(cs, sp["n_cu"]) == "nonuniform_R", (cs, SC.launched_reason(cs, sp["n_cu"]))
    return g["filter_kernel"], sp


def _run_all(f, cs, pb):
    """every pass and part without a look in between"""
    for ep in range(NC.passes_of(cs)):
        netlib.start_pass(f, cs, pb, ep)
        for a, b in cs["parts"]:
            f.run(a, b)
    return f.get_state(), f.y_pred(0, cs["T"])


def _sq_bound(tol, a, y):
    """what an elementwise error of tol x max |a| in a allows in sum (a - y)^2"""
    e = tol * float(np.max(np.abs(a)))
    return 2.0 * e * float(np.sum(np.abs(a - y))) + a.size * e * e


def _bits(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _rotation_boundary(c, f, cs, pb, rot, ref, last, tol):
    """the boundary of the rotation on a dense case that has finished its run: [(quantity, part, error, bound)]"""
    T, d, r = cs["T"], cs["d"], cs["r"]
    s = f.get_state()
    assert all(_bits(s[k], v) for k, v in f.get_state().items()), "get_state twice: the resident C was disturbed"
    full = {dt: f.y_pred(0, T, dtype=dt) for dt in (np.float64, np.float32)}
    for a, n in ((1, max(1, T - 2)), (T // 2, max(1, (T - T // 2) - 1))):          # interior wherever T >= 3
        for dt in full:
            assert _bits(f.y_pred(a, n, dtype=dt), full[dt][a:a + n]), (cs, a, n, dt)
    # project(I_r) is C: both come out of the resident U^T C, by two different GEMMs (and get_state's through the storage type)
    ptol = 2e-7 if cs["storage"] == "f32" else 1e-13          # 2^-23 of an entry; 2 d u of float64 sums at d <= 257
    errs = [("project(I)", last, relerr(f.project(np.eye(r)).T, s["C"]), ptol)]
    # the roll-out and the sums of squares, in original coordinates
    want = ref[-1]
    dyn = NC.BC.dynamics_of(pb)
    n_pred = 3
    roll = NC.O.predict_rollout(want["C"], want["mu"], want["theta"], dyn, T, n_pred)
    errs.append(("predict", last, relerr(f.predict(T, n_pred), roll), tol))
    held = np.random.default_rng(cs["seed"] ^ 0x4E1D).standard_normal((n_pred, d))
    sq = float(np.sum((roll - held) ** 2))
    errs.append(("predict_sq_error", last, abs(f.predict_sq_error(T, held) - sq), _sq_bound(tol, roll, held)))
    ran = next(rec for rec in reversed(ref) if rec["b"] > rec["a"])          # the last part that ran: its y_hat is the last pass's
    a, b, yp = ran["a"], ran["b"], ran["y_pred"]
    errs.append(("sq_error", last, abs(f.sq_error(a, b - a) - float(np.sum((yp - pb["Y"][a:b]) ** 2))), _sq_bound(tol, yp, pb["Y"][a:b])))
    # the series in pieces: the same bits as the whole-series upload, after the same run
    g = _open(c, cs, pb, rot=rot, pieces=True)
    try:
        s2, yp2 = _run_all(g, cs, pb)
    finally:
        g.close()
    assert _bits(yp2, full[np.float64]) and all(_bits(s2[k], s[k]) for k in s), (cs, "upload in pieces")
    return errs


def _sharded(c, cs, pb, n):
    from rpsmf_amd.sharding import shard_rows

    def worker(rank, comm):
        f = _open(c, cs, pb, shard=shard_rows(cs["d"], n, rank), comm=comm)
        try:
            return _run_all(f, cs, pb)
        finally:
            f.close()

    grp, out = netlib.run_ranks(n, worker, 50)
    assert grp.calls[0] > 0
    return [s for s, _ in out], [y for _, y in out]


def _shard_errors(c, cs, pb, one):
    """2 and 3 row shards of the case against its unsharded run `one` = (state, y_hat): replicated state bit-identical"""
    tol = 2e-6 if cs["storage"] == "f32" else 1e-11
    errs = []
    for n in cs["shards"]:
        states, yps = _sharded(c, cs, pb, n)
        for k in ("V", "P", "mu", "Q", "rho", "lam"):
            assert all(_bits(s[k], states[0][k]) for s in states[1:]), (cs, n, k)
        errs += [("C", f"{n} shards", relerr(np.vstack([s["C"] for s in states]), one[0]["C"]), tol), ("y_pred", f"{n} shards", relerr(np.hstack(yps), one[1]), tol)]
        errs += [(k, f"{n} shards", relerr(states[0][k], one[0][k]), tol) for k in ("V", "P", "mu", "rho")]
        assert states[0]["lam"] == one[0]["lam"]
    return errs


def _run_case(c, cs, pb, ref):
    rot = NC.eigen(pb, cs["d"]) if cs["family"] == "dense" else None
    f = _open(c, cs, pb, rot=rot)
    try:
        kernel, sp = _check_dispatch(f, cs)
        tol, gtol = NC.bar(cs), NC.gradsum_bar(cs)
        errs = []          # (quantity, part, error, bound)
        want = iter(ref)
        for ep in range(NC.passes_of(cs)):
            netlib.start_pass(f, cs, pb, ep)
            for j, (a, b) in enumerate(cs["parts"]):
                j += ep * len(cs["parts"])
                f.run(a, b)
                errs += netlib.state_errors(cs, f.get_state(), next(want), j, tol, gtol, y_pred=f.y_pred(a, b - a) if b > a else None)
        assert f.geometry()["filter_kernel"] == kernel and not f.step_plan()["usable"]
        if rot is not None:
            errs += _rotation_boundary(c, f, cs, pb, rot, ref, len(ref) - 1, tol)
        if cs["shards"]:
            errs += _shard_errors(c, cs, pb, (f.get_state(), f.y_pred(0, cs["T"])))
        return kernel, sp, errs
    finally:
        f.close()


@pytest.mark.parametrize("i", range(NC.N_CASES))
def test_noise_net(i):
    from rpsmf_amd import _capi as c

    t0 = time.perf_counter()
    cs = NC.device_case(i)
    pb = NC.problem(cs)
    ref = NC.reference(cs, pb)
    t1 = time.perf_counter()
    with netlib.env(cs["env"]):
        kernel, sp, errs = _run_case(c, cs, pb, ref)
    worst = netlib.verdict(errs)
    print(f"\nNET case={i} target={cs['family']}:{cs['spectrum']} kernel={kernel} plan=(wg={sp['n_row_wg']} rows={sp['rows_per_wg']} np={sp['np']} cu={sp['n_cu']}) "
          f"storage={cs['storage']} upload={cs['upload']} masked=0 dyn={cs['dyn']} hooks={cs['hooks']} filter={cs['filter']} r={cs['r']} d={cs['d']} T={cs['T']} "
          f"parts={cs['parts']} passes={NC.passes_of(cs)} robust={int(cs['robust'])} rec={cs['recursive']} sched={int(cs['sched'])} genQ={int(cs['general_Q'])} "
          f"env={cs['env']} shards={cs['shards']} bar={NC.bar(cs):.0e} worst={worst[0]}@{worst[1]} err={worst[2]:.3e} ratio={worst[2] / worst[3]:.3g} "
          f"wall={time.perf_counter() - t0:.2f}s (oracle {t1 - t0:.2f}s)")
    netlib.assert_within(errs, cs)
