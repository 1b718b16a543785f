"""The per-step engine on configurations drawn at random (seeded, tests/step_cases.py) and aimed at the persistent kernel
psmf_pstep_k: every one of its 44 instances (padded rank 8 / 16 / 32 / 64 x 4 / 8 / 12 / 16 row passes x float32 / float64 storage
x unmasked / masked) on two cases at least, rows from 1 to 783 360 -- below one row pass, one workgroup against two, a last
workgroup of one row, every NP threshold, the hub's fan-in exactly full, the windows of d at 33 <= r <= 48 that the planner used
to refuse -- cos-phase dynamics, the in-loop Adam / SGD, the five hook configurations, R_k / Q_k schedules and a general Q on the
big-d instances too, PSMF / rPSMF with fixed lambda and scaling factors, one to three launches with cuts at 1 and T - 1, empty
runs, a second pass; masked handles with a row never observed, a column without observations, a whole row workgroup unobserved
and the last workgroup observed alone; and every reason for which a handle keeps the launches per timestep.  Each against the
float64 oracle after every run part (masked: oracle/impute_oracle.py, at the end of the pass), and each asserts that the handle
reports the kernel and the launch geometry that step_cases.plan / expected_kernel restate.
GPU only: `pytest -m gpu`; `-s` shows the error figures of every case (each prints before it asserts).

Bars (the ones the suite states for this engine, step_cases.bar): float64 storage 1e-9, masked 5e-9, gradsum 1e-7; float32
storage 1e-5; coverage of the masked bands exactly (float32: 5e-4).  tests/test_step_cases_cpu.py has shown that the oracle's own
response to a last-bit change of the inputs sits 16 x inside them for every case.  The coverage claims of that file are for a
device of 256 compute units; on another count the expectations are recomputed with the device's.
Measured on one MI355X: the whole file takes 15 s, its slowest case 0.6 s (profiles/step_engine_net_gpu_tests.txt); the limit below is per case.
Reference: pypsmf/psmf/psmf.py:85-188,287-304, rpsmf.py:116-184; ExperimentImpute/PSMF.py:40-95, rPSMF.py:40-148."""

import time

import numpy as np
import pytest

import netlib
import step_cases as SC
from conftest import relerr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(60)]


def _check_dispatch(f, cs):
    """the handle reports the kernel and the plan the tables predict; returns (kernel, plan as reported)"""
    sp = f.step_plan()
    n_cu = sp["n_cu"]
    want = SC.expected_kernel(cs, n_cu)
    got = f.geometry()["filter_kernel"]
    assert got == want, (cs, got, want, SC.launched_reason(cs, n_cu), sp)
    assert sp["usable"] == (want == "psmf_pstep_k"), (cs, sp)
    # the planner runs wherever the switches, the rank, R and the dynamics admit the kernel: its answer is kept with the handle
    p = SC.plan(cs["d"], cs["r"], n_cu, cs["masked"]) if SC.launched_reason(cs, n_cu) in (None, "rows") else None
    reported = (sp["n_row_wg"], sp["rows_per_wg"], sp["np"])
    assert reported == ((p["n_row_wg"], p["rows_per_wg"], p["np"]) if p else (0, 0, 0)), (cs, sp, p)
    return got, sp


def _run_unmasked(c, cs, pb, ref):
    nl = pb["nl"]
    f = netlib.open_filter(c, cs, pb, "step", nonuniform_R=cs["nonuniform"])
    try:
        if cs["nonuniform"]:
            f.set_row_noise(pb["rho_rows"])
        f.upload_series(pb["Y"])
        f.set_state(pb["C0"], pb["V0"], pb["P0"], pb["Q"], pb["mu0"], rho=pb["rho"], lambda0=pb["lam"], theta=pb["theta"] if nl.n_params else None)
        if cs["sched"]:
            f.set_schedules(pb["rho_k"], pb["q_k"])
        kernel, sp = _check_dispatch(f, cs)
        tol, gtol = SC.bar(cs), SC.gradsum_bar(cs)
        errs = []          # (quantity, part, error, bound)
        want = iter(ref)
        for ep in range(SC.passes_of(cs)):
            netlib.start_pass(f, cs, pb, ep)
            for j, (a, b) in enumerate(cs["parts"]):
                j += ep * len(cs["parts"])
                f.run(a, b)
                # (rho is not compared where R is not uniform: the oracle's is diag(R), a vector)
                errs += netlib.state_errors(cs, f.get_state(), next(want), j, tol, gtol, y_pred=f.y_pred(a, b - a) if b > a else None,
                                            skip=("rho",) if cs["nonuniform"] else ())
        assert f.geometry()["filter_kernel"] == kernel
        return kernel, sp, errs
    finally:
        f.close()


def _run_masked(c, cs, pb, ref):
    T = cs["T"]
    f = c.DeviceFilter(cs["d"], cs["r"], robust=cs["robust"], storage=cs["storage"], masked=True, engine="step")
    try:
        f.upload_series(np.ascontiguousarray(pb["Yorig"].T))
        f.upload_mask(np.ascontiguousarray(pb["M"].T))
        f.set_state(pb["C0"], pb["V0"], pb["P0"], pb["Q"], pb["X0"][:, T - 1], rho=pb["rho"], lambda0=pb["lam"])
        kernel, sp = _check_dispatch(f, cs)
        for a, b in cs["parts"]:
            f.run(a, b)
        s, X, m = f.get_state(), f.mu_history(1, T), f.masked_metrics(np.ascontiguousarray(pb["Mmiss"].T), pb["sig"])
        tol = SC.bar(cs)
        assert m[3] == pb["Mmiss"].sum()
        errs = [(k, 0, relerr(s[k], ref[k]), tol) for k in ("C", "V", "P")] + [("X", 0, relerr(X, ref["X"]), tol)]
        errs += [("Epred", 0, relerr(np.sqrt(m[0] / m[3]), ref["Epred"]), tol), ("Efull", 0, relerr(np.sqrt(m[1] / m[3]), ref["Efull"]), tol)]
        cov = abs(m[2] / m[3] - ref["coverage"])
        errs.append(("coverage", 0, cov, SC.coverage_bar(cs) if cs["storage"] == "f32" else 0.5 / m[3]))      # (float64: the same count)
        return kernel, sp, errs
    finally:
        f.close()


@pytest.mark.parametrize("i", range(SC.N_CASES))
def test_step_engine_net(i):
    from rpsmf_amd import _capi as c

    t0 = time.perf_counter()
    cs = SC.device_case(i)
    pb = SC.problem(cs)
    ref = SC.reference(cs, pb)
    t1 = time.perf_counter()
    with netlib.env(cs["env"]):
        kernel, sp, errs = (_run_masked if cs["masked"] else _run_unmasked)(c, cs, pb, ref)
    worst = netlib.verdict(errs)
    print(f"\nNET case={i} target={cs['target']} kernel={kernel} plan=(wg={sp['n_row_wg']} rows={sp['rows_per_wg']} np={sp['np']} cu={sp['n_cu']}) "
          f"storage={cs['storage']} masked={int(cs['masked'])} dyn={cs['dyn']} hooks={cs['hooks']} r={cs['r']} d={cs['d']} T={cs['T']} parts={cs['parts']} "
          f"passes={SC.passes_of(cs)} robust={int(cs['robust'])} rec={cs['recursive']} sched={int(cs['sched'])} genQ={int(cs['general_Q'])} env={cs['env']} "
          f"bar={SC.bar(cs):.0e} worst={worst[0]}@{worst[1]} err={worst[2]:.3e} ratio={worst[2] / worst[3]:.3g} "
          f"wall={time.perf_counter() - t0:.2f}s (oracle {t1 - t0:.2f}s)")
    netlib.assert_within(errs, cs)
