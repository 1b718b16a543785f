"""The launched form of the per-step engine on configurations drawn at random (seeded, tests/gram_cases.py) and aimed at the
matrix-core Gram mgram_body (psmf_masked.hip): the masked Gram of psmf_serial_mgram -- its ten instances under every reason
that keeps a masked handle on the launches per timestep (MLE-SMF, TMF, r > 32, PSMF_STEP_PERSISTENT=0, row shards) -- and the
weighted Gram of psmf_wgram_mfma -- its eight instances and the vector-unit twin -- with rows from 8 to 163 847: one partial slab
with 255 idle workgroups, exactly one slab per wave, a second slab of a single row, three trips through a wave's slab loop;
dense SPD V0 and P0, a general Q in half the cases, one to three passes (a quarter of the masked cases through impute_batch), runs cut behind the empty and the full column of the
mask (in half the cases the mean handed back through set_state at the cut: the look-ahead Gram re-formed there), masks with a row never observed, one wave's slab
unobserved, the last slab observed alone and -- on the big-row cases -- only the slabs of a second trip observed; non-uniform R
over three decades and rotated (dense) R; 2 .. 4 uneven shards with a shard of three rows, shards astride the one-slab bound.
Each against the float64 oracle (oracle/impute_oracle.py; oracle/psmf_oracle.py after every run part), sharded cases also
against the unsharded handle, with replicated state bit-identical and the message sizes counted.
GPU only: `pytest -m gpu`; `-s` shows the error figures of every case (each prints before it asserts).

Bars (the ones the suite states for these paths, gram_cases.bar): masked 5e-9, weighted 1e-9, float32 storage 1e-5; coverage
exactly (float32: 5e-4); sharded against unsharded 1e-11.  tests/test_gram_cases_cpu.py has shown that the oracle's own response
to a last-bit change of the inputs sits 16 x inside them for every case.
Reference: ExperimentImpute/PSMF.py:40-95, rPSMF.py:40-148, MLESMF.py:40-92, TMF.py:30-73; pypsmf/psmf/psmf.py:140-152."""

import time

import numpy as np
import pytest

import gram_cases as GC
import netlib
from conftest import relerr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

METHOD_CODE = {"psmf": 1, "rpsmf": 1, "mle_smf": 2, "tmf": 3}          # cfg.masked (include/psmf_hip.h)


def _gam(ep):
    return 1e-6 / (ep + 1) ** 0.7          # MLESMF.py:59-60, TMF.py:46-48


# ---- masked cases
def _masked_handle(c, cs, pb, row0, dl, comm=None):
    """One masked handle (or row shard) over the passes and parts of the case -> dict(s, X, yp, m, sc, kernel)."""
    T, r = cs["T"], cs["r"]
    sl = slice(row0, row0 + dl)
    f = c.DeviceFilter(cs["d"], r, robust=cs["robust"], storage=cs["storage"], masked=METHOD_CODE[cs["method"]], engine="step", row0=row0, d_local=dl)
    try:
        if comm is not None:
            f.comm_init_host(*comm)
        Mt = np.ascontiguousarray(pb["M"].T[:, sl])
        f.upload_series(np.ascontiguousarray(pb["Y"].T[:, sl]))
        f.upload_mask(Mt)
        mu0 = pb["X0"][:, T - 1]
        if cs["method"] == "tmf":            # TMF.py:47,60: Pbar = I / nu at every step, nu = 2 -- as Q with P = 0; V unused
            f.set_state(pb["C0"][sl], np.eye(r), np.zeros((r, r)), 0.5 * np.eye(r), mu0, rho=1.0, lambda0=0.0)
        else:
            f.set_state(pb["C0"][sl], pb["V0"], pb["P0"], pb["Q"], mu0, rho=cs["rho"], lambda0=cs["lam"] if cs["robust"] else 0.0)
        kernel = f.geometry()["filter_kernel"]
        for ep in range(cs["passes"]):
            if ep and cs["robust"]:          # rPSMF.py:77-79: Q, R, lambda restart; V, P, C and the mean carry over
                f.set_state(Q=pb["Q"], rho=cs["rho"], lambda0=cs["lam"])
            if cs["method"] in ("mle_smf", "tmf"):
                f.set_step_size(_gam(ep))
            for j, (a, b) in enumerate(cs["parts"]):
                if j and cs["restate"]:      # a state set between two runs: the next one prepares again, the look-ahead Gram of step a + 1 included
                    f.set_state(mu=f.get_state(want_C=False)["mu"])
                f.run(a, b)
        out = dict(s=f.get_state(), X=f.mu_history(1, T), yp=f.y_pred(0, T), sc=f.step_scalars(0, T), kernel=kernel,
                   m=f.masked_metrics(np.ascontiguousarray(pb["Mmiss"].T[:, sl]), 0.0 if cs["method"] == "tmf" else cs["sig"]))
        assert f.geometry()["filter_kernel"] == kernel
        return out
    finally:
        f.close()


def _bands(cs, pb, yp, sc):
    """the bands from the step scalars (s_t, eta_t): PSMF.py:83-84, rPSMF.py:121-123, MLESMF.py:81-82"""
    s, eta = sc[:, 0:1], sc[:, 1:2]
    band = cs["sig"] * np.sqrt(s * pb["M"].T + eta if cs["robust"] else s + eta)
    return yp - band, yp + band


def _masked_errs(cs, pb, ref, got, tol):
    m = got["m"]
    assert m[3] == pb["Mmiss"].sum()
    errs = [("C", relerr(got["C"], ref["C"]), tol), ("X", relerr(got["X"], ref["X"]), tol), ("y_hat", relerr(got["yp"], ref["Yrec"]), tol)]
    errs += [(k, relerr(got[k], ref[k]), tol) for k in ("V", "P") if k in ref and k in got]
    errs += [("Epred", relerr(np.sqrt(m[0] / m[3]), ref["Epred"][-1]), tol), ("Efull", relerr(np.sqrt(m[1] / m[3]), ref["Efull"][-1]), tol)]
    if "coverage" in ref:
        lo, hi = _bands(cs, pb, got["yp"], got["sc"])
        errs += [("band_low", relerr(lo, ref["YrecL"]), tol), ("band_high", relerr(hi, ref["YrecH"]), tol)]
        errs.append(("coverage", abs(m[2] / m[3] - ref["coverage"]), GC.coverage_bar(cs) if cs["storage"] == "f32" else 0.5 / m[3]))      # (float64: the same count)
    return errs


def _run_masked(c, cs, pb, ref):
    tol, r, T = GC.bar(cs), cs["r"], cs["T"]
    if cs["route"] == "batch":
        from rpsmf_amd import impute

        res = impute.impute_batch(pb["Y"], pb["M"], pb["Mmiss"], pb["C0"], pb["X0"], pb["V0"], pb["Q"], cs["rho"], pb["P0"],
                                  0.0 if cs["method"] == "tmf" else cs["sig"], cs["passes"], robust=cs["robust"], lambda0=cs["lam"],
                                  want_bands=True, method=cs["method"] if cs["method"] in ("mle_smf", "tmf") else None)
        assert res["kernel"] == "masked per-step engine" and res["status"][0] == 0, (res["kernel"], res["status"])
        errs = [("C", relerr(res["C"][0], ref["C"]), tol), ("X", relerr(res["X"][0].T, ref["X"]), tol), ("y_hat", relerr(res["Yrec"][0].T, ref["Yrec"]), tol),
                ("Epred", relerr(res["Epred"][0], ref["Epred"]), tol), ("Efull", relerr(res["Efull"][0], ref["Efull"]), tol)]
        if "coverage" in ref:
            errs += [("band_low", relerr(res["YrecL"][0].T, ref["YrecL"]), tol), ("band_high", relerr(res["YrecH"][0].T, ref["YrecH"]), tol),
                     ("coverage", abs(res["inside"][0] - ref["coverage"]), 0.5 / pb["Mmiss"].sum())]
        return res["kernel"], errs
    whole = _masked_handle(c, cs, pb, 0, cs["d"])
    # (a PSMF / rPSMF handle at r <= 32 is on the launches per timestep because of its shards alone: unsharded, the persistent kernel)
    assert whole["kernel"] == ("psmf_pstep_k" if cs["target"][3] == "shards" else "psmf_sweep_solve"), whole["kernel"]
    flat = lambda o: dict(o["s"], X=o["X"], yp=o["yp"], sc=o["sc"], m=o["m"])          # noqa: E731
    errs = _masked_errs(cs, pb, ref, flat(whole), tol)
    if cs["shards"]:
        row0 = np.concatenate([[0], np.cumsum(cs["shards"])]).astype(int)
        grp, out = netlib.run_ranks(len(cs["shards"]), lambda rank, comm: _masked_handle(c, cs, pb, int(row0[rank]), cs["shards"][rank], comm), 100)
        assert all(o["kernel"] == "psmf_sweep_solve" for o in out), [o["kernel"] for o in out]
        for o in out[1:]:                    # replicated state: the same bits on every shard
            for k in {"psmf": ("V", "P", "mu"), "rpsmf": ("V", "P", "mu"), "mle_smf": ("P", "mu"), "tmf": ("mu",)}[cs["method"]]:      # (what the method keeps)
                assert np.array_equal(o["s"][k], out[0]["s"][k]), k
            assert np.array_equal(o["X"], out[0]["X"]) and np.array_equal(o["sc"], out[0]["sc"])
        gathered = dict(out[0]["s"], C=np.concatenate([o["s"]["C"] for o in out]), X=out[0]["X"], sc=out[0]["sc"],
                        yp=np.concatenate([o["yp"] for o in out], axis=1), m=sum(o["m"] for o in out))
        errs += [("sharded " + k, e, b) for k, e, b in _masked_errs(cs, pb, ref, gathered, tol)]
        if cs["storage"] == "f64":
            errs += [("vs whole " + k, relerr(gathered[k], flat(whole)[k]), GC.SHARD_BAR) for k in ("C", "X", "yp") + tuple(k for k in ("V", "P") if k in ref)]          # (V, P: where the method keeps them)
            assert gathered["m"][3] == whole["m"][3] and gathered["m"][2] == whole["m"][2]          # the two counts are integers
        # per step one (h, ee) message of r + 1 doubles and one masked Gram of r^2 + 1, formed a step ahead: + one at every start
        # of a run that prepares (each pass, and each cut where the state was set again)
        starts = cs["passes"] * (1 + (len(cs["parts"]) - 1 if cs["restate"] else 0))
        assert set(grp.sizes) == {r * r + 1, r + 1}, set(grp.sizes)
        assert grp.sizes.count(r + 1) == cs["passes"] * T and grp.sizes.count(r * r + 1) == cs["passes"] * T + starts, (grp.sizes.count(r + 1), grp.sizes.count(r * r + 1), starts)
    return whole["kernel"], errs


# ---- weighted cases
def _weighted_handle(c, cs, pb, ref, row0, dl, comm=None):
    """One non-uniform-R handle (or row shard) -> (kernel, the state and y_pred after every part)"""
    sl = slice(row0, row0 + dl)
    f = c.DeviceFilter(cs["d"], cs["r"], robust=cs["robust"], storage=cs["storage"], engine="step", nonuniform_R=True, row0=row0, d_local=dl)
    try:
        if comm is not None:
            f.comm_init_host(*comm)
        if cs["rotated"]:
            f.set_noise_rotation(pb["U"], pb["rho_rows"])
        else:
            f.set_row_noise(pb["rho_rows"][sl], rho_mean=float(pb["rho_rows"].sum()) / cs["d"])
        f.upload_series(np.ascontiguousarray(pb["Y"][:, sl]))
        f.set_state(pb["C0"][sl], pb["V0"], pb["P0"], pb["Q"], pb["mu0"], rho=1.0, lambda0=cs["lam"])
        kernel = f.geometry()["filter_kernel"]
        recs = []
        for ep in range(cs["passes"]):
            if ep and cs["robust"]:          # rPSMF's step_reset (rpsmf.py:106-114)
                f.set_state(Q=pb["Q"], rho=1.0, lambda0=cs["lam"])
            for a, b in cs["parts"]:
                f.run(a, b)
                s = f.get_state()
                recs.append(dict(C=s["C"], V=s["V"], mu=s["mu"], P=s["P"], y_pred=f.y_pred(a, b - a)))
        return kernel, recs
    finally:
        f.close()


def _run_weighted(c, cs, pb, ref):
    tol, r = GC.bar(cs), cs["r"]
    kernel, whole = _weighted_handle(c, cs, pb, ref, 0, cs["d"])
    assert kernel == "psmf_sweep_solve", kernel
    errs = [(f"{k}@{j}", relerr(g[k], w[k]), tol) for j, (g, w) in enumerate(zip(whole, ref)) for k in GC.WEIGHTED_KEYS]
    if cs["shards"]:
        row0 = np.concatenate([[0], np.cumsum(cs["shards"])]).astype(int)
        grp, out = netlib.run_ranks(len(cs["shards"]), lambda rank, comm: _weighted_handle(c, cs, pb, ref, int(row0[rank]), cs["shards"][rank], comm)[1], 100)
        for j, w in enumerate(ref):
            for o in out[1:]:
                for k in ("V", "P", "mu"):
                    assert np.array_equal(o[j][k], out[0][j][k]), (k, j)
            g = dict(out[0][j], C=np.concatenate([o[j]["C"] for o in out]), y_pred=np.concatenate([o[j]["y_pred"] for o in out], axis=1))
            errs += [(f"sharded {k}@{j}", relerr(g[k], w[k]), tol) for k in GC.WEIGHTED_KEYS]
            if cs["storage"] == "f64":
                errs += [(f"vs whole {k}@{j}", relerr(g[k], whole[j][k]), GC.SHARD_BAR) for k in GC.WEIGHTED_KEYS]
        # per step: the weighted Gram GR (r^2 doubles) and the step's partial sums (2 (r + 1)); + the exact Gram at the start of every pass
        steps = cs["passes"] * cs["T"]
        count = {n: grp.sizes.count(n) for n in sorted(set(grp.sizes))}
        assert count == {2 * (r + 1): steps, r * r: steps + cs["passes"]}, (count, steps)
    return kernel, errs


@pytest.mark.parametrize("i", range(GC.N_CASES))
def test_masked_gram_net(i):
    from rpsmf_amd import _capi as c

    t0 = time.perf_counter()
    cs = GC.device_case(i)
    pb = GC.problem(cs)
    with np.errstate(all="ignore"):
        ref = GC.reference(cs, pb)
    t1 = time.perf_counter()
    with netlib.env(cs["env"]):
        kernel, errs = (_run_masked if cs["masked"] else _run_weighted)(c, cs, pb, ref)
    p = GC.plan_of(cs)
    worst = max(errs, key=lambda e: (e[1] / e[2]) if np.isfinite(e[1]) else np.inf)
    print(f"\nGRAM case={i} target={cs['target']} kernel={kernel} plan=(nt={p['nt']} nw={p['nw']} slabs={p['n_slab']} trips={p['trips']} last={p['last_rows']}) "
          f"method={cs['method']} storage={cs['storage']} r={cs['r']} d={cs['d']} shards={cs['shards']} T={cs['T']} parts={cs['parts']} passes={cs['passes']} "
          f"route={cs['route']} genQ={int(cs['general_Q'])} rotated={int(cs['rotated'])} restate={int(cs['restate'])} env={cs['env']} "
          f"bar={GC.bar(cs):.0e} worst={worst[0]} err={worst[1]:.3e} ratio={worst[1] / worst[2]:.3g} "
          f"wall={time.perf_counter() - t0:.2f}s (oracle {t1 - t0:.2f}s)")
    bad = [e for e in errs if not e[1] < e[2]]
    assert not bad, (cs, bad)


def test_an_identity_all_reduce_disagrees():
    """Negative control: a shard whose 'all-reduce' hands its own partial sums back does not reproduce the filter -- masked
    (the Gram and the count of r^2 + 1, the (h, ee) of r + 1) and weighted (GR of r^2)."""
    from rpsmf_amd import _capi as c

    # masked: the case whose first shard holds most of the rows (its own sums stay solvable); weighted: the first sharded case
    masked = max((i for i, s in enumerate(GC.SPECS) if s[2] and s[0][0] == "m"), key=lambda i: GC.SPECS[i][2][1][0] / sum(GC.SPECS[i][2][1]))
    for i in (masked, next(i for i, s in enumerate(GC.SPECS) if s[2] and s[0][0] == "w")):
        cs = GC.device_case(i)
        pb = GC.problem(cs)
        solo = (len(cs["shards"]), 0, lambda v: v)
        if cs["masked"]:
            whole, bad = _masked_handle(c, cs, pb, 0, cs["d"]), _masked_handle(c, cs, pb, 0, cs["shards"][0], solo)
            err = relerr(bad["X"], whole["X"])
        else:
            whole, bad = _weighted_handle(c, cs, pb, None, 0, cs["d"])[1], _weighted_handle(c, cs, pb, None, 0, cs["shards"][0], solo)[1]
            err = relerr(bad[-1]["mu"], whole[-1]["mu"])
        print(f"\nidentity all-reduce, case {i}: {err:.3e}")
        assert np.isfinite(err) and err > 1e-6, (i, err)


def test_a_mask_that_arrives_in_pieces():
    """The masked Gram is formed one step ahead: a run that stops at the end of the uploaded mask has read the row behind it,
    which was never written.  The rows uploaded afterwards must be taken up: the piecewise handle ends where the handle that had
    the whole mask from the start ends (same kernels, same order of the sums: 1e-11, the bar of sharded against unsharded),
    on the launched form (r = 40) and on the persistent kernel (r = 5).  A range beyond the uploaded rows is refused by name."""
    from rpsmf_amd import _capi as c

    d, T, cut = 300, 12, 7
    rng = np.random.default_rng(11)
    Y = np.cumsum(0.3 * rng.standard_normal((T, d)), axis=0) + 3.0
    M = (rng.random((T, d)) > 0.4).astype(np.uint8)
    M[cut] = 0
    M[cut, :3] = 1                       # the row behind the first piece: three observations, far from whatever the memory holds
    for r, kernel in ((40, "psmf_sweep_solve"), (5, "psmf_pstep_k")):
        C0 = rng.random((d, r))
        out = []
        for pieces in (False, True):
            f = c.DeviceFilter(d, r, storage="f64", masked=1, engine="step")
            try:
                f.upload_series(Y)
                f.upload_mask(M[:cut] if pieces else M)
                f.set_state(C0, netlib.spd(np.random.default_rng(r), r, 2.0), np.eye(r), 0.1 * np.eye(r), np.full(r, 0.3), rho=5.0)
                assert f.geometry()["filter_kernel"] == kernel
                if pieces:
                    with pytest.raises(ValueError, match="beyond the uploaded mask"):
                        f.run(0, T)
                f.run(0, cut)
                if pieces:
                    f.upload_mask(M[cut:], cut)
                f.run(cut, T)
                s = f.get_state()
                assert s["k"] == T
                out.append(dict(C=s["C"], V=s["V"], P=s["P"], X=f.mu_history(1, T), yp=f.y_pred(0, T), sc=f.step_scalars(0, T)))
            finally:
                f.close()
        errs = {k: relerr(out[1][k], out[0][k]) for k in out[0]}
        print(f"\nmask in pieces, r={r} ({kernel}): {errs}")
        assert max(errs.values()) <= GC.SHARD_BAR, (r, errs)


def test_refusals_by_message():
    """What the ABI refuses around these paths, each by its message: schedules and cos-phase dynamics on a masked handle,
    psmf_set_row_noise on a handle created without nonuniform_R, a run beyond the uploaded mask, a rotation on row shards."""
    from rpsmf_amd import _capi as c

    d, r, T = 40, 5, 6
    rng = np.random.default_rng(4)
    f = c.DeviceFilter(d, r, storage="f64", masked=1, engine="step")
    try:
        with pytest.raises(ValueError, match="masked handles take a constant R"):
            f.set_schedules(np.ones(T + 1), None)
        with pytest.raises(ValueError, match="masked handles take a constant Q"):
            f.set_q_matrix_schedule(np.tile(np.eye(r), (T + 1, 1, 1)))
        with pytest.raises(c.PsmfError, match="nonuniform_R = 0"):
            f.set_row_noise(np.ones(d))
        f.upload_series(rng.standard_normal((T, d)))
        f.set_state(rng.random((d, r)), np.eye(r), np.eye(r), 0.1 * np.eye(r), np.zeros(r), rho=1.0)
        with pytest.raises(c.PsmfError, match="psmf_upload_mask first"):
            f.run(0, T)
        with pytest.raises((ValueError, c.PsmfError), match="psmf_upload_mask"):
            f.upload_mask(np.ones((T + 1, d)))          # longer than the series that sized the mask buffer
        # a mask shorter than the run: the rows behind it were never written (the buffer is not cleared when it is allocated)
        f.upload_mask(np.ones((T - 2, d)))
        with pytest.raises(ValueError, match="beyond the uploaded mask"):
            f.run(0, T)
        f.upload_mask(np.ones((1, d)), T - 1)          # behind a gap: does not count
        with pytest.raises(ValueError, match="beyond the uploaded mask"):
            f.run(0, T)
    finally:
        f.close()
    with pytest.raises(ValueError, match="random-walk"):
        c.DeviceFilter(d, r, masked=1, dyn_kind=c.DYN_COS_PHASE, engine="step", storage="f64")
    g = c.DeviceFilter(d, r, storage="f64", nonuniform_R=True, engine="step", row0=0, d_local=d // 2)
    try:
        with pytest.raises(c.PsmfError, match="one shard only"):
            g.set_noise_rotation(np.eye(d), np.ones(d))
    finally:
        g.close()
