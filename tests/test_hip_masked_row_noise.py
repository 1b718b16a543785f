"""The masked per-step engine of the large-d handle with per-row observation noise: DeviceFilter(masked = 1 / 2, nonuniform_R =
True) -- the masked weighted Gram sum_i m_i c_i c_i^T / (rho rho_i + s) of every step on the matrix cores (psmf_mwgram_mfma,
rpsmf_amd/csrc/psmf_masked.hip) in front of the sweep, the unweighted masked Gram one step ahead beside the serial stage with
sum m_i rho_i in its count slot.  The cases of tests/masked_noise_cases.py (conditioned by tests/test_masked_noise_cases_cpu.py)
against oracle/impute_oracle.py with the (d,) vector, two passes, each cut in two runs; two uneven row shards; the series ring;
a vector of equal entries against the uniform handle; the refusals; and the uniform masked handle against the bits it gave before
the count slot changed (tests/golden/masked_uniform_parent.npz, tests/golden/make_golden_masked_uniform.py).
GPU only: `pytest -m gpu`; `-s` shows the error figures (each prints before it asserts).

Bars: the ones the suite states for this engine (tests/gram_cases.py: bar, coverage_bar, SHARD_BAR) -- float64 storage 5e-9 and the
coverage exactly, float32 storage 1e-5 and the coverage within 5e-4, sharded against unsharded 1e-11.
Reference: ExperimentImpute/PSMF.py:40-95 (70-72), rPSMF.py:40-148 (91-98), MLESMF.py:40-92 (70-76)."""

import os

import numpy as np
import pytest

import gram_cases as GC
import masked_noise_cases as MC
import netlib
from conftest import relerr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "masked_uniform_parent.npz")


def _gam(ep):
    return 1e-6 / (ep + 1) ** 0.7          # MLESMF.py:59-60


def run_handle(c, cs, pb, row0=0, dl=None, comm=None, rho_rows="case", rho=1.0, passes=None):
    """One handle (or row shard) over the passes of the case, each pass cut in two runs -> dict(s, X, yp, sc, m).
    rho_rows = "case": per-row noise from the problem (rho the scalar in front); None: a uniform handle with R = rho I."""
    d, n, r = cs["d"], cs["n"], cs["r"]
    dl = d if dl is None else dl
    sl = slice(row0, row0 + dl)
    rows = pb["rho"] if isinstance(rho_rows, str) else rho_rows
    f = c.DeviceFilter(d, r, robust=cs["robust"], storage=cs["storage"], masked=MC.METHOD_CODE[cs["method"]], engine="step",
                       nonuniform_R=rows is not None, row0=row0, d_local=dl)
    try:
        if comm is not None:
            f.comm_init_host(*comm)
        f.upload_series(np.ascontiguousarray(pb["Yorig"].T[:, sl]))
        f.upload_mask(np.ascontiguousarray(pb["M"].T[:, sl]))
        if rows is not None:
            f.set_row_noise(rows[sl], float(rows.sum()) / d)
        f.set_state(pb["C0"][sl], pb["V"], pb["P"], pb["Q"], pb["X0"][:, n - 1], rho=rho, lambda0=MC.LAMBDA0 if cs["robust"] else 0.0)
        for ep in range(cs["passes"] if passes is None else passes):
            if ep and cs["robust"]:          # rPSMF.py:77-79: Q, R, lambda restart; V, P, C and the mean carry over
                f.set_state(Q=pb["Q"], rho=rho, lambda0=MC.LAMBDA0)
            if cs["method"] == "mle_smf":
                f.set_step_size(_gam(ep))
            f.run(0, n // 2)
            f.run(n // 2, n)
        assert f.geometry()["filter_kernel"] == "psmf_sweep_solve"
        return dict(s=f.get_state(), X=f.mu_history(1, n), yp=f.y_pred(0, n), sc=f.step_scalars(0, n),
                    m=f.masked_metrics(np.ascontiguousarray(pb["Mmiss"].T[:, sl]), MC.SIG))
    finally:
        f.close()


def _bands(cs, pb, yp, sc):
    """the bands from the step scalars (s_t, eta_t): PSMF.py:83-84, rPSMF.py:121-123, MLESMF.py:81-82 (s_t = 0 there)"""
    s, eta = sc[:, 0:1], sc[:, 1:2]
    band = MC.SIG * np.sqrt(s * pb["M"].T + eta if cs["robust"] else s + eta)
    return yp - band, yp + band


def _errs(cs, pb, ref, C, X, yp, sc, m):
    tol = GC.bar(cs)
    lo, hi = _bands(cs, pb, yp, sc)
    assert m[3] == pb["Mmiss"].sum()
    return [("C", relerr(C, ref["C"]), tol), ("X", relerr(X, ref["X"]), tol), ("Yrec", relerr(yp, ref["Yrec"]), tol),
            ("YrecL", relerr(lo, ref["YrecL"]), tol), ("YrecH", relerr(hi, ref["YrecH"]), tol),
            ("Epred", relerr(np.sqrt(m[0] / m[3]), ref["Epred"][-1]), tol), ("Efull", relerr(np.sqrt(m[1] / m[3]), ref["Efull"][-1]), tol),
            ("inside", abs(m[2] / m[3] - ref["coverage"]), GC.coverage_bar(cs) if cs["storage"] == "f32" else 0.5 / m[3])]      # (float64: the same count)


def _report(what, errs):
    worst = max(errs, key=lambda e: (e[1] / e[2]) if np.isfinite(e[1]) else np.inf)
    print(f"\nROW NOISE {what}: " + " ".join(f"{k}={e:.3e}" for k, e, _ in errs) + f"  worst {worst[0]} at {worst[1] / worst[2]:.3g} of its bar")
    bad = [e for e in errs if not e[1] < e[2]]
    assert not bad, (what, bad)


@pytest.mark.parametrize("cs", MC.CASES, ids=MC.IDS)
def test_masked_row_noise_vs_oracle(cs):
    """Every case, every method listed, against the oracle run with the (d,) vector."""
    from rpsmf_amd import _capi as c

    pb, ref = MC.reference(cs)
    got = run_handle(c, cs, pb)
    _report(MC.IDS[MC.CASES.index(cs)], _errs(cs, pb, ref, got["s"]["C"], got["X"], got["yp"], got["sc"], got["m"]))


@pytest.mark.parametrize("method", ["psmf", "rpsmf"])
def test_two_uneven_shards(method):
    """(2001, 50, 20) on two uneven row shards under the host communicator: gathered C and y_hat and summed metrics equal the
    unsharded handle's within SHARD_BAR (and the oracle within the case's bar); replicated V, P, mu bit-identical; per step one
    masked weighted Gram of r^2 doubles, one (h, ee | b, q) message of 2 (r + 1) and one look-ahead masked Gram of r^2 + 1."""
    from rpsmf_amd import _capi as c

    cs = MC.find(2001, 20, method)
    pb, ref = MC.reference(cs)
    d, n, r = cs["d"], cs["n"], cs["r"]
    whole = run_handle(c, cs, pb)
    shards = (1207, 794)
    row0 = (0, shards[0])
    grp, out = netlib.run_ranks(2, lambda rank, comm: run_handle(c, cs, pb, row0[rank], shards[rank], comm), 100)
    for k in ("V", "P", "mu"):
        assert np.array_equal(out[0]["s"][k], out[1]["s"][k]), k
    assert np.array_equal(out[0]["X"], out[1]["X"]) and np.array_equal(out[0]["sc"], out[1]["sc"])
    Cg = np.concatenate([o["s"]["C"] for o in out])
    ypg = np.concatenate([o["yp"] for o in out], axis=1)
    m = out[0]["m"] + out[1]["m"]
    vs = [("vs whole " + k, relerr(a, b), GC.SHARD_BAR) for k, a, b in (("C", Cg, whole["s"]["C"]), ("y_hat", ypg, whole["yp"]), ("X", out[0]["X"], whole["X"]),
                                                                         ("V", out[0]["s"]["V"], whole["s"]["V"]), ("P", out[0]["s"]["P"], whole["s"]["P"]))]
    vs += [("vs whole sums", relerr(m[:2], whole["m"][:2]), GC.SHARD_BAR)]
    assert m[3] == whole["m"][3] == pb["Mmiss"].sum() and m[2] == whole["m"][2]          # the two counts are integers
    _report(f"two shards {method}", vs + _errs(cs, pb, ref, Cg, out[0]["X"], ypg, out[0]["sc"], m))
    steps, starts = cs["passes"] * n, cs["passes"] * 2          # every run call here follows a set_state or stands where the last one ended
    count = {k: grp.sizes.count(k) for k in sorted(set(grp.sizes))}
    assert set(count) == {r * r, r * r + 1, 2 * (r + 1)} and count[r * r] == steps and count[2 * (r + 1)] == steps, count
    assert steps + cs["passes"] <= count[r * r + 1] <= steps + starts, count


def test_series_ring_same_bits():
    """(700, 60, 3) rPSMF through series_ring(16, 3), the chunks fed by run_stream (which uploads the chunk behind a run -- and so
    the first mask row of it, which the look-ahead Gram reads -- before it queues that run): the bits of the resident handle cut
    at the same steps."""
    from rpsmf_amd import _capi as c

    cs = MC.find(700, 3, "rpsmf")
    pb, _ = MC.reference(cs)
    d, n, r, ch = cs["d"], cs["n"], cs["r"], 16
    Y, M = np.ascontiguousarray(pb["Yorig"].T), np.ascontiguousarray(pb["M"].T)
    spans = [(a, min(a + ch, n)) for a in range(0, n, ch)]
    out = []
    for ring in (False, True):
        f = c.DeviceFilter(d, r, robust=True, storage="f64", masked=1, engine="step", nonuniform_R=True)
        try:
            if ring:
                f.series_ring(ch, 3)
            f.set_row_noise(pb["rho"])
            if not ring:
                f.upload_series(Y)
                f.upload_mask(M)
            f.set_state(pb["C0"], pb["V"], pb["P"], pb["Q"], pb["X0"][:, n - 1], rho=1.0, lambda0=MC.LAMBDA0)
            if ring:
                yps = [yp for _, _, yp in f.run_stream(((Y[a:b], M[a:b]) for a, b in spans), y_pred_dtype=np.float64)]
            else:
                yps = []
                for a, b in spans:
                    f.run(a, b)
                    yps.append(f.y_pred(a, b - a))
            s = f.get_state()
            assert s["k"] == n and f.geometry()["filter_kernel"] == "psmf_sweep_solve"
            out.append(dict(C=s["C"], V=s["V"], P=s["P"], mu=s["mu"], rho=s["rho"], yp=np.concatenate(yps)))
        finally:
            f.close()
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k


@pytest.mark.parametrize("method", ["psmf", "rpsmf", "mle_smf"])
def test_equal_entries_agree_with_the_uniform_handle(method):
    """rho_rows all equal to 10 with rho = 1 against the uniform masked handle with rho = 10: other kernels, another order of the
    sums, the same filter -- within SHARD_BAR."""
    from rpsmf_amd import _capi as c

    cs = MC.find(700, 3, method)
    pb, _ = MC.reference(cs)
    with netlib.env({"PSMF_STEP_PERSISTENT": "0"}):          # the uniform handle on the launched form too: the same sweep and serial stage
        uni = run_handle(c, cs, pb, rho_rows=None, rho=10.0)
    row = run_handle(c, cs, pb, rho_rows=np.full(cs["d"], 10.0), rho=1.0)
    errs = [(k, relerr(row["s"][k], uni["s"][k]), GC.SHARD_BAR) for k in ("C", "P")] + [(k, relerr(row[k], uni[k]), GC.SHARD_BAR) for k in ("X", "yp", "sc")]
    errs.append(("sums", relerr(row["m"][:2], uni["m"][:2]), GC.SHARD_BAR))
    assert row["m"][2] == uni["m"][2] and row["m"][3] == uni["m"][3]
    _report(f"equal entries {method}", errs)


def test_graph_capture_and_tail_reduce_variants():
    """A run longer than the graph chunk of 256 steps: the captured graph (the extra Gram in front of every sweep included) gives
    the bits of the eager launches.  PSMF_TAIL_REDUCE=0 / 1 (who sums the sweep's partial rows, now 2 (r + 1) wide): the same
    filter in another order of the sums -- within SHARD_BAR of each other."""
    from rpsmf_amd import _capi as c

    d, r, n = 64, 6, 300
    rng = np.random.default_rng(31)
    Y = np.cumsum(0.3 * rng.standard_normal((n, d)), axis=0) + 3.0 * rng.random(d)
    M = (rng.random((n, d)) > 0.4).astype(np.uint8)
    rho, C0 = 10.0 * 100.0 ** (rng.random(d) - 0.5), rng.random((d, r))
    out = []
    for use_graph in (False, True):
        f = c.DeviceFilter(d, r, robust=True, storage="f64", masked=1, engine="step", nonuniform_R=True, use_graph=use_graph)
        try:
            f.upload_series(Y)
            f.upload_mask(M)
            f.set_row_noise(rho)
            f.set_state(C0, 2 * np.eye(r), np.eye(r), 0.1 * np.eye(r), np.full(r, 0.3), rho=1.0, lambda0=MC.LAMBDA0)
            f.run(0, n)
            assert f.geometry()["graph_chunk"] == (256 if use_graph else 0)
            s = f.get_state()
            out.append(dict(C=s["C"], V=s["V"], P=s["P"], X=f.mu_history(1, n), yp=f.y_pred(0, n), sc=f.step_scalars(0, n)))
        finally:
            f.close()
    for k in out[0]:
        assert np.all(np.isfinite(out[0][k])) and np.array_equal(out[0][k], out[1][k]), k
    cs = MC.find(700, 3, "rpsmf")
    pb, ref = MC.reference(cs)
    got = []
    for v in ("0", "1"):
        with netlib.env({"PSMF_TAIL_REDUCE": v}):
            got.append(run_handle(c, cs, pb))
    errs = [(k, relerr(got[1]["s"][k], got[0]["s"][k]), GC.SHARD_BAR) for k in ("C", "V", "P")] + [(k, relerr(got[1][k], got[0][k]), GC.SHARD_BAR) for k in ("X", "yp", "sc")]
    for v, g in zip("01", got):
        errs += [(f"tail={v} {k}", e, b) for k, e, b in _errs(cs, pb, ref, g["s"]["C"], g["X"], g["yp"], g["sc"], g["m"])]
    _report("PSMF_TAIL_REDUCE 1 against 0", errs)


def test_refusals_by_message():
    """TMF with a row noise, a rotation on a masked handle, a run before psmf_set_row_noise, and the vector-unit Gram switch (it has
    no masked form): each refused by its message."""
    from rpsmf_amd import _capi as c

    d, r, T = 40, 5, 6
    rng = np.random.default_rng(4)
    with pytest.raises(ValueError, match=r"TMF\) ignores R"):
        c.DeviceFilter(d, r, storage="f64", masked=3, nonuniform_R=True, engine="step")
    with netlib.env({"PSMF_WGRAM_MFMA": "0"}):
        with pytest.raises(ValueError, match="PSMF_WGRAM_MFMA=0.*no masked form"):
            c.DeviceFilter(d, r, storage="f64", masked=1, nonuniform_R=True, engine="step")
        c.DeviceFilter(d, r, storage="f64", nonuniform_R=True, engine="step").close()          # the unmasked twin exists
    f = c.DeviceFilter(d, r, storage="f64", masked=1, nonuniform_R=True, engine="step")
    try:
        with pytest.raises(c.PsmfError, match="psmf_set_noise_rotation: not on a masked handle"):
            f.set_noise_rotation(np.eye(d), np.ones(d))
        f.upload_series(rng.standard_normal((T, d)))
        f.upload_mask(np.ones((T, d)))
        f.set_state(rng.random((d, r)), np.eye(r), np.eye(r), 0.1 * np.eye(r), np.zeros(r), rho=1.0)
        with pytest.raises(c.PsmfError, match="psmf_set_row_noise first"):
            f.run(0, T)
        f.set_row_noise(np.linspace(0.5, 2.0, d))
        f.run(0, T)
        assert f.get_state()["k"] == T
    finally:
        f.close()


def uniform_parent_runs(c):
    """The runs whose bits tests/golden/masked_uniform_parent.npz pins: (40, 90, 24) PSMF, float64, R = 10 I on a uniform masked
    handle -- on its default route and on the launched form (PSMF_STEP_PERSISTENT=0), whose look-ahead masked Gram is the kernel
    that now also serves the row-noise handles."""
    cs = MC.find(40, 24, "psmf")
    pb = MC.problem(cs)
    out = {}
    for name, env in (("default", {}), ("launched", {"PSMF_STEP_PERSISTENT": "0"})):
        with netlib.env(env):
            d, n, r = cs["d"], cs["n"], cs["r"]
            f = c.DeviceFilter(d, r, storage="f64", masked=True, engine="step")
            try:
                f.upload_series(np.ascontiguousarray(pb["Yorig"].T))
                f.upload_mask(np.ascontiguousarray(pb["M"].T))
                f.set_state(pb["C0"], pb["V"], pb["P"], pb["Q"], pb["X0"][:, n - 1], rho=10.0)
                for _ in range(2):
                    f.run(0, n // 2)
                    f.run(n // 2, n)
                out["kernel_" + name] = np.array(f.geometry()["filter_kernel"])
                out["C_" + name], out["X_" + name] = f.get_state()["C"], f.mu_history(1, n)
            finally:
                f.close()
    return out


def test_uniform_masked_handle_keeps_its_bits():
    """nonuniform_R = False: the same bits as before the count slot of the masked Gram learnt to carry sum m_i rho_i."""
    from rpsmf_amd import _capi as c

    want = np.load(GOLDEN)
    got = uniform_parent_runs(c)
    assert str(got["kernel_launched"]) == "psmf_sweep_solve" and set(want.files) == set(got)
    for k in want.files:
        assert np.array_equal(got[k], want[k]), k
    assert np.all(np.isfinite(want["C_launched"])) and np.all(np.isfinite(want["X_launched"]))
