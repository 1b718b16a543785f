"""The masked, batched one-workgroup engine (psmf_impute_run / psmf_impute_run_rows) on configurations drawn at random (seeded,
tests/impute_cases.py): all twelve kernels -- psmf_impute_kernel3<3|5|8|12|20>, their row-noise twins, psmf_impute_kernel2 and
psmf_impute_kernel2w -- with every method they take, dense V0 / P0, a general Q, one to three passes, band factors and lambda0
other than the experiments' constants, series from n = 2 to n = 300, the row edges of both column loops, r = 15 / 16, noise
vectors with a single differing entry, and batches of DIFFERENT replicas (own mask, C0, X0), each replica against its own run of
the float64 oracle.  The engine's hand-picked tests hold almost all of these at one value (V = 2 I, P = I, two passes, sig = 2,
lambda0 = 1.8, n <= 150, copies of one replica); this is the net under it.
GPU only: `pytest -m gpu`; `-s` shows the error figures of every case (each prints before it asserts) and, at the end, the worst
error / bar per (kernel instance, method).

Bars (impute_cases.bar, the ones the suite already holds this engine to on random draws): C, X, Yrec, YrecL, YrecH 1e-9 for PSMF
on the kernel3 instances with r < d; 1e-8 for MLE-SMF, TMF and anything on kernel2 / kernel2w; 1e-7 for rPSMF or r >= d.  Epred,
Efull 1e-8; coverage exact (1e-12).  tests/test_impute_cases_cpu.py has shown that the oracle's own response to a last-bit change
of the inputs sits 16 x inside them for every case, and that no held-out entry is near enough to a band edge to flip the count.
Every third case runs a second time without bands: the same bits in Epred, Efull, inside, C, X and status.
Reference: ExperimentImpute/PSMF.py:40-95, rPSMF.py:40-148, MLESMF.py:40-92, TMF.py:30-73, common.py:79-94."""

import ctypes as C

import numpy as np
import pytest

import impute_cases as IC
import netlib
from conftest import relerr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

WORST = {}          # (instance, method) -> (error / bar, quantity, case)


@pytest.mark.parametrize("i", range(IC.N_CASES))
def test_impute_engine_random_configuration(i):
    from rpsmf_amd import impute

    cs = IC.device_case(i)
    pb = IC.problem(cs)
    ref = IC.oracle(cs, pb)
    banded = cs["method"] in IC.BAND_METHODS
    run = lambda bands: impute.impute_batch(pb["Yorig"], pb["M"], pb["Mmiss"], pb["C0"], pb["X0"], pb["V"], pb["Q"], pb["R"], pb["P"],
                                            cs["sig"], cs["n_iter"], lambda0=cs["lambda0"], method=cs["method"], want_bands=bands)
    with netlib.env(cs["env"]):
        res = run(True)
        res2 = run(False) if i % 3 == 0 else None
    tol = IC.bar(cs)
    errs = []          # (quantity, replica, error, bound)
    for b, want in enumerate(ref):
        errs.append(("Epred", b, relerr(res["Epred"][b], want["Epred"]), IC.ERR_BAR))
        errs.append(("Efull", b, relerr(res["Efull"][b], want["Efull"]), IC.ERR_BAR))
        if banded:
            errs.append(("inside", b, abs(float(res["inside"][b]) - want["inside"]), IC.INSIDE_BAR))
        for k in IC.OUTPUTS:
            if k in want:
                errs.append((k, b, relerr(res[k][b], want[k]) if np.all(np.isfinite(res[k][b])) else np.inf, tol))
    worst = netlib.verdict(errs)
    print(f"\nNET case={i} kernel={res['kernel']} method={cs['method']} d={cs['d']} r={cs['r']} n={cs['n']} passes={cs['n_iter']} batch={cs['batch']} "
          f"sig={cs['sig']} lambda0={cs['lambda0']} Q={'general' if cs['general_Q'] else 'qI'} V,P={'dense' if cs['dense'] else 'diagonal'} "
          f"R={cs['R_kind']} observed={cs['frac']} env={cs['env']} bar={tol:.0e} worst={worst[0]}@{worst[1]} err={worst[2]:.3e} "
          f"ratio={worst[2] / worst[3]:.3g}")
    key = (cs["instance"], cs["method"])
    if key not in WORST or not worst[2] / worst[3] <= WORST[key][0]:
        WORST[key] = (worst[2] / worst[3], worst[0], i)
    assert res["kernel"] == IC.expected_kernel(cs) == cs["instance"], (res["kernel"], cs)
    assert np.all(res["status"] == 0), res["status"]
    netlib.assert_within(errs, cs)
    if res2 is not None:
        assert res2["kernel"] == res["kernel"] and "Yrec" not in res2
        for k in ("Epred", "Efull", "inside", "C", "X", "status"):
            assert np.array_equal(res[k], res2[k], equal_nan=True), ("want_bands changes", k)


@pytest.mark.parametrize("batched", [False, True], ids=["one replica", "batch"])
def test_rank_one_call_leaves_the_callers_X0_alone(batched):
    """What the net found (its cases with r = 1 that ran twice): impute_batch handed the device the caller's own X0 at r = 1 -- the
    transposed (batch, n, 1) view already counts as C-contiguous, so np.ascontiguousarray made no copy -- and the final X
    overwrote it: a second call on the same arguments then started from the first call's answer.  Smallest shape: d = 2, r = 1,
    n = 2.  The caller's arrays are inputs (only the drop-in functions update X, as the reference does: PSMF.py:74)."""
    from rpsmf_amd import impute

    d, r, n = 2, 1, 2
    rng = np.random.default_rng(11)
    Yorig, M = rng.standard_normal((d, n)), np.array([[1, 0], [1, 1]])
    Mmiss, C0, X0 = 1.0 - M, rng.random((d, r)), rng.random((r, n))
    if batched:
        M, Mmiss, C0, X0 = (np.stack([a, a]) for a in (M, Mmiss, C0, X0))
    kept = [a.copy() for a in (Yorig, M, Mmiss, C0, X0)]
    run = lambda: impute.impute_batch(Yorig, M, Mmiss, C0, X0, 2 * np.eye(r), 0.1 * np.eye(r), 10.0, np.eye(r), 2, 1)
    a = run()
    for now, then in zip((Yorig, M, Mmiss, C0, X0), kept):
        assert np.array_equal(now, then)
    M1, Mm1, C1, X1 = (a_[0] if batched else a_ for a_ in kept[1:])
    assert not np.shares_memory(a["X"], X0) and not np.array_equal(a["X"][0], X1)
    b = run()
    for k in ("Epred", "Efull", "C", "X"):
        assert np.array_equal(a[k], b[k]), k
    ep, ef, _, st = IC.impute_filter(Yorig * M1, C1, X1.copy(), M1, Mm1, 2 * np.eye(r), 0.1 * np.eye(r), 10.0, np.eye(r), 2, 1, Yorig, 0.0,
                                     return_state=True)
    assert relerr(b["X"][0], st["X"]) < 1e-9 and relerr(b["C"][0], st["C"]) < 1e-9 and relerr(b["Efull"][0], ef[0, 1:]) < 1e-8


def test_worst_error_over_bar_per_instance_and_method():
    """The table of the net: worst error / bar over every compared quantity per (kernel instance, method), over the cases that
    ran before this test (all of them in a whole-file run)."""
    print("\nworst error / bar per (kernel instance, method):")
    for (instance, method), (ratio, what, i) in sorted(WORST.items(), key=lambda kv: IC.TARGETS.index(kv[0])):
        print(f"WORST {instance:28s} {method:8s} ratio={ratio:.3g} ({what}, case {i})")
    assert all(ratio < 1.0 for ratio, _, _ in WORST.values())


# ---- what the C ABI refuses: PSMF_ERR_ARG, a message, nothing launched (every output buffer as it was)
def _refusals():
    bad = lambda **kw: kw
    return [("n = 1", bad(n=1), "bad n"), ("n_iter = 0", bad(n_iter=0), "n_iter"), ("batch = 0", bad(batch=0), "batch"),
            ("method = 4", bad(method=4), "method"), ("want_bands without band buffers", bad(want_bands=1), "want_bands"),
            ("r = 65", bad(r=65), "PSMF_RMAX"), ("device ordinal = device count", bad(device="count"), "device ordinal"),
            ("negative noise entry", bad(rows=-1.0), "finite and >= 0"), ("NaN noise entry", bad(rows=float("nan")), "finite and >= 0")]


@pytest.mark.parametrize("what,change,word", _refusals(), ids=[w for w, _, _ in _refusals()])
def test_c_abi_refusals(what, change, word):
    from rpsmf_amd import _capi

    lib = _capi.load_library()
    d, n, r, B = 19, 6, 4, 2
    f = dict(d=d, n=n, r=r, batch=B, method=0, n_iter=2, device=0, want_bands=0)
    change = dict(change)
    rows = change.pop("rows", None)
    f.update(change)
    if f["device"] == "count":
        f["device"] = _capi.device_count()
        assert f["device"] >= 1
    rr, nn, BB = max(f["r"], r), max(f["n"], n), max(f["batch"], B)          # buffers large enough for whatever the call names
    cfg = _capi.PsmfImputeConfig(abi_version=_capi.ABI_VERSION, sig=2.0, lambda0=1.8, **f)
    rng = np.random.default_rng(3)
    Y, Mk = rng.standard_normal((nn, d)), np.ones((BB, nn, d), dtype=np.uint8)
    Cm, X, E = rng.random((BB, d, rr)), rng.random((BB, nn, rr)), np.eye(rr)
    ep, ef, ins = np.full((BB, 2), -7.0), np.full((BB, 2), -7.0), np.full(BB, -7.0)
    status = np.full(BB, 77, dtype=np.int32)
    ms = C.c_float(-1.0)
    before = [a.copy() for a in (Cm, X, ep, ef, ins, status)]
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    if rows is None:
        run, noise = lib.psmf_impute_run, 10.0
    else:
        vec = np.linspace(1.0, 2.0, d)
        vec[d - 1] = rows
        run, noise = lib.psmf_impute_run_rows, dp(vec)
    rc = run(C.byref(cfg), dp(Y), up(Mk), up(Mk), dp(Cm), dp(X), dp(E), dp(E), dp(E), noise, dp(ep), dp(ef), dp(ins), None, None, None,
             status.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(ms))
    msg = lib.psmf_last_error(None).decode()
    print(f"\n{what}: rc = {rc}, {msg!r}")
    assert rc == _capi.ERR_ARG, (what, rc, msg)
    assert msg.startswith("psmf_impute_run_rows: " if rows is not None else "psmf_impute_run: ") and word in msg, (what, msg)
    for a, b in zip((Cm, X, ep, ef, ins, status), before):
        assert np.array_equal(a, b), what
    assert ms.value == -1.0
