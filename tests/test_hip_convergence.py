"""psmf_conv_run / rpsmf_amd.convergence on the device: the convergence experiment (rpsmf_amd/csrc/psmf_conv.hip).

Known answers: the reference's stored run (tests/golden/convergence_expdata.npz) -- its Kalman path, and iteration 10001 from its final
state, which the stored iteration-to-iteration drift bounds (tests/test_conv_cases_cpu.py).  The net of tests/conv_cases.py, every one of
the twelve (r, capacity) instances, against the extended-precision model at BAR = 1e-9 relative (avW, CerrI, ErM of every iteration,
C, Xps, Pps, Cerr; W per step as |W^2 - W^2_ref| <= 1e-9 (|dm|^2 + tr S1 + tr S2), the quantity that is well conditioned).  Same bits:
one call of 2 k iterations and two of k; 1, 2 and the default number of iterations per launch (PSMF_CONV_ITERS); chunks of 1 and 65
replicas and the default (PSMF_CONV_CHUNK); shared data and the same data given per replica.  Status: a replica with a NaN in its C0.
And iteration 1 beside linear_psmf_batch (A = I, H = I, carry_P), the one other device route to a sweep.

Worst error as a share of its bar (error / 1e-9), per instance, measured on the MI355X (test_worst_ratio_per_instance prints it;
profiles/conv_gpu_tests.txt, docs/MEASUREMENTS.md):

    r    capacity 4       capacity 8       capacity 16
    1    6.9e-5 (ErM)     1.5e-5 (Pk)      8.8e-5 (Pk)
    2    3.5e-4 (ErM)     1.8e-5 (ErM)     4.4e-5 (ErM)
    3    4.6e-5 (ErM)     4.3e-5 (W^2)     8.5e-5 (ErM)
    4    2.1e-4 (C)       3.0e-4 (ErM)     5.4e-5 (ErM)"""

import os
from functools import lru_cache

import numpy as np
import pytest

import conv_cases as CC
from conftest import ROOT
from netlib import env, relerr

pytestmark = pytest.mark.gpu

assert np.finfo(np.longdouble).eps < 1.1e-19, "these tests need an 80-bit long double: the extended model is no reference without it"

GOLDEN = os.path.join(ROOT, "tests", "golden", "convergence_expdata.npz")
AVW, CERRI, ERM = 0.08244964400063459, 0.6336846011233929, 10.31679111693605      # entry 10000 of the stored avW, CerrI, ErM
KEYS = ("avW", "CerrI", "ErM", "C", "Xps", "Pps", "Cerr", "Xk", "Pk")
OUT_KEYS = ("avW", "CerrI", "ErM", "Xk", "Pk", "Xps", "Pps", "W", "Cerr", "C", "x0", "P0")


def run(cs, n_iter=None, start=None, want_moments=True, status=True, switches=None, per_replica=False, C0=None):
    """one call for the case; start = (C, x0, P0) of a call to continue; per_replica: shared data given to every replica"""
    from rpsmf_amd import convergence_batch

    Cs, xs, Ps = start or (cs["C0"] if C0 is None else C0, cs["x0"], cs["P0"])
    Y, Ct, xk, Pk = cs["Y"], cs["Ctrue"], cs["x0k"], cs["P0k"]
    if per_replica:
        assert not cs["own"]
        Y, Ct, xk, Pk = (np.broadcast_to(a, (cs["B"],) + a.shape) for a in (Y, Ct, xk, Pk))
    with env(switches or {}):
        return convergence_batch(Y, Ct, Cs, xs, Ps, Q=cs["Q"], R=cs["Rdiag"], v=cs["v"], q_scale=cs["q_scale"], r_scale=cs["r_scale"],
                                 n_iter=n_iter or cs["n_iter"], x0_kalman=xk, P0_kalman=Pk, want_moments=want_moments, status=status)


def same_bits(a, b, what, keys=OUT_KEYS):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if a["Xk"].ndim != b["Xk"].ndim and k in ("Xk", "Pk"):      # shared against per replica: one path against a batch of it
            x, y = np.broadcast_arrays(x, y)
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), f"{what}: {k} differs"


# ---- known answers
def stored_case():
    g = dict(np.load(GOLDEN))
    cs = dict(r=1, d=4, n=1000, n_iter=1, B=1, own=False, Y=g["Y"], Ctrue=g["Ctrue"], Q=g["Q"], Rdiag=g["Rdiag"], x0k=g["X0k"][:, 0], P0k=g["P0k"],
              C0=g["C"][None], x0=g["Xps"][None, :, 0], P0=g["Pps"][None, :, :, 0], v=np.ones(1), q_scale=np.ones(1), r_scale=np.ones(1))
    return g, cs


def test_the_kalman_pass_and_iteration_10001_of_the_stored_run():
    g, cs = stored_case()
    res = run(cs, want_moments=False)
    assert res["status"][0] == 0
    ex, ep = np.max(np.abs(res["Xk"] - g["Xk"])), np.max(np.abs(res["Pk"] - g["Pk"]))
    print(f"\nKalman pass against the stored path: Xk {ex:.2e}, Pk {ep:.2e}")
    assert ex < 2e-12 and ep < 2e-12
    m = CC.model(cs)
    errs = {k: relerr(res[k], m[k]) for k in ("avW", "CerrI", "ErM", "C", "Xps", "Pps", "Cerr", "W")}
    print("iteration 10001 against the float64 model:", {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) <= CC.BAR, errs
    away = dict(avW=abs(res["avW"][0, 0] - AVW), CerrI=abs(res["CerrI"][0, 0] - CERRI), ErM=abs(res["ErM"][0, 0] - ERM),
                Xps=np.max(np.abs(res["Xps"][0] - g["Xps"])), C=np.max(np.abs(res["C"][0] - g["C"])))
    print("iteration 10001 against the stored values:", {k: f"{v:.2e}" for k, v in away.items()})
    # ten times the stored iteration-to-iteration drift: the drift of one further iteration dwarfs rounding
    assert away["avW"] < 1.1e-12 and away["CerrI"] < 9e-12 and away["ErM"] < 4e-14 and away["Xps"] < 6e-12 and away["C"] < 1.3e-11, away


# ---- the net
@lru_cache(maxsize=None)
def _net(i):
    """((quantity, error / bar) worst first, the device's result) of case i: one call"""
    cs = CC.device_case(i)
    ref = cs["ref"]
    res = run(cs)
    assert res["status"].shape == (cs["B"],) and not res["status"].any(), (i, res["status"])
    ratios = {k: relerr(res[k], ref[k] if cs["own"] or k not in ("Xk", "Pk") else ref[k][0]) / CC.BAR for k in KEYS}
    w2 = np.abs(res["W"] ** 2 - np.maximum(ref["W2"], 0.0))
    scale = np.where(ref["W2scale"] > 0, ref["W2scale"], 1.0)       # (step 1 has no distance: W = 0 on both sides)
    ratios["W2"] = float(np.max(w2 / scale)) / CC.BAR
    assert np.all(res["W"][:, 0] == 0.0)
    return sorted(ratios.items(), key=lambda kv: -kv[1] if np.isfinite(kv[1]) else -np.inf), res


@pytest.mark.parametrize("i", range(len(CC.SPECS)))
def test_every_case_against_the_extended_model(i):
    ratios, _ = _net(i)
    print(f"\nconv case {i} {CC.describe(CC.device_case(i))}: worst error / bar " + ", ".join(f"{k} {v:.1e}" for k, v in ratios[:4]))
    assert all(v <= 1.0 for _, v in ratios), ratios      # (`<=`: a NaN fails)


def test_worst_ratio_per_instance():
    """the summary of the net: per (r, capacity) instance, the worst error as a share of its bar"""
    table = {}
    for i in range(len(CC.SPECS)):
        key, (quantity, ratio) = CC.instance(CC.device_case(i)), _net(i)[0][0]
        if key not in table or not ratio <= table[key][1]:
            table[key] = (quantity, ratio, i)
    assert len(table) == 12
    print()
    for (r, cap), worst in sorted(table.items()):
        print(f"conv instance r = {r}, capacity {cap}: worst error / bar {worst[1]:.2e} ({worst[0]}, case {worst[2]})")


def test_without_moments_only_the_last_ErM_is_formed():
    cs = CC.device_case(9)
    full, res = _net(9)[1], run(cs, want_moments=False)
    assert np.all(np.isnan(res["ErM"][:, :-1])) and relerr(res["ErM"][:, -1], full["ErM"][:, -1]) <= CC.BAR      # (||Y - C Xps|| as it stands against the sums)
    same_bits(res, full, "want_moments off against on", keys=[k for k in OUT_KEYS if k != "ErM"])
    assert relerr(res["ErM"][:, -1], cs["ref"]["ErM"][:, -1]) <= CC.BAR


# ---- same bits
@pytest.mark.parametrize("i", [1, 14, 21])
def test_two_calls_of_k_iterations_are_one_call_of_2k(i):
    cs = CC.device_case(i)
    k = cs["n_iter"] // 2
    whole = run(cs, n_iter=2 * k)
    first = run(cs, n_iter=k)
    second = run(cs, n_iter=k, start=(first["C"], first["x0"], first["P0"]))
    for key in ("avW", "CerrI", "ErM"):
        assert np.array_equal(np.concatenate([first[key], second[key]], axis=1), whole[key]), key
    same_bits(second, whole, "k + k against 2 k", keys=[k_ for k_ in OUT_KEYS if k_ not in ("avW", "CerrI", "ErM")])
    fresh = CC.draw(i, CC.REPLACED.get(i, 0))
    assert all(np.array_equal(cs[key], fresh[key]) for key in ("Y", "Ctrue", "C0", "x0", "P0", "x0k", "P0k", "v")), "no argument is modified"


@pytest.mark.parametrize("i", [1, 14, 19])
@pytest.mark.parametrize("iters", ["1", "2"])
def test_iterations_per_launch_change_no_bit(i, iters):
    """PSMF_CONV_ITERS (read at every call): the state crosses launches as float64"""
    same_bits(run(CC.device_case(i), switches={"PSMF_CONV_ITERS": iters}), _net(i)[1], f"PSMF_CONV_ITERS={iters}")


@pytest.mark.parametrize("i", [7, 14, 22, 23])
@pytest.mark.parametrize("chunk", ["1", "65"])
def test_chunks_of_replicas_change_no_bit(i, chunk):
    """PSMF_CONV_CHUNK (read at every call): 129 or 65 replicas in chunks of 1 and of 65 (the last one partial or empty)"""
    same_bits(run(CC.device_case(i), switches={"PSMF_CONV_CHUNK": chunk}), _net(i)[1], f"PSMF_CONV_CHUNK={chunk}")


@pytest.mark.parametrize("i", [1, 7, 16, 22])
def test_shared_data_given_per_replica_is_the_same_run(i):
    same_bits(run(CC.device_case(i), per_replica=True), _net(i)[1], "own-data instance against shared-data instance")


def test_bad_switches_are_refused():
    for name in ("PSMF_CONV_CHUNK", "PSMF_CONV_ITERS"):
        with pytest.raises(ValueError, match=name):
            run(CC.device_case(0), switches={name: "-1"})


# ---- status
def test_a_replica_with_a_nan_fails_alone():
    cs = CC.device_case(16)                              # 65 replicas: one wave and a lane
    assert cs["B"] == 65
    for bad in (37, 64):
        C0 = cs["C0"].copy()
        C0[bad, 2, 1] = np.nan
        res, clean = run(cs, C0=C0), _net(16)[1]
        want = np.zeros(65, dtype=np.int32)
        want[bad] = -4                                   # PSMF_ERR_NUMERIC
        assert np.array_equal(res["status"], want)
        keep = np.arange(65) != bad
        for k in ("avW", "CerrI", "ErM", "Xps", "Pps", "W", "Cerr", "C", "x0", "P0"):
            assert np.array_equal(res[k][keep], clean[k][keep]), (bad, k)
        with pytest.raises(np.linalg.LinAlgError, match=f"replica {bad}"):
            run(cs, C0=C0, status=None)


def test_a_state_that_leaves_the_finite_range_on_the_device_fails_its_replica():
    cs = CC.device_case(6)                               # own data, r = 2: finite inputs, but an x0 whose square overflows
    x0 = cs["x0"].copy()
    x0[5] = 1e200
    res = run(dict(cs, x0=x0))
    want = np.zeros(cs["B"], dtype=np.int32)
    want[5] = -4
    assert np.array_equal(res["status"], want)
    keep = np.arange(cs["B"]) != 5
    assert np.array_equal(res["avW"][keep], _net(6)[1]["avW"][keep]) and np.array_equal(res["C"][keep], _net(6)[1]["C"][keep])


# ---- the parent's only device route to a sweep
def test_iteration_1_beside_linear_psmf_batch():
    """d = 8, r = 4, n = 50, R = rho I, no scaling: iteration 1 is a run of linear_psmf_batch with A = I, H = I, p = r, carry_P.  Both
    against the extended model at the net's bar -- X and the final C from both, the final V from linear_psmf_batch (the experiment has
    no use for V and psmf_conv_run does not return it) -- and their mutual distance, printed."""
    from rpsmf_amd.ssm import linear_psmf_batch

    base = CC.draw(20)
    assert (base["r"], base["d"], base["n"]) == (4, 8, 50) and len(set(base["Rdiag"])) == 1 and not base["own"]
    B = 6
    cs = dict(base, B=B, n_iter=1, C0=base["C0"][:B], x0=base["x0"][:B], P0=base["P0"][:B], v=base["v"][:B], q_scale=np.ones(B), r_scale=np.ones(B))
    ref = CC.model(cs, np.longdouble)
    conv = run(cs, want_moments=False)
    I = np.eye(4)
    ssm = linear_psmf_batch(np.broadcast_to(cs["Y"], (B,) + cs["Y"].shape), cs["C0"], cs["x0"], cs["v"][:, None, None] * I, cs["P0"], I, cs["Q"], I,
                            float(cs["Rdiag"][0]), carry_P=True)
    assert not conv["status"].any() and not ssm["status"].any()
    f = lambda a: np.asarray(a, dtype=np.float64)
    errs = dict(conv_X=relerr(conv["Xps"], f(ref["Xps"])), conv_C=relerr(conv["C"], f(ref["C"])), ssm_X=relerr(ssm["X"], f(ref["Xps"])),
                ssm_C=relerr(ssm["C"], f(ref["C"])), ssm_V=relerr(ssm["V"], f(ref["V"])))
    print("\nagainst the extended model:", {k: f"{v:.1e}" for k, v in errs.items()})
    print(f"psmf_conv_run against psmf_ssm_run: X {relerr(conv['Xps'], ssm['X']):.1e}, C {relerr(conv['C'], ssm['C']):.1e}")
    assert max(errs.values()) <= CC.BAR, errs
