"""psmf_ssm_run / rpsmf_amd.ssm on the device: the batched PSMF with linear-Gaussian dynamics and an observation map
(rpsmf_amd/csrc/psmf_ssm.hip) against the line-for-line model of ExperimentChange/PSMF.m:6-45 (tests/ssm_cases.py: literal_model).

The bar is 5e-9 in conftest.relerr, the suite's float64 bar for the one-workgroup engines; tests/test_ssm_cases_cpu.py shows that
every case is conditioned 500 x below it and that carry_P and H both move X by more than 1e-2.  Every case runs as a batch of three
replicas (different seeds for Y, C0, x0), once per module; the other tests share those runs."""

from functools import lru_cache

import numpy as np
import pytest

import ssm_cases as SC
from conftest import relerr

pytestmark = pytest.mark.gpu

BAR = 5e-9
SEEDS = (0, 1, 2)
ERR_NUMERIC = -4


def _call(pbs, **kw):
    from rpsmf_amd.ssm import linear_psmf_batch

    pb = pbs[0]
    return linear_psmf_batch(np.stack([q["Y"] for q in pbs]), np.stack([q["C0"] for q in pbs]), np.stack([q["x0"] for q in pbs]),
                             pb["V"], pb["P0"], pb["A"], pb["Q"], pb["H"], pb["rho"], **kw)


@lru_cache(maxsize=None)
def _device(i):
    cs = SC.CASES[i]
    return _call([SC.reference(cs, seed=s)[0] for s in SEEDS], carry_P=bool(cs["carry_P"]), want_pred=True)


def _errors(res, b, ref):
    return {k: relerr(res[k][b], ref[k]) for k in SC.COMPARED}


def _same_bits(a, b, keys=SC.COMPARED):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


@pytest.mark.parametrize("cs", SC.CASES, ids=SC.IDS)
def test_every_case_against_the_literal_model(cs):
    res = _device(SC.CASES.index(cs))
    assert list(res["status"]) == [0, 0, 0]
    assert res["X"].shape == (3, cs["p"], cs["n"]) and res["Ypred"].shape == (3, cs["d"], cs["n"]) and res["scalars"].shape == (3, cs["n"], 2)
    worst = {}
    for b, seed in enumerate(SEEDS):
        err = _errors(res, b, SC.reference(cs, seed=seed)[1])
        print(f"\nssm {SC.IDS[SC.CASES.index(cs)]} replica {b}: {err}")
        worst = {k: max(worst.get(k, 0.0), v) for k, v in err.items()}
    assert max(worst.values()) <= BAR, worst


@pytest.mark.parametrize("cs", SC.CASES, ids=SC.IDS)
def test_a_replica_run_alone_and_a_second_run_give_the_same_bits(cs):
    res = _device(SC.CASES.index(cs))
    alone = _call([SC.reference(cs, seed=SEEDS[1])[0]], carry_P=bool(cs["carry_P"]), want_pred=True)
    assert alone["status"][0] == 0
    assert all(np.array_equal(alone[k][0], res[k][1]) for k in SC.COMPARED), "replica 1 alone differs from replica 1 of the batch"
    again = _call([SC.reference(cs, seed=s)[0] for s in SEEDS], carry_P=bool(cs["carry_P"]), want_pred=True)
    assert _same_bits(again, res), "the same call twice gives different bits"


def test_more_workgroups_than_compute_units():
    cs = SC.find(5, 2, "matern", 1)
    B = 300
    pbs = [SC.problem(cs, seed=s) for s in range(B)]
    res = _call(pbs, carry_P=True, want_pred=True)
    assert res["status"].shape == (B,) and not res["status"].any()
    for b in (0, 150, 299):
        err = _errors(res, b, SC.literal_model(pbs[b], 1))
        print(f"\nssm batch of {B}, replica {b}: {err}")
        assert max(err.values()) <= BAR, (b, err)


@pytest.mark.parametrize("carry_P", [1, 0])
@pytest.mark.parametrize("shape", [(20, 10, "matern"), (33, 7, "dense")])
def test_two_calls_continue_a_series(shape, carry_P):
    from rpsmf_amd.ssm import linear_psmf_batch

    cs = SC.find(shape[0], shape[1], shape[2], carry_P)
    res = _device(SC.CASES.index(cs))
    pbs = [SC.reference(cs, seed=s)[0] for s in SEEDS]
    pb, n1 = pbs[0], cs["n"] // 3 + 1
    Y = np.stack([q["Y"] for q in pbs])
    a = linear_psmf_batch(Y[:, :, :n1], np.stack([q["C0"] for q in pbs]), np.stack([q["x0"] for q in pbs]), pb["V"], pb["P0"],
                          pb["A"], pb["Q"], pb["H"], pb["rho"], carry_P=bool(carry_P), want_pred=True)
    b = linear_psmf_batch(Y[:, :, n1:], a["C"], a["x"], a["V"], a["P"], pb["A"], pb["Q"], pb["H"], pb["rho"], carry_P=bool(carry_P),
                          first_step=False, want_pred=True)
    two = dict(X=np.concatenate([a["X"], b["X"]], axis=2), Ypred=np.concatenate([a["Ypred"], b["Ypred"]], axis=2),
               scalars=np.concatenate([a["scalars"], b["scalars"]], axis=1), C=b["C"], V=b["V"], P=b["P"], x=b["x"])
    err = {k: relerr(two[k], res[k]) for k in SC.COMPARED}
    print(f"\nssm continuation {shape} carry_P={carry_P}: n = {n1} + {cs['n'] - n1}, bits equal: {_same_bits(two, res)}, {err}")
    assert max(err.values()) <= 1e-12, err


def test_a_replica_with_a_nan_fails_alone():
    cs = SC.find(20, 10, "matern", 1)
    res = _device(SC.CASES.index(cs))
    pbs = [dict(SC.reference(cs, seed=s)[0]) for s in SEEDS]
    Y = pbs[1]["Y"].copy()
    Y[3, 17] = np.nan
    pbs[1]["Y"] = Y
    out = _call(pbs, carry_P=True, want_pred=True)
    assert list(out["status"]) == [0, ERR_NUMERIC, 0]
    for b in (0, 2):
        assert all(np.array_equal(out[k][b], res[k][b]) for k in SC.COMPARED), f"replica {b} was touched by its neighbour's failure"
    with pytest.raises(np.linalg.LinAlgError, match="replica 1"):
        _call(pbs, carry_P=True, status=None)


def test_refusals_by_message():
    from rpsmf_amd.ssm import PSMF, linear_psmf_batch

    def run(d, r, p, Q=None):
        return linear_psmf_batch(np.zeros((d, 6)), np.ones((d, r)), np.zeros(p), np.eye(r), np.eye(p), np.eye(p),
                                 np.eye(p) if Q is None else Q, np.ones((r, p)), 0.5)

    with pytest.raises(ValueError, match="d <= 512"):
        run(513, 2, 4)
    with pytest.raises(ValueError, match="r <= 16"):
        run(8, 17, 20)
    with pytest.raises(ValueError, match="p <= 32"):
        run(8, 4, 33)
    with pytest.raises(ValueError, match="p >= r"):
        run(8, 4, 3)
    Q = np.eye(4)
    Q[0, 1] = 0.1
    with pytest.raises(ValueError, match="Q must be symmetric"):
        run(8, 2, 4, Q)
    R = 0.1 * np.eye(8)
    R[0, 1] = 0.01
    with pytest.raises(NotImplementedError, match="rho \\* I"):
        PSMF(2, np.zeros((8, 6)), np.eye(4), np.eye(4), R, np.ones((2, 4)), np.eye(2), np.eye(4), np.ones((8, 2)), None, 8, 6, x0=np.zeros(4))


def test_the_drop_in_is_the_batch_entry_point_with_carry_P_off():
    from rpsmf_amd.ssm import PSMF

    cs = SC.find(20, 10, "matern", 0)
    pb, ref = SC.reference(cs, seed=0)
    res = _device(SC.CASES.index(cs))
    d, n, r = cs["d"], cs["n"], cs["r"]
    X = PSMF(r, pb["Y"], pb["Q"], pb["A"], pb["rho"] * np.eye(d), pb["H"], pb["V"], pb["P0"], pb["C0"], np.zeros((cs["p"], n)), d, n, x0=pb["x0"])
    assert X.shape == (cs["p"], n)
    assert np.array_equal(X, res["X"][0]), "PSMF(...) and linear_psmf_batch(carry_P=False) give different bits"
    err = relerr(X, ref["X"])
    print(f"\nssm drop-in against the literal model: {err}")
    assert err <= BAR
