"""psmf_ssm_run_ex / rpsmf_amd.ssm on the device: the robust (rPSMF) and masked forms of the batched PSMF with linear-Gaussian dynamics
and an observation map (rpsmf_amd/csrc/psmf_ssm.hip: psmf_ssm_kernel<robust, masked>) against the line-for-line model
(tests/ssm_robust_cases.py: literal_model).

The bar is 5e-9 in conftest.relerr, the suite's float64 bar for the one-workgroup engines; tests/test_ssm_robust_cases_cpu.py shows
that every case is conditioned 500 x below it and that the robust flag and the mask each move X by more than 1e-2.  Every case runs
as a batch of three replicas (different seeds for Y, C0, x0 and the mask), once per module; the other tests share those runs."""

from functools import lru_cache

import numpy as np
import pytest

import ssm_cases as SC
import ssm_robust_cases as RC
from conftest import relerr

pytestmark = pytest.mark.gpu

BAR = 5e-9
SEEDS = (0, 1, 2)
ERR_NUMERIC = -4


def _kw(cs):
    kw = dict(carry_P=bool(cs["carry_P"]), want_pred=True)
    if cs["robust"]:
        kw.update(robust=True, lambda0=cs["lambda0"], fixed_lambda=cs["fixed_lambda"])
    return kw


def _call(pbs, masked, **kw):
    from rpsmf_amd.ssm import linear_psmf_batch

    pb = pbs[0]
    if masked:
        kw["mask"] = np.stack([q["mask"] for q in pbs])
    return linear_psmf_batch(np.stack([q["Y"] for q in pbs]), np.stack([q["C0"] for q in pbs]), np.stack([q["x0"] for q in pbs]),
                             pb["V"], pb["P0"], pb["A"], pb["Q"], pb["H"], pb["rho"], **kw)


@lru_cache(maxsize=None)
def _device(i):
    cs = RC.CASES[i]
    return _call([RC.reference(cs, seed=s)[0] for s in SEEDS], cs["masked"], **_kw(cs))


def _errors(res, b, ref):
    return {k: relerr(res[k][b], ref[k]) for k in RC.COMPARED}


def _same_bits(a, b, keys=RC.COMPARED):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


@pytest.mark.parametrize("cs", RC.CASES, ids=RC.IDS)
def test_every_case_against_the_literal_model(cs):
    res = _device(RC.CASES.index(cs))
    n = cs["n"]
    assert list(res["status"]) == [0, 0, 0]
    assert res["X"].shape == (3, cs["p"], n) and res["Ypred"].shape == (3, cs["d"], n) and res["scalars"].shape == (3, n, 2)
    assert res["omega"].shape == (3, n) and res["phi"].shape == (3, n) and res["robust_state"].shape == (3, 2)
    worst = {}
    for b, seed in enumerate(SEEDS):
        err = _errors(res, b, RC.reference(cs, seed=seed)[1])
        print(f"\nssm robust {RC.IDS[RC.CASES.index(cs)]} replica {b}: {err}")
        worst = {k: max(worst.get(k, 0.0), v) for k, v in err.items()}
    assert max(worst.values()) <= BAR, worst


@pytest.mark.parametrize("carry_P", [1, 0])
@pytest.mark.parametrize("shape", [(5, 2, "matern"), (33, 7, "dense"), (96, 16, "dense"), (512, 3, "dense")])
def test_not_robust_and_no_mask_through_the_new_entry_point_is_psmf_ssm_run(shape, carry_P):
    """robust=numpy.False_ is enough to leave the old entry point; the bits are its own"""
    cs = SC.find(shape[0], shape[1], shape[2], carry_P)
    pbs = [SC.reference(cs, seed=s)[0] for s in SEEDS]
    old = _call(pbs, False, carry_P=bool(carry_P), want_pred=True)
    new = _call(pbs, False, carry_P=bool(carry_P), want_pred=True, robust=np.False_)
    assert "omega" not in old and old["scalars"].shape == new["scalars"].shape == (3, cs["n"], 2)
    assert _same_bits(old, new, SC.COMPARED)
    assert np.array_equal(new["omega"], np.ones((3, cs["n"]))) and np.array_equal(new["phi"], np.ones((3, cs["n"])))
    assert np.array_equal(new["robust_state"], np.tile([0.0, 1.0], (3, 1)))
    # ... and an all-ones mask on the plain form gives those bits too
    ones = _call([dict(q, mask=np.ones(q["Y"].shape, dtype=np.uint8)) for q in pbs], True, carry_P=bool(carry_P), want_pred=True)
    assert _same_bits(old, ones, SC.COMPARED), "the plain form with an all-ones mask differs from psmf_ssm_run"


@pytest.mark.parametrize("cs", [c for c in RC.CASES if c["variant"] in ("rob", "rob-fix")], ids=lambda c: RC.IDS[RC.CASES.index(c)])
def test_an_all_ones_mask_gives_the_bits_of_no_mask(cs):
    res = _device(RC.CASES.index(cs))
    pbs = [RC.reference(cs, seed=s)[0] for s in SEEDS]
    assert all(q["mask"].all() for q in pbs)
    ones = _call(pbs, True, **_kw(cs))
    assert _same_bits(ones, res), "the robust form with an all-ones mask differs from the robust form without a mask"


@pytest.mark.parametrize("cs", [c for c in RC.CASES if c["masked"]], ids=lambda c: RC.IDS[RC.CASES.index(c)])
def test_nan_under_a_zero_mask_is_never_read(cs):
    res = _device(RC.CASES.index(cs))
    pbs = [RC.reference(cs, seed=s)[0] for s in SEEDS]
    zeros = _call([dict(q, Y=np.where(q["mask"] > 0, q["Y"], 0.0)) for q in pbs], True, **_kw(cs))
    nans = _call([dict(q, Y=np.where(q["mask"] > 0, q["Y"], np.nan)) for q in pbs], True, **_kw(cs))
    assert list(nans["status"]) == [0, 0, 0]
    assert _same_bits(zeros, res) and _same_bits(nans, res)


@pytest.mark.parametrize("cs", RC.CASES, ids=RC.IDS)
def test_a_replica_run_alone_and_a_second_run_give_the_same_bits(cs):
    res = _device(RC.CASES.index(cs))
    alone = _call([RC.reference(cs, seed=SEEDS[1])[0]], cs["masked"], **_kw(cs))
    assert alone["status"][0] == 0
    assert all(np.array_equal(alone[k][0], res[k][1]) for k in RC.COMPARED), "replica 1 alone differs from replica 1 of the batch"
    again = _call([RC.reference(cs, seed=s)[0] for s in SEEDS], cs["masked"], **_kw(cs))
    assert _same_bits(again, res), "the same call twice gives different bits"


def test_one_batch_may_mix_masks():
    """replica 0 all observed, replica 1 the case's mask, replica 2 another: each is what it is alone"""
    for variant in ("mask", "rob-mask"):
        cs = RC.find(33, 7, "dense", 1, variant)
        pbs = [dict(RC.reference(cs, seed=s)[0]) for s in SEEDS]
        pbs[0]["mask"] = np.ones_like(pbs[0]["mask"])
        pbs[2]["mask"] = np.roll(pbs[2]["mask"], 5, axis=0)
        res = _call(pbs, True, **_kw(cs))
        assert list(res["status"]) == [0, 0, 0]
        for b in range(3):
            ref = RC.literal_model(pbs[b], 1, **RC.model_kw(cs))
            err = _errors(res, b, ref)
            print(f"\nssm robust mixed masks, {variant}, replica {b}: {err}")
            assert max(err.values()) <= BAR, (b, err)
        assert all(np.array_equal(res[k][1], _device(RC.CASES.index(cs))[k][1]) for k in RC.COMPARED)


@pytest.mark.parametrize("variant", ["rob-mask", "rob-fix-mask"])
@pytest.mark.parametrize("carry_P", [1, 0])
@pytest.mark.parametrize("shape", [(20, 10, "matern"), (33, 7, "dense")])
def test_two_calls_continue_a_series(shape, carry_P, variant):
    from rpsmf_amd.ssm import linear_psmf_batch

    cs = RC.find(shape[0], shape[1], shape[2], carry_P, variant)
    res = _device(RC.CASES.index(cs))
    pbs = [RC.reference(cs, seed=s)[0] for s in SEEDS]
    pb, n1 = pbs[0], cs["n"] // 3 + 1
    Y, M = np.stack([q["Y"] for q in pbs]), np.stack([q["mask"] for q in pbs])
    kw = _kw(cs)
    a = linear_psmf_batch(Y[:, :, :n1], np.stack([q["C0"] for q in pbs]), np.stack([q["x0"] for q in pbs]), pb["V"], pb["P0"],
                          pb["A"], pb["Q"], pb["H"], pb["rho"], mask=M[:, :, :n1], **kw)
    b = linear_psmf_batch(Y[:, :, n1:], a["C"], a["x"], a["V"], a["P"], pb["A"], pb["Q"], pb["H"], pb["rho"], mask=M[:, :, n1:],
                          first_step=False, robust_state=a["robust_state"], **kw)
    cat = lambda k, ax: np.concatenate([a[k], b[k]], axis=ax)
    two = dict(X=cat("X", 2), Ypred=cat("Ypred", 2), scalars=cat("scalars", 1), omega=cat("omega", 1), phi=cat("phi", 1), C=b["C"], V=b["V"],
               P=b["P"], x=b["x"], robust_state=b["robust_state"])
    err = {k: relerr(two[k], res[k]) for k in RC.COMPARED}
    print(f"\nssm robust continuation {shape} carry_P={carry_P} {variant}: n = {n1} + {cs['n'] - n1}, bits equal: {_same_bits(two, res)}, {err}")
    assert max(err.values()) <= 1e-12, err


def test_more_workgroups_than_compute_units():
    cs = RC.find(5, 2, "matern", 1, "rob-mask")
    B = 300
    pbs = [RC.problem(cs, seed=s) for s in range(B)]
    res = _call(pbs, True, **_kw(cs))
    assert res["status"].shape == (B,) and not res["status"].any()
    for b in (0, 150, 299):
        err = _errors(res, b, RC.literal_model(pbs[b], 1, **RC.model_kw(cs)))
        print(f"\nssm robust batch of {B}, replica {b}: {err}")
        assert max(err.values()) <= BAR, (b, err)


def test_a_nan_at_an_observed_entry_fails_that_replica_alone():
    cs = RC.find(20, 10, "matern", 1, "rob-mask")
    res = _device(RC.CASES.index(cs))
    pbs = [dict(RC.reference(cs, seed=s)[0]) for s in SEEDS]
    t = 17
    i = int(np.flatnonzero(pbs[1]["mask"][:, t])[0])
    Y = pbs[1]["Y"].copy()
    Y[i, t] = np.nan
    pbs[1]["Y"] = Y
    out = _call(pbs, True, **_kw(cs))
    assert list(out["status"]) == [0, ERR_NUMERIC, 0]
    for b in (0, 2):
        assert all(np.array_equal(out[k][b], res[k][b]) for k in RC.COMPARED), f"replica {b} was touched by its neighbour's failure"
    with pytest.raises(np.linalg.LinAlgError, match="replica 1"):
        _call(pbs, True, status=None, **_kw(cs))


def test_refusals_by_message():
    from rpsmf_amd.ssm import linear_psmf_batch, rPSMF

    def run(d=8, r=2, p=4, **kw):
        return linear_psmf_batch(np.zeros((d, 6)), np.ones((d, r)), np.zeros(p), np.eye(r), np.eye(p), np.eye(p), np.eye(p), np.ones((r, p)),
                                 0.5, **kw)

    with pytest.raises(ValueError, match="d <= 512"):
        run(d=513, robust=True, lambda0=2.0)
    with pytest.raises(ValueError, match="r <= 16"):
        run(r=17, p=20, mask=np.ones((8, 6), dtype=bool))
    with pytest.raises(ValueError, match="lambda0 > 0"):
        run(robust=True, lambda0=0.0)
    with pytest.raises(ValueError, match="lambda0 > 0"):
        run(robust=True)
    with pytest.raises(ValueError, match="alpha and beta"):
        run(robust=True, lambda0=2.0, beta=0.0)
    m = np.ones((8, 6), dtype=bool)
    m[:, 3] = False
    with pytest.raises(ValueError, match="no observed row in replica 0, step 3"):
        run(mask=m)
    with pytest.raises(ValueError, match="0 and 1 only"):
        run(mask=3 * np.ones((8, 6)))
    with pytest.raises(ValueError, match="mask has shape"):
        run(mask=np.ones((6, 8), dtype=bool))
    with pytest.raises(ValueError, match="lambda0 > 0"):
        rPSMF(2, np.zeros((8, 6)), np.eye(4), np.eye(4), 0.1, np.ones((2, 4)), np.eye(2), np.eye(4), np.ones((8, 2)), None, 8, 6, np.nan,
              x0=np.zeros(4))
    # the same arguments on a problem that is not degenerate run (above, H = ones makes P_z singular: nothing there reaches the kernel)
    pb = RC.problem(RC.find(5, 2, "dense", 1, "rob-mask"))
    ok = linear_psmf_batch(pb["Y"], pb["C0"], pb["x0"], pb["V"], pb["P0"], pb["A"], pb["Q"], pb["H"], pb["rho"], robust=True, lambda0=2.0,
                           mask=pb["mask"].astype(bool))
    assert ok["status"][0] == 0 and ok["omega"].shape == (1, 40) and np.all(ok["omega"] > 0)


@pytest.mark.parametrize("variant", ["rob", "rob-fix-mask"])
def test_the_drop_in_is_the_batch_entry_point_with_carry_P_off(variant):
    from rpsmf_amd.ssm import PSMF, rPSMF

    cs = RC.find(20, 10, "matern", 0, variant)
    pb, ref = RC.reference(cs, seed=0)
    res = _device(RC.CASES.index(cs))
    d, n, r = cs["d"], cs["n"], cs["r"]
    X = rPSMF(r, pb["Y"], pb["Q"], pb["A"], pb["rho"] * np.eye(d), pb["H"], pb["V"], pb["P0"], pb["C0"], np.zeros((cs["p"], n)), d, n,
              cs["lambda0"], x0=pb["x0"], fixed_lambda=cs["fixed_lambda"], mask=pb["mask"] if cs["masked"] else None)
    assert X.shape == (cs["p"], n)
    assert np.array_equal(X, res["X"][0]), "rPSMF(...) and linear_psmf_batch(robust=True, carry_P=False) give different bits"
    err = relerr(X, ref["X"])
    print(f"\nssm robust drop-in against the literal model, {variant}: {err}")
    assert err <= BAR
    if cs["masked"]:
        mk = RC.find(20, 10, "matern", 0, "mask")
        Xm = PSMF(r, pb["Y"], pb["Q"], pb["A"], pb["rho"], pb["H"], pb["V"], pb["P0"], pb["C0"], None, d, n, x0=pb["x0"], mask=pb["mask"])
        assert np.array_equal(Xm, _device(RC.CASES.index(mk))["X"][0]), "PSMF(mask=...) and linear_psmf_batch(mask=...) give different bits"
