"""tests/ssm_robust_cases.py without a GPU: the robust (rPSMF) and masked forms of the batched PSMF with linear-Gaussian dynamics and
an observation map.  Every case (1) runs to finite values with V positive definite in the line-for-line model; (2) admits the
r x r algebra the kernel implements: device_algebra_model agrees with literal_model to 1e-11 on X, C, V, P, x, Ypred, (s, eta),
omega, phi and (lambda, Omega); (3) is conditioned well enough for the device bar (5e-9) to mean something: C0 and x0 moved by
4 * 2^-52 move every compared array by at most 1e-11 -- conditions on the inputs, 500 x below the device bar; (4) depends on what it
is about: the robust flag moves X by more than 1e-2, and so does reading the masked entries as zeros.
With robust off and an all-ones mask the line-for-line model is ssm_cases.literal_model; a series cut in two is the same recursion
when (lambda, Omega) is handed on; and the argument checks of rpsmf_amd/ssm.py that need no device."""

import numpy as np
import pytest

import ssm_cases as SC
import ssm_robust_cases as RC
from rpsmf_amd import ssm


def test_the_list_is_ssm_cases_in_five_variants():
    assert len(RC.CASES) == 80 and len(set(RC.IDS)) == 80
    for v, (robust, lambda0, fixed, masked) in RC.VARIANTS.items():
        mine = [c for c in RC.CASES if c["variant"] == v]
        assert [(c["d"], c["r"], c["p"], c["kind"], c["carry_P"]) for c in mine] == [(c["d"], c["r"], c["p"], c["kind"], c["carry_P"]) for c in SC.CASES]
        assert all(c["n"] <= 60 and c["n"] <= s["n"] for c, s in zip(mine, SC.CASES))
        assert {c["carry_P"] for c in mine} == {0, 1}
        assert all((c["robust"], c["lambda0"], c["fixed_lambda"], c["masked"]) == (robust, lambda0, fixed, masked) for c in mine)
    assert sorted(RC.VARIANTS.values(), key=str) == sorted([(True, 1.8, False, False), (True, 10.0, True, False), (False, None, False, True),
                                                            (True, 1.8, False, True), (True, 10.0, True, True)], key=str)
    # coverage: the limits, an odd r, a d that is no multiple of 4
    assert max(c["d"] for c in RC.CASES) == ssm.MAX_D and max(c["r"] for c in RC.CASES) == ssm.MAX_R and max(c["p"] for c in RC.CASES) == ssm.MAX_P
    assert any(c["r"] % 2 for c in RC.CASES) and any(c["d"] % 4 for c in RC.CASES)


def test_the_problem_is_contaminated_and_every_column_is_observed():
    for cs in (RC.find(20, 10, "matern", 1, "rob-mask"), RC.find(512, 3, "dense", 0, "mask"), RC.find(5, 2, "dense", 1, "rob")):
        pb = RC.problem(cs)
        clean = SC.problem(dict(cs))
        moved = np.mean(pb["Y"] != clean["Y"])
        assert pb["Y"].shape == (cs["d"], cs["n"]) and 0.02 <= moved <= 0.09, moved
        assert np.array_equal(pb["C0"], clean["C0"]) and np.array_equal(pb["A"], clean["A"]) and pb["rho"] == clean["rho"]
        m = pb["mask"]
        assert m.dtype == np.uint8 and m.shape == pb["Y"].shape and set(np.unique(m)) <= {0, 1} and m.sum(axis=0).min() >= 1
        if cs["masked"]:
            assert 0.7 <= m.mean() <= 0.9
        else:
            assert m.all()


@pytest.mark.parametrize("cs", SC.CASES, ids=SC.IDS)
def test_not_robust_and_all_observed_is_the_literal_model_of_ssm_cases(cs):
    """1e-13: the two are the same expressions (measured <= 1e-16)"""
    pb = dict(SC.reference(cs)[0])
    pb["mask"] = np.ones(pb["Y"].shape, dtype=np.uint8)
    mine, ref = RC.literal_model(pb, cs["carry_P"]), SC.reference(cs)[1]
    err = {k: RC.relerr(mine[k], ref[k]) for k in SC.COMPARED}
    print(f"\nssm robust literal model, robust off, all observed, {SC.IDS[SC.CASES.index(cs)]}: {err}")
    assert max(err.values()) <= 1e-13, err
    assert np.array_equal(mine["omega"], np.ones(cs["n"])) and np.array_equal(mine["phi"], np.ones(cs["n"]))


@pytest.mark.parametrize("cs", RC.CASES, ids=RC.IDS)
def test_case_by_the_models_alone(cs):
    pb, ref = RC.reference(cs)
    kw = RC.model_kw(cs)
    d, n = cs["d"], cs["n"]
    # (1) finite, V positive definite
    for k, v in ref.items():
        assert np.all(np.isfinite(v)), k
    assert np.linalg.eigvalsh(0.5 * (ref["V"] + ref["V"].T)).min() > 0
    assert ref["omega"].shape == (n,) and ref["phi"].shape == (n,) and ref["robust_state"].shape == (2,)
    # (2) the kernel's algebra
    alg = RC.device_algebra_model(pb, cs["carry_P"], **kw)
    algebra = {k: RC.relerr(alg[k], ref[k]) for k in RC.COMPARED}
    # (3) conditioning: a few ulp on C0 and x0
    pert = RC.literal_model(RC.problem(cs, perturb=(d + n, 4 * 2.0 ** -52)), cs["carry_P"], **kw)
    cond = {k: RC.relerr(pert[k], ref[k]) for k in RC.COMPARED}
    # (4) the robust flag; the mask (the masked entries read as zeros)
    moved = {}
    if cs["robust"]:
        moved["robust"] = RC.relerr(RC.literal_model(pb, cs["carry_P"])["X"], ref["X"])
        assert np.isclose(ref["robust_state"][0], 10.0 if cs["fixed_lambda"] else 1.8 + n * d, rtol=1e-12) and ref["robust_state"][1] != 1.0
    else:
        assert np.array_equal(ref["robust_state"], [0.0, 1.0]) and np.all(ref["omega"] == 1.0) and np.all(ref["phi"] == 1.0)
    if cs["masked"]:
        zeros = dict(pb, Y=np.where(pb["mask"] > 0, pb["Y"], 0.0))
        moved["mask"] = RC.relerr(RC.literal_model(zeros, cs["carry_P"], mask=np.ones_like(pb["mask"]), **kw)["X"], ref["X"])
        # what stands under a zero is not read
        nan = dict(pb, Y=np.where(pb["mask"] > 0, pb["Y"], np.nan))
        assert np.array_equal(RC.literal_model(nan, cs["carry_P"], **kw)["X"], ref["X"])
    print(f"\nssm robust case {RC.IDS[RC.CASES.index(cs)]}: algebra {algebra}; a few ulp on C0, x0 {cond}; moved by {moved}; "
          f"(lambda, Omega) {ref['robust_state']}")
    assert max(algebra.values()) <= 1e-11, algebra
    assert max(cond.values()) <= 1e-11, cond
    assert moved and min(moved.values()) > 1e-2, moved


@pytest.mark.parametrize("variant", ["rob-mask", "rob-fix-mask"])
@pytest.mark.parametrize("carry_P", [1, 0])
def test_continuing_a_series_is_the_same_recursion(carry_P, variant):
    """n steps at once against n1 + n2 with C, V, x, P and (lambda, Omega) handed on"""
    cs = RC.find(33, 7, "dense", carry_P, variant)
    pb, ref = RC.reference(cs)
    kw = RC.model_kw(cs)
    n1 = 17
    for model in (RC.literal_model, RC.device_algebra_model):
        whole = ref if model is RC.literal_model else model(pb, carry_P, **kw)
        a = model(dict(pb, Y=pb["Y"][:, :n1], mask=pb["mask"][:, :n1]), carry_P, **kw)
        b = model(dict(pb, Y=pb["Y"][:, n1:], mask=pb["mask"][:, n1:], C0=a["C"], V=a["V"], x0=a["x"], P0=a["P"]), carry_P, first_step=False,
                  robust_state=a["robust_state"], **kw)
        assert np.array_equal(np.concatenate([a["X"], b["X"]], axis=1), whole["X"]) and np.array_equal(b["P"], whole["P"])
        assert np.array_equal(np.concatenate([a["omega"], b["omega"]]), whole["omega"])
        assert np.array_equal(b["robust_state"], whole["robust_state"])
        # without the hand-over it is another series
        c = model(dict(pb, Y=pb["Y"][:, n1:], mask=pb["mask"][:, n1:], C0=a["C"], V=a["V"], x0=a["x"], P0=a["P"]), carry_P, first_step=False,
                  robust_state=np.array([kw["lambda0"], 1.0]), **kw)
        assert RC.relerr(c["X"], b["X"]) > 1e-3


def test_argument_checks_need_no_device():
    run = ssm.linear_psmf_batch
    I2, I4, H = np.eye(2), np.eye(4), np.ones((2, 4))
    Y, C0, x0 = np.zeros((3, 8, 6)), np.ones((3, 8, 2)), np.zeros((3, 4))
    args = (Y, C0, x0, I2, I4, I4, I4, H, 0.5)
    ones = np.ones((3, 8, 6), dtype=bool)
    # the mask: shape and values
    with pytest.raises(ValueError, match="mask has shape"):
        run(*args, mask=ones[:2])
    with pytest.raises(ValueError, match="mask has shape"):
        run(*args, mask=ones[0])                       # (d, n) is for a single series
    with pytest.raises(ValueError, match="mask has shape"):
        run(*args, mask=np.ones((3, 6, 8), dtype=bool))
    with pytest.raises(ValueError, match="0 and 1 only"):
        run(*args, mask=2 * np.ones((3, 8, 6)))
    with pytest.raises(ValueError, match="0 and 1 only"):
        run(*args, mask=np.where(ones, 0.5, 0.0))
    with pytest.raises(ValueError, match="0 and 1 only"):
        run(*args, mask=np.full((3, 8, 6), "1"))
    # the empty column: the replica and the step by name
    m = ones.copy()
    m[2, :, 4] = False
    with pytest.raises(ValueError, match="no observed row in replica 2, step 4"):
        run(*args, mask=m)
    with pytest.raises(ValueError, match="no observed row in replica 2, step 4"):
        run(*args, mask=m.astype(np.float64), robust=True, lambda0=2.0)
    # lambda0, alpha, beta
    for bad in (None, 0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="lambda0 > 0"):
            run(*args, robust=True, lambda0=bad)
    with pytest.raises(ValueError, match="alpha and beta"):
        run(*args, robust=True, lambda0=2.0, alpha=0.0)
    with pytest.raises(ValueError, match="alpha and beta"):
        run(*args, robust=True, lambda0=2.0, beta=-1.0)
    with pytest.raises(ValueError, match="needs robust_state"):
        run(*args, robust=True, lambda0=2.0, first_step=False)
    with pytest.raises(ValueError, match="robust_state has shape"):
        run(*args, robust=True, lambda0=2.0, first_step=False, robust_state=np.ones((3, 3)))
    with pytest.raises(ValueError, match="belong to robust=True"):
        run(*args, lambda0=2.0)
    with pytest.raises(ValueError, match="belong to robust=True"):
        run(*args, mask=ones, fixed_lambda=True)
    # the limits are psmf_ssm_run's, through the new entry point too
    with pytest.raises(ValueError, match="psmf_ssm_run_ex.*d <= 512"):
        run(np.zeros((513, 6)), np.ones((513, 2)), np.zeros(4), I2, I4, I4, I4, H, 0.5, robust=True, lambda0=2.0)
    with pytest.raises(ValueError, match="psmf_ssm_run_ex.*Q must be symmetric"):
        Q = np.eye(4)
        Q[0, 1] = 0.1
        run(Y, C0, x0, I2, I4, I4, Q, H, 0.5, mask=ones)


def test_the_library_refuses_by_itself():
    """psmf_ssm_run_ex's own checks (before it looks for a device): what the Python layer would have caught first"""
    import ctypes as C

    from rpsmf_amd import _capi

    lib = _capi.load_library()
    B, d, n, r, p = 2, 8, 6, 2, 4
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    Y, Cm, V, x, P = np.zeros((B, n, d)), np.ones((B, d, r)), np.stack([np.eye(r)] * B), np.zeros((B, p)), np.stack([np.eye(p)] * B)
    A, Q, H, X, sc, rs = np.eye(p), np.eye(p), np.ones((r, p)), np.zeros((B, n, p)), np.zeros((B, n, 4)), np.ones((B, 2))

    def call(mask=None, **kw):
        f = dict(abi_version=_capi.ABI_VERSION, d=d, n=n, r=r, p=p, batch=B, device=0, carry_P=1, first_step=1, want_pred=0, robust=1,
                 fixed_lambda=0, lambda0=2.0, alpha=1.0, beta=1.0)
        f.update(kw)
        cfg = _capi.PsmfSsmConfigEx(**f)
        rc = lib.psmf_ssm_run_ex(C.byref(cfg), dp(Y), None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_uint8)), dp(Cm), dp(V),
                                 dp(x), dp(P), dp(A), dp(Q), dp(H), 0.5, dp(rs), dp(X), None, dp(sc), None, None)
        return rc, lib.psmf_last_error(None).decode()

    for kw, msg in ((dict(lambda0=0.0), "lambda0 > 0"), (dict(lambda0=float("nan")), "lambda0 > 0"), (dict(alpha=0.0), "alpha and beta"),
                    (dict(beta=-2.0), "alpha and beta")):
        rc, text = call(**kw)
        assert rc == _capi.ERR_ARG and msg in text and text.startswith("psmf_ssm_run_ex: "), (kw, rc, text)
    m = np.ones((B, n, d), dtype=np.uint8)
    m[1, 3, :] = 0
    rc, text = call(mask=m)
    assert rc == _capi.ERR_ARG and "replica 1, step 3" in text, (rc, text)
    rc, text = call(mask=m, robust=0)
    assert rc == _capi.ERR_ARG and "replica 1, step 3" in text, (rc, text)
    m[1, 3, 0] = 7
    rc, text = call(mask=m)
    assert rc == _capi.ERR_ARG and "0 and 1 only" in text, (rc, text)


def test_the_drop_ins_take_the_new_arguments():
    import inspect

    sig = inspect.signature(ssm.rPSMF)
    assert list(sig.parameters) == ["r", "Y", "Q", "A", "R", "H", "V", "P0", "C", "X", "m", "n", "lambda0", "x0", "rng", "carry_P", "fixed_lambda",
                                    "mask"]
    assert sig.parameters["carry_P"].default is False and sig.parameters["fixed_lambda"].default is False
    assert list(inspect.signature(ssm.PSMF).parameters)[-1] == "mask"
    Y, Cm = np.zeros((8, 6)), np.ones((8, 2))
    R = 0.1 * np.eye(8)
    R[0, 1] = 0.01
    with pytest.raises(NotImplementedError, match="rho \\* I"):
        ssm.rPSMF(2, Y, np.eye(4), np.eye(4), R, np.ones((2, 4)), np.eye(2), np.eye(4), Cm, None, 8, 6, 2.0, x0=np.zeros(4))
    with pytest.raises(ValueError, match="lambda0 > 0"):
        ssm.rPSMF(2, Y, np.eye(4), np.eye(4), 0.1, np.ones((2, 4)), np.eye(2), np.eye(4), Cm, None, 8, 6, -1.0, x0=np.zeros(4))
    with pytest.raises(ValueError, match="no observed row in replica 0, step 2"):
        m = np.ones((8, 6), dtype=bool)
        m[:, 2] = False
        ssm.PSMF(2, Y, np.eye(4), np.eye(4), 0.1, np.ones((2, 4)), np.eye(2), np.eye(4), Cm, None, 8, 6, x0=np.zeros(4), mask=m)
    assert "rob" in ssm.__doc__ and "omega = (lambda + e^T S^-1 e) / (lambda + d)" in ssm.__doc__
