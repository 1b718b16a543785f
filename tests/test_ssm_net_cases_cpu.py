"""tests/ssm_net_cases.py without a GPU: the random-configuration net of the batched PSMF with linear-Gaussian dynamics and an
observation map is sound.  (1) Every case is admitted by the two float64 models alone -- finite, V positive definite, the kernel's
r x r algebra within 1e-11 of the line-for-line d x d model on every compared array, and 4 * 2^-52 on C0 and x0 moving every
compared array by at most 1e-11 (500 x below the device bar) -- and ssm_net_cases.REPLACED is what that admission answers;
(2) at most 5 % of the draws were replaced; (3) the coverage the net is for, asserted so that it cannot go thin unnoticed;
(4) the net can see what it is for: four deliberately wrong variants of the line-for-line model each move some compared array by
more than 1e-6 (200 x the device bar) in at least 10 cases.
Wall time: about a minute on one core."""

from collections import Counter

import numpy as np
import pytest

import ssm_net_cases as NC
import ssm_robust_cases as RC

CASES = [NC.device_case(i) for i in range(NC.N_CASES)]
BY_INSTANCE = {name: [c for c in CASES if NC.instance(c) == name] for name in NC.INSTANCES}


def test_the_draw_is_a_function_of_the_case_number():
    assert NC.N_CASES == 240 and all(len(v) == NC.N_CASES // 4 for v in BY_INSTANCE.values())
    for i in (0, 7, 101, 238):
        assert NC.case(i) == NC.case(i) and NC.instance(NC.case(i)) == NC.INSTANCES[i % 4]
        a, b = NC.problem(NC.case(i)), NC.problem(NC.case(i))
        assert all(np.array_equal(x[k], y[k]) for x, y in zip(a, b) for k in x)
        assert NC.case(i, 1) != NC.case(i)
    assert NC.bar(CASES[0]) == 5e-9 and NC.ADMIT == 1e-11 and NC.EPS == 4 * 2.0 ** -52


def test_every_problem_is_what_the_module_says():
    for cs in CASES[::7]:
        pbs = NC.problem(cs)
        d, n, r, p = cs["d"], cs["n"], cs["r"], cs["p"]
        assert len(pbs) == cs["batch"] and cs["batch"] in (2, 3)
        pb = pbs[0]
        assert 1 <= r <= p <= 32 and r <= 16 and 1 <= d <= 512 and n in NC.N_LIST and (d <= 256 or n <= 40)
        assert not np.allclose(pb["A"], pb["A"].T) or p == 1
        assert np.array_equal(pb["Q"], pb["Q"].T) and np.linalg.eigvalsh(pb["Q"]).min() > 0
        sv = np.linalg.svd(pb["H"], compute_uv=False)
        assert pb["H"].shape == (r, p) and 0.5 - 1e-12 <= sv.min() and sv.max() <= 1.5 + 1e-12
        for q in pbs:
            assert q["Y"].shape == (d, n) and q["C0"].shape == (d, r) and q["x0"].shape == (p,)
            assert np.array_equal(q["V"], q["V"].T) and np.linalg.eigvalsh(q["V"]).min() > 0 and (r == 1 or np.count_nonzero(q["V"]) == r * r)
            assert np.array_equal(q["P0"], q["P0"].T) and np.linalg.eigvalsh(q["P0"]).min() > 0
            m = q["mask"]
            assert m.dtype == np.uint8 and m.shape == (d, n) and set(np.unique(m)) <= {0, 1} and m.sum(axis=0).min() >= 1
            assert cs["masked"] or m.all()
        assert not np.array_equal(pbs[0]["Y"], pbs[1]["Y"]) and not np.array_equal(pbs[0]["C0"], pbs[1]["C0"])
        assert (pbs[0]["V"] is pbs[1]["V"]) == (not cs["own_VP"]) and np.array_equal(pbs[0]["V"], pbs[1]["V"]) == (not cs["own_VP"])
        rho_ok = NC.RHOS if d <= 64 else NC.RHOS[1:]
        assert cs["rho"] in rho_ok


def test_the_structured_masks_are_what_they_are_called():
    seen = Counter()
    for cs in CASES:
        if cs["mask_kind"] not in NC.STRUCTURED:
            continue
        seen[cs["mask_kind"]] += 1
        d = cs["d"]
        for q in NC.problem(cs):
            m = q["mask"].astype(bool)
            cnt = m.sum(axis=0)
            if cs["mask_kind"] == "last-row":
                assert d >= 2 and np.any((cnt == 1) & m[d - 1])
            elif cs["mask_kind"] == "dark-wave":
                assert d >= 65 and any((~m[64 * k:64 * k + 64]).all(axis=0).any() for k in range((d + 63) // 64))
            else:
                assert d >= 2 and cs["n"] >= 2 and np.any(cnt == d) and np.any(cnt < d)
    print("\nstructured masks:", dict(seen))
    assert all(seen[k] >= 6 for k in NC.STRUCTURED), seen
    # the row that alone is observed lies in the second row of its thread somewhere
    assert any(c["mask_kind"] == "last-row" and c["d"] > 256 for c in CASES)


def test_coverage():
    rs, ds = {c["r"] for c in CASES}, {c["d"] for c in CASES}
    assert set(NC.R_EDGES) <= rs and set(NC.D_EDGES) <= ds
    assert {16, 17, 31, 32} <= {c["p"] for c in CASES}
    assert any(c["p"] == c["r"] for c in CASES) and any(c["p"] == c["r"] + 1 for c in CASES)
    assert any(c["p"] == c["r"] and c["r"] >= 15 for c in CASES) and any(c["p"] == 32 and c["r"] <= 3 for c in CASES)
    for name, mine in BY_INSTANCE.items():
        assert {1, 2} <= {c["n"] for c in mine}, name
        assert {15, 16} <= {c["r"] for c in mine}, name
        assert {True, False} == {c["own_VP"] for c in mine} == {c["edge"] for c in mine}, name
        assert {0, 1} == {c["carry_P"] for c in mine}, name
        assert {2, 3} == {c["batch"] for c in mine}, name
    for name in ("masked", "robust+masked"):
        assert any(c["d"] >= 257 for c in BY_INSTANCE[name]), name
        assert set(NC.FRACTIONS) == {c["frac"] for c in BY_INSTANCE[name]}, name
    for name in ("robust", "robust+masked"):
        mine = BY_INSTANCE[name]
        assert any(c["alpha"] != 1 for c in mine) and any(c["beta"] != 1 for c in mine), name
        assert 3 * sum(c["alpha"] != c["beta"] for c in mine) >= len(mine), name
        assert set(NC.LAMBDAS) == {c["lambda0"] for c in mine} and {True, False} == {c["fixed_lambda"] for c in mine}, name
    for name in ("plain", "masked"):
        assert all(c["alpha"] == c["beta"] == 1.0 and c["lambda0"] is None and not c["fixed_lambda"] for c in BY_INSTANCE[name])
    assert set(NC.RHOS) == {c["rho"] for c in CASES}


def test_at_most_a_twentieth_of_the_draws_was_replaced():
    print("\nreplaced draws {case: sub-seed}:", NC.REPLACED)
    assert NC.N_REPLACED == sum(NC.REPLACED.values())
    assert 20 * NC.N_REPLACED <= NC.N_CASES, NC.N_REPLACED


@pytest.mark.parametrize("i", range(NC.N_CASES))
def test_case_is_admitted_by_the_models_alone(i):
    """finite, V positive definite, algebra and conditioning within 1e-11: for the recorded sub-seed of the case, and -- for the
    cases REPLACED lists -- not for the draws it replaced"""
    sub, log = NC.resolve(i)
    for line in log:
        print("\nnot admitted:", line)
    assert sub == NC.REPLACED.get(i, 0), (i, sub, log)


# ---- the net can see what it is for: four wrong variants of ssm_robust_cases.literal_model
def _literal_copy(pb, carry_P, wrong=None, robust=False, lambda0=None, fixed_lambda=False, alpha=1.0, beta=1.0):
    """ssm_robust_cases.literal_model from the first step of a series, statement for statement (wrong=None: the same bits), with
       wrong="sM"       s M in place of s I in S
       wrong="count"    omega and phi divided by lambda + (observed count) in place of lambda + d
       wrong="rho_d"    rho_t d in place of rho_t sum m_i in eta"""
    Y, A, Q, H, rho = pb["Y"], pb["A"], pb["Q"], pb["H"], pb["rho"]
    M = pb["mask"].astype(float)
    C, V, x, P0 = pb["C0"].copy(), pb["V"].copy(), pb["x0"].copy(), pb["P0"]
    d, n = Y.shape
    p = A.shape[0]
    X, Yp, sc = np.zeros((p, n)), np.zeros((d, n)), np.zeros((n, 4))
    P = P0.copy()
    lam, Om = (float(lambda0), 1.0) if robust else (0.0, 1.0)
    for t in range(n):
        m = M[:, t]
        Cm = m[:, None] * C
        Pprev = P if (carry_P or t == 0) else np.zeros((p, p))
        xb = A @ x
        Pb = A @ Pprev @ A.T + Om * Q
        z = H @ xb
        Yp[:, t] = C @ H @ xb
        Rm = np.diag(m * (Om * rho))
        s = z @ V @ z
        PHC = Pb @ H.T @ Cm.T
        CPC = Cm @ (H @ Pb @ H.T) @ Cm.T
        S = CPC + np.diag(m * (Om * rho) + (s * m if wrong == "sM" else s))
        e = np.where(m > 0, np.where(m > 0, Y[:, t], 0.0) - Cm @ H @ xb, 0.0)
        sol = np.linalg.solve(S.T, np.column_stack([PHC.T, e]))
        K, Se = sol[:, :-1].T, sol[:, -1]
        x = xb + K @ e
        den = lam + (m.sum() if wrong == "count" else d)
        omega = (lam + e @ Se) / den if robust else 1.0
        P = (beta * omega if robust else 1.0) * (Pb - K @ Cm @ H @ Pb)
        eta = (np.trace(CPC) + Om * rho * d) / d if wrong == "rho_d" else np.trace(Rm + CPC) / d
        N = xb @ H.T @ V @ H @ xb + eta
        w = xb @ H.T @ V
        Cnew = C + np.outer(e, w) / N
        U = s * m + eta
        phi = (lam + np.sum(e * e / U)) / den if robust else 1.0
        V = (alpha * phi if robust else 1.0) * (V - (V @ H @ np.outer(xb, xb) @ H.T @ V) / N)
        C = Cnew
        X[:, t] = x
        sc[t] = N - eta, eta, omega, phi
        if robust:
            Om = omega * Om
            if not fixed_lambda:
                lam = lam + d
    return RC._out(X, C, V, P, x, Yp, sc, lam, Om)


def test_the_local_copy_of_the_literal_model_is_the_literal_model():
    for i in (3, 6, 11, 50, 121):
        cs, pbs, refs = NC.reference(i)
        mine = _literal_copy(pbs[0], cs["carry_P"], **NC.model_kw(cs))
        assert all(np.array_equal(mine[k], refs[0][k]) for k in RC.COMPARED), i


def _exchanged(cs, pb):
    kw = NC.model_kw(cs)
    kw.update(alpha=cs["beta"], beta=cs["alpha"])
    return RC.literal_model(pb, cs["carry_P"], **kw)


WRONG = {
    "alpha and beta exchanged": (lambda c: c["robust"] and c["alpha"] != c["beta"], _exchanged),
    "s M in place of s I in S": (lambda c: c["masked"], lambda cs, pb: _literal_copy(pb, cs["carry_P"], "sM", **NC.model_kw(cs))),
    "omega, phi over lambda + observed count": (lambda c: c["masked"] and c["robust"],
                                                lambda cs, pb: _literal_copy(pb, cs["carry_P"], "count", **NC.model_kw(cs))),
    "rho_t d in place of rho_t sum m_i in eta": (lambda c: c["masked"], lambda cs, pb: _literal_copy(pb, cs["carry_P"], "rho_d", **NC.model_kw(cs))),
}


@pytest.mark.parametrize("what", list(WRONG))
def test_a_wrong_model_is_seen_by_the_net(what):
    """Each wrong variant moves some compared array of replica 0 by more than 1e-6, 200 x the device bar, in at least 10 cases (the
    search stops there).  `s M` makes the d x d matrix S exactly singular at a step with an unobserved row -- row i of M C is zero, so
    row i of S is its diagonal entry alone, s with s I and 0 with s M: the variant has no finite answer there (LinAlgError, or a
    result that is not finite), which counts as moved; in the r x r algebra of the kernel the unobserved rows never enter."""
    applies, model = WRONG[what]
    seen, tried = [], 0
    for i in range(NC.N_CASES):
        cs = CASES[i]
        if not applies(cs) or cs["n"] * cs["d"] > 4000:          # (small cases first: the search is for ten)
            continue
        _, pbs, refs = NC.reference(i)
        if not (pbs[0]["mask"] == 0).any() and cs["masked"]:
            continue
        tried += 1
        try:
            with np.errstate(all="ignore"):
                got = model(cs, pbs[0])
            moved = max(RC.relerr(got[k], refs[0][k]) if np.all(np.isfinite(got[k])) else np.inf for k in NC.compared(cs))
        except np.linalg.LinAlgError:
            moved = np.inf
        if moved > 1e-6:
            seen.append((i, moved))
        if len(seen) >= 10:
            break
    print(f"\n{what}: seen in {len(seen)} of {tried} cases tried: {[(i, float(f'{m:.2g}')) for i, m in seen]}")
    assert len(seen) >= 10, (what, seen)
