"""tests/noise_cases.py without a GPU: (1) the seeded case list of the noise net covers what its docstring claims -- every row
count, rank, storage x upload dtype, filter, spectrum of R, mode, run shape and switch, in the admitted set -- so that the net
cannot go thin unnoticed; (2) every case is well enough conditioned for its bar to mean something: the float64 oracle runs it to
finite values and its answer moves by at most 1/16 of the bar when C0, Y and theta move by a relative 2^-50 (float32 storage:
2^-23, after the rounding); noise_cases.RESOLUTION records the outcome and this file recomputes it; (3) the two references agree
with a second model each: oracle.literal_step (extended by the theta gradient) with lowrank_step at every diagonal R of the list,
and on every dense case literal_step on R with lowrank_step on (U^T y, U^T C, lam) rotated back -- the identity the device relies
on; (4) the edges of rpsmf_amd._noise.structure_of, which decides what a handle is given.
Reference: pypsmf/psmf/psmf.py:85-180, rpsmf.py:116-184 (through oracle/)."""

from collections import Counter

import numpy as np
import pytest

import netlib
import noise_cases as NC
from oracle import psmf_oracle as O
from rpsmf_amd import _noise

CASES = [NC.device_case(i) for i in range(NC.N_CASES)]
ROW = [cs for cs in CASES if cs["family"] == "row"]
DENSE = [cs for cs in CASES if cs["family"] == "dense"]


@pytest.mark.parametrize("i", range(NC.N_CASES))
def test_case_is_admissible_by_the_oracle_alone(i):
    """No LinAlgError, finite, and the oracle's response to a last-bit change of the inputs is at most bar / 16: for the recorded
    resolution of the case, and -- for the cases the table lists -- not for the draw it replaced."""
    (salt, halved), log = NC.resolve(i)
    for line in log:
        print("\nnot admissible:", line)
    assert (salt, halved) == NC.RESOLUTION.get(i, (0, 0)), (i, salt, halved, log)


def test_the_case_list_is_what_the_module_says():
    assert len(ROW) == NC.N_ROW == 36 and len(DENSE) == NC.N_DENSE == 24 and set(NC.RESOLUTION) <= set(range(NC.N_CASES))
    print("\nshortened or replaced (case: (salt, times halved)):", NC.RESOLUTION)
    for cs in CASES:
        assert cs["r"] <= cs["d"] and 2 <= cs["T"] <= NC.T_MAX and not cs["masked"] and cs["nonuniform"]
        assert cs["parts"][0][0] == 0 and cs["parts"][-1][1] == cs["T"] and all(a <= b for a, b in cs["parts"])
        assert all(p[1] == q[0] for p, q in zip(cs["parts"][:-1], cs["parts"][1:])), cs["parts"]
        assert 1 <= sum(1 for a, b in cs["parts"] if b > a) <= 3
        assert not (cs["sched"] and cs["robust"]) and not (cs["dyn"] in NC.BC.DENSE_KINDS and cs["r"] > NC.DENSE_KIND_R_MAX)
        assert NC.bar(cs) == ({"row": 1e-9, "dense": 1e-8}[cs["family"]] if cs["storage"] == "f64" else 1e-5)
        assert NC.gradsum_bar(cs) == (1e-7 if cs["storage"] == "f64" else 1e-5)
    assert all(cs["d"] <= NC.DENSE_D_MAX and not cs["env"] and not cs["shards"] for cs in DENSE)


def test_every_axis_value_is_in_the_admitted_set():
    assert {cs["d"] for cs in ROW} == set(NC.D_LIST) and {cs["d"] for cs in DENSE} == {d for d in NC.D_LIST if d <= NC.DENSE_D_MAX}
    for name, fam in (("row", ROW), ("dense", DENSE)):
        assert {cs["r"] for cs in fam} == set(NC.R_LIST), name
        assert {(cs["storage"], cs["upload"]) for cs in fam} == set(NC.IO), name
        assert {cs["filter"] for cs in fam} == set(NC.FILTERS), name
        assert any(cs["robust"] and cs["fixed_lambda"] for cs in fam) and any(cs["robust"] and cs["alpha"] != 1.0 and cs["beta"] != 1.0 for cs in fam)
        assert {cs["mode"] for cs in fam} == set(range(len(NC.MODES))), name
        assert {cs["hooks"] for cs in fam} == set(NC.HOOKS) and {cs["dyn"] for cs in fam} == {"random_walk", "cos_phase", "scaled_walk"}, name
        assert {(cs["recursive"], cs["update_every"] > 1) for cs in fam if cs["recursive"]} == {(1, True), (2, True)}, name
        assert any(cs["sched"] for cs in fam) and any(cs["general_Q"] for cs in fam), name
        # weights under the simplified hooks: no weighted Gram, but rPSMF's quad takes the per-row kappa
        assert any(cs["robust"] and cs["hooks"] == "simplified" for cs in fam) or any(cs["robust"] and cs["hooks"] == "no_update" for cs in fam), name
        assert {cs["shape"] for cs in fam} == set(NC.SHAPES) and {sum(1 for a, b in cs["parts"] if b > a) for cs in fam} == {1, 2, 3}, name
        cuts = Counter()
        for cs in fam:
            for _, b in cs["parts"][:-1]:
                cuts["1"] += b == 1
                cuts["T-1"] += b == cs["T"] - 1
        assert cuts["1"] >= 4 and cuts["T-1"] >= 4, (name, cuts)
        assert any(a == b for cs in fam for a, b in cs["parts"]), name
        assert any(cs["second_pass"] and cs["robust"] for cs in fam) and any(cs["second_pass"] and not cs["robust"] for cs in fam), name
    assert {cs["spectrum"] for cs in ROW} == set(NC.ROW_SPECTRA) and {cs["spectrum"] for cs in DENSE} == set(NC.DENSE_SPECTRA)
    # the switch of the weighted Gram, on and off, where the step forms one (coef_update) -- at every padded rank
    for sw in ({}, {"PSMF_WGRAM_MFMA": "0"}):
        have = {NC.SC.rpad_of(cs["r"]) for cs in ROW if cs["env"] == sw and NC.HOOKS[cs["hooks"]][0]}
        assert have == {8, 16, 32, 64}, (sw, have)


def test_the_spectra_are_what_their_names_say():
    for cs in ROW:
        rho = NC.row_noise(cs)
        assert rho.shape == (cs["d"],) and np.all(rho >= 0.0) and rho.sum() > 0.0
        if cs["spectrum"] == "benign":
            assert rho.min() >= 0.3 and rho.max() <= 2.3
        elif cs["spectrum"] == "spread_1e6":
            assert rho.max() / rho.min() == 1e6
        elif cs["spectrum"] == "zeros":
            assert 1 <= np.count_nonzero(rho == 0.0) <= 3 and np.count_nonzero(rho) >= 1
        else:
            assert sorted(Counter(rho.tolist()).values()) == ([1, cs["d"] - 1] if cs["d"] > 2 else [1, 1])
    for cs in DENSE:
        d, R = cs["d"], NC.dense_noise(cs)
        assert np.array_equal(R, R.T) and np.count_nonzero(R) > np.count_nonzero(np.diagonal(R))
        lam, U = NC.eigen(dict(R0=R), d)
        assert lam.min() >= 0.0 and np.allclose((U * lam) @ U.T, R, rtol=0.0, atol=1e-12 * lam.max())
        zero = int(np.count_nonzero(lam <= 1e-12 * lam.max()))
        if cs["spectrum"] == "singular":
            assert zero == d - max(1, d // 2) >= 1 and np.count_nonzero(lam == 0.0) >= 1, (d, zero)          # (clipped to 0 exactly)
        else:
            assert zero == 0, (cs["spectrum"], d, zero)
        if cs["spectrum"] == "well":
            assert lam.max() / lam.min() < 1e3
        if cs["spectrum"] == "block":
            n = d // 3 if d >= 6 else 2
            assert not R[:n, n:].any() and R[:n, :n].all()
        if cs["spectrum"] == "repeated":
            assert np.count_nonzero(np.abs(lam - 0.5) < 1e-12) == max(2, d // 2)


def test_the_shards():
    assert len(NC.SHARDED) == 6 and NC.SHARDS == (2, 3)
    sh = [cs for cs in CASES if cs["shards"]]
    assert [cs["i"] for cs in sh] == list(NC.SHARDED) and all(cs["family"] == "row" and cs["d"] >= 15 and cs["dyn"] == "random_walk" for cs in sh)
    assert len({cs["mode"] for cs in sh}) == 6 and {cs["storage"] for cs in sh} == {"f32", "f64"} and any(cs["robust"] for cs in sh)


def _agree(cs, ref0, ref1):
    """two models of one case, to within the margin of the admission"""
    state, grad = netlib.response(ref0, ref1, NC.compared(cs)), NC.BC.grad_response(ref0, ref1)
    print(f"\ncase {cs['i']} {NC.describe(cs)}: state {state:.2e} (bar {NC.bar(cs):.0e}), gradsum {grad:.2e}")
    assert state <= NC.bar(cs) / 16 and grad <= NC.gradsum_bar(cs) / 16, (cs, state, grad)
    for a, b in zip(ref0, ref1):
        assert np.array_equal(a["theta"].shape, b["theta"].shape) and netlib.relerr(b["theta"], a["theta"]) <= NC.bar(cs) / 16


@pytest.mark.parametrize("i", [cs["i"] for cs in ROW if cs["d"] <= NC.DENSE_D_MAX])
def test_literal_step_with_the_theta_gradient_is_lowrank_step_at_a_diagonal_R(i):
    """The dense restatement (d x d matrices, Woodbury inverse) against the O(d r^2) one on the row cases: state, y_pred, rPSMF's
    scalars, and the gradient sum and the stepped theta that literal_step now carries."""
    cs = CASES[i]
    pb = NC.problem(cs)
    _agree(cs, NC.reference(cs, pb), NC.run_oracle(cs, pb, pb["Y"], pb["C0"], pb["rho_rows"], O.literal_step))


@pytest.mark.parametrize("i", [cs["i"] for cs in DENSE])
def test_dense_step_is_the_row_step_in_the_eigenbasis(i):
    """literal_step on R (the dense inverse) against lowrank_step on (U^T y, U^T C, lam) rotated back: what the device does"""
    cs = CASES[i]
    pb = NC.problem(cs)
    _agree(cs, NC.reference(cs, pb), NC.reference_rotated(cs, pb))


def test_structure_of_edges():
    d = 6
    rng = np.random.default_rng(4)
    A = rng.standard_normal((d, d))
    R = A @ A.T / d + 0.1 * np.eye(d)
    R = 0.5 * (R + R.T)
    (lam, U), rows = _noise.structure_of(R, d)
    assert rows is lam and np.allclose((U * lam) @ U.T, R, rtol=0.0, atol=1e-14)
    # asymmetry inside the tolerance (rtol 1e-12) is a rounding of the caller's; outside it is not a covariance
    Rin, Rout = R.copy(), R.copy()
    Rin[1, 4] *= 1.0 + 1e-13
    Rout[1, 4] *= 1.0 + 1e-9
    assert Rin[1, 4] != Rin[4, 1]
    (lam_in, _), _ = _noise.structure_of(Rin, d)
    assert np.allclose(lam_in, lam, rtol=1e-12, atol=0.0)
    with pytest.raises(NotImplementedError, match="symmetric"):
        _noise.structure_of(Rout, d)
    # an eigenvalue of -1e-13 lam_max is rounding and is clipped; -1e-6 lam_max is an indefinite matrix
    Q = np.linalg.qr(rng.standard_normal((d, d)))[0]
    ev = np.array([-1e-13, 0.2, 0.5, 0.7, 0.9, 1.0])
    Rc = (Q * ev) @ Q.T
    (lam_c, _), _ = _noise.structure_of(0.5 * (Rc + Rc.T), d)
    assert lam_c[0] == 0.0 and np.allclose(lam_c[1:], ev[1:], rtol=1e-12)
    ev[0] = -1e-6
    Rn = (Q * ev) @ Q.T
    with pytest.raises(NotImplementedError, match="semi-definite"):
        _noise.structure_of(0.5 * (Rn + Rn.T), d)
    # a (d, d) matrix without an entry off the diagonal is a diagonal R: not dense -- rows if they differ, nothing if R = c I
    dg = 0.3 + rng.random(d)
    dense, rows = _noise.structure_of(np.diag(dg), d)
    assert dense is None and np.array_equal(rows, dg)
    assert _noise.structure_of(0.7 * np.eye(d), d) == (None, None)
    dg[2] = 0.0          # (a zero on the diagonal of a diagonal R: still its rows)
    dense, rows = _noise.structure_of(np.diag(dg), d)
    assert dense is None and np.array_equal(rows, dg)
    # zeros on the diagonal with entries off it: PSD only if their rows are zero -- R = v v^T with v = (1, 1, 0) is dense and singular
    v = np.array([1.0, 1.0, 0.0])
    (lam_v, U_v), _ = _noise.structure_of(np.outer(v, v), 3)
    assert np.allclose(lam_v, [0.0, 0.0, 2.0], atol=1e-15) and lam_v.min() >= 0.0 and np.allclose((U_v * lam_v) @ U_v.T, np.outer(v, v), atol=1e-15)
    with pytest.raises(NotImplementedError, match="semi-definite"):
        _noise.structure_of(np.array([[0.0, 1.0], [1.0, 0.0]]), 2)          # a zero diagonal under a coupling: indefinite
