"""tests/masked_noise_cases.py without a GPU, by the oracle alone: every case of the masked per-step engine with per-row
observation noise (1) runs to finite values; (2) depends on the weights -- against the same case with the scalar mean(rho) the
coefficients X differ by more than 1e-2, so a kernel that drops the row weights cannot pass the device test; (3) is well enough
conditioned for the device bars (5e-9 with float64 storage) to mean something: C0 and X0 moved by a few ulp move C, X, Yrec,
YrecL, YrecH by at most 1e-11 -- a condition on the inputs, 500 x below the device bar, not a tolerance of the device; (4) the big
case is one row past one slab per wave of the weighted Gram, and its marked column has observations in second-trip slabs only.
Reference: ExperimentImpute/PSMF.py:40-95, rPSMF.py:40-148, MLESMF.py:40-92 (through oracle/impute_oracle.py)."""

import numpy as np
import pytest

import masked_noise_cases as MC


def test_the_list_is_the_one_the_device_test_runs():
    shapes = {(c["d"], c["n"], c["r"], c["storage"]) for c in MC.CASES}
    assert shapes == {(700, 60, 3, "f64"), (40, 90, 24, "f64"), (2001, 50, 20, "f64"), (1041, 40, 40, "f64"), (530, 30, 64, "f64"),
                      (MC.BOUND + 1, 24, 10, "f64"), (700, 60, 3, "f32"), (2001, 50, 20, "f32")}
    for d, r in ((700, 3), (40, 24)):
        assert {c["method"] for c in MC.CASES if (c["d"], c["r"], c["storage"]) == (d, r, "f64")} == {"psmf", "rpsmf", "mle_smf"}
    for c in MC.CASES:
        assert {"psmf", "rpsmf"} <= {x["method"] for x in MC.CASES if (x["d"], x["r"], x["storage"]) == (c["d"], c["r"], c["storage"])}
        assert c["passes"] == (1 if c["d"] > MC.BOUND else 2)
    assert MC.BOUND == 16 * 256 * 8 == 32_768 and MC.trips(MC.BOUND) == 1 and MC.trips(MC.BOUND + 1) == 2


@pytest.mark.parametrize("cs", MC.CASES, ids=MC.IDS)
def test_case_by_the_oracle_alone(cs):
    pb, ref = MC.reference(cs)
    d, n = cs["d"], cs["n"]
    M, rho = pb["M"], pb["rho"]
    # the builder
    assert not M[3].any() and (M[:, 5].sum() == 0) == (cs["method"] != "mle_smf")
    assert 0.5 < M.mean() < 0.65 and rho.shape == (d,) and rho.min() >= 1.0 and rho.max() <= 100.0 and rho.max() / rho.min() > 50.0
    # (4) the second-trip column
    if MC.trips(d) >= 2:
        col = M[:, MC.SECOND_TRIP_COLUMN]
        assert d == MC.BOUND + 1 and not col[:MC.BOUND].any() and col[MC.BOUND:].all()
    # (1) finite
    for k, v in ref.items():
        assert np.all(np.isfinite(v)), k
    # (2) the weights matter
    flat = MC.run_oracle(cs, pb, float(rho.mean()))
    moved = {k: MC.relerr(flat[k], ref[k]) for k in MC.COMPARED}
    # (3) conditioning: a few ulp on C0 and X0
    pert = MC.run_oracle(cs, MC.problem(cs, perturb=(d + n, 4 * 2.0 ** -52)), rho)
    cond = {k: MC.relerr(pert[k], ref[k]) for k in MC.COMPARED}
    print(f"\nrow-noise case {cs['d']}x{cs['n']} r={cs['r']} {cs['method']} {cs['storage']}: against mean(rho) {moved}; a few ulp on C0, X0 {cond}")
    assert moved["X"] > 1e-2, moved
    assert max(cond.values()) <= 1e-11, cond
