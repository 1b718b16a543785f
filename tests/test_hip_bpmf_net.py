"""psmf_bpmf_run on the seeded net of tests/bpmf_net_cases.py, against the extended-precision model (tests/bpmf_model.py with
dtype=np.longdouble in the factor form), which tests/test_bpmf_net_cases_cpu.py admits.  Two families: the whole engine (bpmf_batch:
warm start and sweeps) over d and n below, at and above the 4 rows of a matrix-core product and the 4 and 16 columns of a wave and a
workgroup, every r, up to 5 epochs, beta 0.5 .. 20, 17 workgroups and 2 with a single column in the last; and the sampler alone
(rpsmf_amd.bpmf._sweeps on drawn factors with per-feature scales over three decades and beta up to 100: ill-conditioned precision
matrices, which PMF's warm start never hands it).

Bars, those of tests/test_hip_bpmf.py (bpmf_cases.TOL, imported): Efull within it relative, epoch by epoch; C, X and Yrec within it
in conftest.relerr; mu and mbar with numpy's bits; Yrec non-zero exactly at the probe entries; status 0 everywhere.  One device call
per case, shared by the tests.  A device result beyond the bar is a finding to explain and to fix in the kernel, not a tolerance to
raise and not a case to drop."""

from functools import lru_cache

import numpy as np
import pytest

import bpmf_net_cases as NC
from bpmf_cases import TOL
from conftest import relerr
from netlib import env

pytestmark = pytest.mark.gpu

OUT_KEYS = ("Efull", "C", "X", "Yrec", "mean", "mean_rating", "status")
SMALL_N_CASE = 27      # 17 x 4, four replicas: a wave's four columns are the whole replica

assert np.finfo(np.longdouble).eps < 1.1e-19, "these tests need an 80-bit long double: the extended model is no reference without it"


def _sampler_alone(cs, pb):
    """psmf_bpmf_run on the case's own factors: pmf's host preparation for the layouts and the means, no warm start"""
    from rpsmf_amd import bpmf, pmf

    draws = pb["draws"]
    h = pmf._prepare(pb["YorgInt"], pb["M"], pb["Mmiss"], pb["C0"], pb["X0"], [dr["perms"] for dr in draws], cs["epochs"], 1)
    h["Mt"] = np.ascontiguousarray(np.transpose(pb["M"] != 0, (0, 2, 1)).astype(np.uint8))
    warm = dict(C=np.array(pb["P0"], dtype=np.float64, order="C"), X=np.ascontiguousarray(np.transpose(pb["W0"], (0, 2, 1))), mean=h["mean"],
                mean_rating=h["mbar"], elapsed_ms=0.0)
    return bpmf._sweeps(h, warm, draws, cs["beta"], 0, True)


def _run(no, extra_env=None):
    from rpsmf_amd.bpmf import bpmf_batch

    cs, pb = NC.reference(no)[:2]
    with env({**NC.device_env(cs), **(extra_env or {})}):
        if cs["family"] == "sampler":
            return _sampler_alone(cs, pb)
        return bpmf_batch(pb["YorgInt"], pb["M"], pb["Mmiss"], pb["C0"], pb["X0"], pb["draws"], epochs=cs["epochs"], beta=cs["beta"],
                          warm_start=NC.warm_start(cs, pb), want_rec=True)


@lru_cache(maxsize=None)
def _device(no):
    return _run(no)


@lru_cache(maxsize=None)
def _errors(no):
    """(the device's worst error over the replicas of case `no` against the extended model, the float64 model's distance from it);
    asserts what is exact"""
    cs, pb, ext, f64 = NC.reference(no)
    res = _device(no)
    B, d, n, r = cs["batch"], cs["d"], cs["n"], cs["r"]
    assert list(res["status"]) == [0] * B
    assert res["Efull"].shape == (B, cs["epochs"]) and res["C"].shape == (B, d, r) and res["X"].shape == (B, r, n) and res["Yrec"].shape == (B, d, n)
    worst, model = dict(Efull=0.0, C=0.0, X=0.0, Yrec=0.0), 0.0
    for b in range(B):
        assert res["mean"][b] == f64[b]["mean"] and res["mean_rating"][b] == f64[b]["mean_rating"], "mu and mbar carry numpy's bits"
        assert np.array_equal(res["Yrec"][b] != 0, pb["Mmiss"][b] != 0), "Yrec is set at the probe entries and nowhere else"
        err = dict(Efull=float(np.max(np.abs(res["Efull"][b] - ext[b]["Efull"]) / np.abs(ext[b]["Efull"]))), C=relerr(res["C"][b], ext[b]["P"]),
                   X=relerr(res["X"][b], ext[b]["W"].T), Yrec=relerr(res["Yrec"][b], ext[b]["Yrec"]))
        worst = {k: max(worst[k], err[k]) for k in worst}
        model = max(model, NC.distance(f64[b], ext[b]))
    return worst, model


@pytest.mark.parametrize("no", range(NC.N_CASES), ids=[NC.device_case(i)["name"] for i in range(NC.N_CASES)])
def test_every_case_against_the_extended_model(no):
    worst, model = _errors(no)
    cs = NC.reference(no)[0]
    print(f"\nbpmf {NC.describe(cs)} (columns, workgroups) = {NC.geometry(cs)}: device {worst}; the float64 model is {model:.2e} from the "
          f"extended one; {_device(no)['elapsed_ms']:.3f} ms")
    assert all(v <= TOL for v in worst.values()), worst


def test_worst_error_per_family():
    """the summary of the net: per family, the worst error as a share of the bar"""
    for family in NC.FAMILIES:
        nos = [i for i in range(NC.N_CASES) if NC.device_case(i)["family"] == family]
        assert nos
        worst = {k: max(_errors(no)[0][k] for no in nos) for k in ("Efull", "C", "X", "Yrec")}
        model = max(_errors(no)[1] for no in nos)
        top = max(worst.values())
        print(f"\nbpmf net, family {family} ({len(nos)} cases): worst device error / bar: {top:.2e} / {TOL:g} = {top / TOL:.1e} ({worst}); the "
              f"float64 model's worst distance from the extended one {model:.2e} = {model / TOL:.1e} of the bar")
        assert all(v <= TOL for v in worst.values()), (family, worst)


def test_one_replica_per_chunk_changes_no_bit_at_four_columns():
    """PSMF_BPMF_CHUNK = 1 (read at every call) on a case with n <= 4: four chunks of one replica"""
    cs = NC.reference(SMALL_N_CASE)[0]
    assert cs["n"] <= 4 and cs["batch"] > 1
    whole, res = _device(SMALL_N_CASE), _run(SMALL_N_CASE, {"PSMF_BPMF_CHUNK": "1"})
    assert all(np.array_equal(res[k], whole[k]) for k in OUT_KEYS)


@pytest.mark.parametrize("no", (10, SMALL_N_CASE, 47), ids=lambda no: NC.device_case(no)["name"])
def test_the_same_call_twice_gives_the_same_bits(no):
    first, again = _device(no), _run(no)
    assert all(np.array_equal(first[k], again[k]) for k in OUT_KEYS)
