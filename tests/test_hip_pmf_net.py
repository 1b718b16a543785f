"""psmf_pmf_run on the seeded net of tests/pmf_net_cases.py: both sides of every change of the batch kernel's instance and of its row
tiles, every r (every count of matrix-core products that form S), column counts below, at and above a tile and a workgroup's four
waves, 1 .. 254 batches, several workgroups per replica with partial last tiles, drawn lmd, momentum, epochs and masks -- against the
extended-precision model (tests/pmf_model.py with dtype=np.longdouble), which tests/test_pmf_net_cases_cpu.py admits.

Bars, those of tests/test_hip_pmf.py (pmf_cases.TOL, imported): Efull within it relative, epoch by epoch; C, X and Yrec within it in
conftest.relerr; mu and mbar with numpy's bits; Yrec non-zero exactly at the probe entries; status 0 everywhere.  One device call per
case, shared by the tests.  A device result beyond the bar is a finding to explain and to fix in the kernel, not a tolerance to
raise and not a case to drop."""

from functools import lru_cache

import numpy as np
import pytest

import pmf_net_cases as NC
from conftest import relerr
from netlib import env
from pmf_cases import TOL

pytestmark = pytest.mark.gpu

OUT_KEYS = ("Efull", "C", "X", "Yrec", "mean", "mean_rating", "status")
LDS_CASE = 40          # 257 x 77, four replicas: the instance with its accumulators in LDS, two workgroups per replica

assert np.finfo(np.longdouble).eps < 1.1e-19, "these tests need an 80-bit long double: the extended model is no reference without it"


def _run(no, extra_env=None):
    from rpsmf_amd.pmf import pmf_batch

    cs, pb = NC.reference(no)[:2]
    with env({**NC.device_env(cs), **(extra_env or {})}):
        return pmf_batch(*NC.device_args(pb), **NC.device_kwargs(cs), want_rec=True)


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
    print(f"\npmf {NC.describe(cs)} NT={NC.row_tiles(cs['d'])} (columns, workgroups, tiles a wave) = {NC.geometry(cs)}: device {worst}; "
          f"the float64 model is {model:.2e} from the extended one; {_device(no)['elapsed_ms']:.3f} ms")
    assert all(v <= TOL for v in worst.values()), worst


def test_worst_error_per_instance():
    """the summary of the net: per instance of the batch kernel, the worst error as a share of the bar"""
    for nt in (2, 8, 16, 32):
        nos = [i for i in range(NC.N_CASES) if NC.row_tiles(NC.device_case(i)["d"]) == nt]
        assert nos
        worst = {k: max(_errors(no)[0][k] for no in nos) for k in ("Efull", "C", "X", "Yrec")}
        model = max(_errors(no)[1] for no in nos)
        top = max(worst.values())
        print(f"\npmf net, NT = {nt} ({len(nos)} cases, d {min(NC.device_case(i)['d'] for i in nos)} .. {max(NC.device_case(i)['d'] for i in nos)}): "
              f"worst device error / bar: {top:.2e} / {TOL:g} = {top / TOL:.1e} ({worst}); the float64 model's worst distance from the "
              f"extended one {model:.2e} = {model / TOL:.1e} of the bar")
        assert all(v <= TOL for v in worst.values()), (nt, worst)


def test_one_replica_per_chunk_changes_no_bit_on_the_lds_instance():
    """PSMF_PMF_CHUNK = 1 (read at every call) on a case of the instance with the accumulators in LDS: four chunks of one replica"""
    cs = NC.reference(LDS_CASE)[0]
    assert NC.row_tiles(cs["d"]) == 32 and cs["batch"] > 1
    whole, res = _device(LDS_CASE), _run(LDS_CASE, {"PSMF_PMF_CHUNK": "1"})
    assert all(np.array_equal(res[k], whole[k]) for k in OUT_KEYS)


@pytest.mark.parametrize("no", (15, LDS_CASE), ids=lambda no: NC.device_case(no)["name"])
def test_the_same_call_twice_gives_the_same_bits(no):
    first, again = _device(no), _run(no)
    assert all(np.array_equal(first[k], again[k]) for k in OUT_KEYS)
