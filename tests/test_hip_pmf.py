"""psmf_pmf_run / rpsmf_amd.pmf on the device: the batched PMF baseline (rpsmf_amd/csrc/psmf_pmf.hip) against the numpy model of
tests/pmf_model.py on the cases of tests/pmf_cases.py, and against the answers the reference stores.

Bars: Efull within 1e-12 relative, epoch by epoch; C, X and Yrec within 1e-12 in conftest.relerr.  That is about 400 x what the
result moves when the model sums each batch in another order (2.8e-15 on the CPU; tests/test_pmf_cases_cpu.py admits a case at
1e-13), and the device is free in nothing but the order of its sums.  A device result beyond the bar is a finding to explain, not a
tolerance to raise.  The stored answers (error_full of ExperimentImpute/output/*_PMF.json): 1e-12 relative.  Every case runs once per
module with the reconstruction returned; the other tests share those runs."""

from functools import lru_cache

import numpy as np
import pytest

import pmf_cases as PC
import pmf_model
from conftest import load_golden, relerr
from netlib import env
from rpsmf_amd import impute_harness as H

pytestmark = pytest.mark.gpu

ERR_NUMERIC = -4
OUT_KEYS = ("Efull", "C", "X", "Yrec", "mean", "mean_rating", "status")


def _run(pb, cs, **kw):
    from rpsmf_amd.pmf import pmf_batch

    return pmf_batch(*PC.device_args(pb), **{**PC.device_kwargs(cs), "want_rec": True, **kw})


@lru_cache(maxsize=None)
def _device(i):
    return _run(PC.problem(i), PC.CASES[i])


def _errors(res, b, ref):
    return dict(Efull=float(np.max(np.abs(res["Efull"][b] - ref["Efull"]) / np.abs(ref["Efull"]))), C=relerr(res["C"][b], ref["P"]),
                X=relerr(res["X"][b], ref["W"].T), Yrec=relerr(res["Yrec"][b], ref["Yrec"]))


def _check(res, i, what):
    cs = PC.CASES[i]
    assert list(res["status"]) == [0] * cs["batch"]
    assert res["Efull"].shape == (cs["batch"], cs["epochs"]) and res["C"].shape == (cs["batch"], cs["d"], cs["r"])
    assert res["X"].shape == (cs["batch"], cs["r"], cs["n"]) and res["Yrec"].shape == (cs["batch"], cs["d"], cs["n"])
    worst = {}
    for b, ref in enumerate(PC.reference(i)):
        assert res["mean"][b] == ref["mean"] and res["mean_rating"][b] == ref["mean_rating"], "mu and mbar carry numpy's bits"
        assert np.array_equal(res["Yrec"][b] != 0, PC.problem(i)["Mmiss"][b] != 0), "Yrec is set at the probe entries and nowhere else"
        worst = {k: max(worst.get(k, 0.0), v) for k, v in _errors(res, b, ref).items()}
    print(f"\npmf {cs['name']} {what}: worst over the replicas {worst}; {res['elapsed_ms']:.3f} ms")
    assert all(v <= PC.TOL for v in worst.values()), worst


@pytest.mark.parametrize("i", range(len(PC.CASES)), ids=[c["name"] for c in PC.CASES])
def test_every_case_against_the_model(i):
    _check(_device(i), i, "default columns")


def _cols_for(n, wgs):
    """a PSMF_PMF_COLS that gives `wgs` workgroups per replica (the library rounds it up to a multiple of 16)"""
    cols = -(-(-(-n // wgs)) // 16) * 16
    assert -(-n // cols) == wgs, (n, wgs, cols)
    return cols


@pytest.mark.parametrize("wgs", (1, 2, 3, 9))
@pytest.mark.parametrize("i", PC.COLS_CASES, ids=[PC.CASES[i]["name"] for i in PC.COLS_CASES])
def test_columns_per_workgroup(i, wgs):
    """PSMF_PMF_COLS (read at every call) forcing 1, 2, 3 and 9 workgroups per replica: the same bars"""
    cols = _cols_for(PC.CASES[i]["n"], wgs)
    with env({"PSMF_PMF_COLS": str(cols)}):
        res = _run(PC.problem(i), PC.CASES[i])
    _check(res, i, f"PSMF_PMF_COLS={cols} ({wgs} workgroups per replica)")
    # an odd setting is rounded up to the tile: the same workgroups, the same bits
    with env({"PSMF_PMF_COLS": str(cols - 5)}):
        again = _run(PC.problem(i), PC.CASES[i])
    assert all(np.array_equal(res[k], again[k]) for k in OUT_KEYS)


def test_replicas_per_chunk_change_no_bit():
    """PSMF_PMF_CHUNK (read at every call): 4 replicas in chunks of 1 and of 3 (the last one partial)"""
    i = PC.COLS_CASES[1]
    whole = _device(i)
    for chunk in ("1", "3"):
        with env({"PSMF_PMF_CHUNK": chunk}):
            res = _run(PC.problem(i), PC.CASES[i])
        assert all(np.array_equal(res[k], whole[k]) for k in OUT_KEYS), chunk


@pytest.mark.parametrize("i", (2, 5), ids=[PC.CASES[i]["name"] for i in (2, 5)])
def test_same_bits_twice_and_alone(i):
    first = _device(i)
    pb, cs = PC.problem(i), PC.CASES[i]
    again = _run(pb, cs)
    assert all(np.array_equal(first[k], again[k], equal_nan=True) for k in OUT_KEYS), "the same call twice gives the same bits"
    b = cs["batch"] - 1
    alone = _run(dict(pb, M=pb["M"][b], Mmiss=pb["Mmiss"][b], C0=pb["C0"][b], X0=pb["X0"][b], perms=[pb["perms"][b]]), cs)
    assert all(np.array_equal(first[k][b], alone[k][0]) for k in OUT_KEYS), "a replica alone has the bits it has inside a batch"


def test_a_diverging_replica_is_marked_and_leaves_its_neighbour_alone():
    pb, cs, ref = PC.diverging()
    res = _run(pb, cs)
    assert list(res["status"]) == [ERR_NUMERIC, 0]
    healthy = _device(cs["i"])
    assert all(np.array_equal(res[k][1], healthy[k][1]) for k in OUT_KEYS), "the healthy replica has the bits it has without the bad one"
    err = _errors(res, 1, ref[1])
    assert all(v <= PC.TOL for v in err.values()), err


@pytest.mark.parametrize("ds,pct", PC.KAT_FILES, ids=[f"{ds}_{pct}" for ds, pct in PC.KAT_FILES])
def test_stored_answers_through_pmf_batch(ds, pct):
    """error_full of the first 5 repeats of <ds>_<pct>_PMF.json, the five as one batch with the permutations handed over"""
    from rpsmf_amd.pmf import pmf_batch

    want = load_golden("impute_kat_pmf")[f"{ds}_{pct}_error_full"][:5]
    dr = PC.kat_inputs(ds, pct, 5)
    res = pmf_batch(dr[0]["YorigInt"], np.stack([x["M"] for x in dr]), np.stack([x["Mmiss"] for x in dr]), np.stack([x["C"] for x in dr]),
                    np.stack([x["X"] for x in dr]), [x["perms"] for x in dr], epochs=PC.KAT_EPOCHS)
    err = np.abs(res["Efull"][:, -1] - want) / np.abs(want)
    print(f"\npmf {ds}_{pct}: stored error_full {want}, device off by {err}; {res['elapsed_ms']:.3f} ms")
    assert list(res["status"]) == [0] * 5 and np.all(err <= PC.TOL), err


def test_stored_answers_through_pmf_as_the_script_calls_it():
    """PMF.py:162-228 with rpsmf_amd.pmf.pmf in the place of its function: seed 123, per repeat the draw, the RNG state saved, the
    call, the state restored.  The first 5 repeats of LondonAir_PM25 at 20 %."""
    import kat_replay
    from rpsmf_amd.pmf import pmf

    g = load_golden("impute_kat_pmf")
    Yorig = kat_replay.fixture("pm25")["Yorig"]
    YorigInt = np.nan_to_num(Yorig, nan=0.0)
    d, n = Yorig.shape
    keep = np.random.get_state()
    np.random.seed(123)
    got = []
    for k in range(5):
        pb = H.draw_problem(Yorig, 20, PC.KAT_R)
        assert H.matrix_hash(pb["C"]) == str(g["pm25_20_hash_C"][k])
        Einit = H.RMSEM(pb["C"] @ pb["X"], YorigInt, pb["Mmiss"])
        state = np.random.get_state()
        ep, ef, rt = pmf(pb["Y"], pb["C"], pb["X"], d, n, PC.KAT_R, pb["M"], pb["Mmiss"], YorigInt, Einit, epochs=PC.KAT_EPOCHS)
        np.random.set_state(state)
        assert ep.shape == ef.shape == rt.shape == (1, PC.KAT_EPOCHS + 1)
        assert ep[0, 0] == ef[0, 0] == Einit and np.all(np.isnan(ep[0, 1:])) and rt[0, 0] == 0 and np.all(np.diff(rt[0]) > 0)
        got.append(ef[0, PC.KAT_EPOCHS])
    np.random.set_state(keep)
    want = g["pm25_20_error_full"][:5]
    err = np.abs(np.array(got) - want) / np.abs(want)
    print(f"\npmf() as the script calls it, pm25 at 20 %: device off the stored error_full by {err}")
    assert np.all(err <= PC.TOL), err


def test_arguments_are_unmodified_and_the_rng_moves_as_the_model_s_draws():
    from rpsmf_amd.pmf import pmf, pmf_batch

    i = 3
    pb, cs = PC.problem(i), PC.CASES[i]
    args = [np.array(a, copy=True) for a in PC.device_args(pb)[:5]]
    perms = [[p.copy() for p in rep] for rep in pb["perms"]]
    res = pmf_batch(*args, perms, **PC.device_kwargs(cs))
    assert all(np.array_equal(a, b) for a, b in zip(args, PC.device_args(pb)[:5]))
    assert all(np.array_equal(p, q) for rp, rq in zip(perms, pb["perms"]) for p, q in zip(rp, rq))
    assert np.array_equal(res["Efull"], _device(i)["Efull"]) and "Yrec" not in res

    M, Mm, C0, X0 = (np.array(pb[k][0], copy=True) for k in ("M", "Mmiss", "C0", "X0"))
    Y = pb["YorgInt"] * M
    keep = np.random.get_state()
    np.random.seed(99)
    drawn = pmf_model.draw_perms(int(M.sum()), cs["epochs"])
    after_model = np.random.get_state()
    np.random.seed(99)
    ep, ef, rt = pmf(Y, C0, X0, cs["d"], cs["n"], cs["r"], M, Mm, pb["YorgInt"], 1.5, epochs=cs["epochs"])
    after_pmf = np.random.get_state()
    np.random.set_state(keep)
    assert after_pmf[0] == after_model[0] and np.array_equal(after_pmf[1], after_model[1]) and after_pmf[2:] == after_model[2:]
    assert np.array_equal(M, pb["M"][0]) and np.array_equal(Mm, pb["Mmiss"][0]) and np.array_equal(C0, pb["C0"][0]) and np.array_equal(X0, pb["X0"][0])
    ref = pmf_model.pmf_model(pb["YorgInt"], M, Mm, C0, X0, drawn, epochs=cs["epochs"])
    assert np.max(np.abs(ef[0, 1:] - ref["Efull"]) / np.abs(ref["Efull"])) <= PC.TOL
