"""psmf_bpmf_run / rpsmf_amd.bpmf on the device: the batched BPMF baseline (rpsmf_amd/csrc/psmf_bpmf.hip) against the numpy model of
tests/bpmf_model.py on the cases of tests/bpmf_cases.py, and against the answers the reference stores.

Bars: Efull within bpmf_cases.TOL relative, epoch by epoch; C, X and Yrec within it in conftest.relerr.  TOL = 4.85e-12 is 50 x what
the model's own algebras and summation orders part by on the CPU (9.7e-14, in P; tests/bpmf_cases.py), and the device is free in
nothing else.  A device result beyond the bar is a finding to explain, not a tolerance to raise.  The stored answers (error_full of
ExperimentImpute/output/*_BPMF.json): the same bar.  Every case runs once per module with the reconstruction returned; the other
tests share those runs."""

from functools import lru_cache

import numpy as np
import pytest

import bpmf_cases as BC
from conftest import load_golden, relerr
from netlib import env
from rpsmf_amd import impute_harness as H

pytestmark = pytest.mark.gpu

ERR_NUMERIC = -4
OUT_KEYS = ("Efull", "C", "X", "Yrec", "mean", "mean_rating", "status")


def _run(pb, cs, **kw):
    from rpsmf_amd.bpmf import bpmf_batch

    return bpmf_batch(*BC.device_args(pb), **{**BC.device_kwargs(cs), "want_rec": True, **kw})


@lru_cache(maxsize=None)
def _device(i):
    return _run(BC.problem(i), BC.CASES[i])


def _errors(res, b, ref):
    return dict(Efull=float(np.max(np.abs(res["Efull"][b] - ref["Efull"]) / np.abs(ref["Efull"]))), C=relerr(res["C"][b], ref["P"]),
                X=relerr(res["X"][b], ref["W"].T), Yrec=relerr(res["Yrec"][b], ref["Yrec"]))


def _check(res, i, what):
    cs = BC.CASES[i]
    assert list(res["status"]) == [0] * cs["batch"]
    assert res["Efull"].shape == (cs["batch"], cs["epochs"]) and res["C"].shape == (cs["batch"], cs["d"], cs["r"])
    assert res["X"].shape == (cs["batch"], cs["r"], cs["n"]) and res["Yrec"].shape == (cs["batch"], cs["d"], cs["n"])
    worst = {}
    for b, ref in enumerate(BC.reference(i)):
        assert res["mean"][b] == ref["mean"] and res["mean_rating"][b] == ref["mean_rating"], "mu and mbar carry numpy's bits"
        assert np.array_equal(res["Yrec"][b] != 0, BC.problem(i)["Mmiss"][b] != 0), "Yrec is set at the probe entries and nowhere else"
        worst = {k: max(worst.get(k, 0.0), v) for k, v in _errors(res, b, ref).items()}
    print(f"\nbpmf {cs['name']} {what}: worst over the replicas {worst}; {res['elapsed_ms']:.3f} ms")
    assert all(v <= BC.TOL for v in worst.values()), worst


@pytest.mark.parametrize("i", range(len(BC.CASES)), ids=[c["name"] for c in BC.CASES])
def test_every_case_against_the_model(i):
    _check(_device(i), i, "default columns")


def _cols_for(n, wgs):
    """a PSMF_BPMF_COLS that gives `wgs` workgroups per replica (the library rounds it up to a multiple of 4)"""
    cols = -(-(-(-n // wgs)) // 4) * 4
    assert -(-n // cols) == wgs, (n, wgs, cols)
    return cols


@pytest.mark.parametrize("wgs", (1, 3, 35))
@pytest.mark.parametrize("i", BC.COLS_CASES, ids=[BC.CASES[i]["name"] for i in BC.COLS_CASES])
def test_columns_per_workgroup(i, wgs):
    """PSMF_BPMF_COLS (read at every call) forcing 1, 3 and 35 workgroups per replica, where the default gives 11 and 47: the
    partial sums of the row sweep and of the covariance of W are cut elsewhere, within the same bars"""
    cols = _cols_for(BC.CASES[i]["n"], wgs)
    with env({"PSMF_BPMF_COLS": str(cols)}):
        res = _run(BC.problem(i), BC.CASES[i])
    _check(res, i, f"PSMF_BPMF_COLS={cols} ({wgs} workgroups per replica)")
    # an odd setting is rounded up to the four columns of a wave: the same workgroups, the same bits
    with env({"PSMF_BPMF_COLS": str(cols - 3)}):
        again = _run(BC.problem(i), BC.CASES[i])
    assert all(np.array_equal(res[k], again[k]) for k in OUT_KEYS)


def test_replicas_per_chunk_change_no_bit():
    """PSMF_BPMF_CHUNK (read at every call): 4 replicas in chunks of 1 and of 3 (the last one partial)"""
    i = BC.COLS_CASES[1]
    whole = _device(i)
    for chunk in ("1", "3"):
        with env({"PSMF_BPMF_CHUNK": chunk}):
            res = _run(BC.problem(i), BC.CASES[i])
        assert all(np.array_equal(res[k], whole[k]) for k in OUT_KEYS), chunk


@pytest.mark.parametrize("i", (2, 6), ids=[BC.CASES[i]["name"] for i in (2, 6)])
def test_same_bits_twice_and_alone(i):
    first = _device(i)
    pb, cs = BC.problem(i), BC.CASES[i]
    again = _run(pb, cs)
    assert all(np.array_equal(first[k], again[k], equal_nan=True) for k in OUT_KEYS), "the same call twice gives the same bits"
    b = cs["batch"] - 1
    alone = _run(dict(pb, M=pb["M"][b], Mmiss=pb["Mmiss"][b], C0=pb["C0"][b], X0=pb["X0"][b], draws=[pb["draws"][b]]), cs)
    assert all(np.array_equal(first[k][b], alone[k][0]) for k in OUT_KEYS), "a replica alone has the bits it has inside a batch"


def test_a_replica_that_is_not_positive_definite_is_marked_and_leaves_its_neighbour_alone():
    """replica 0 is handed Bartlett factors of zeros (a numerical refusal: alpha = 0, a zero pivot); the reference raises LinAlgError"""
    pb, cs = BC.nonspd()
    res = _run(pb, cs)
    assert list(res["status"]) == [ERR_NUMERIC, 0]
    healthy = _device(cs["i"])
    assert all(np.array_equal(res[k][1], healthy[k][1]) for k in OUT_KEYS), "the healthy replica has the bits it has without the bad one"
    err = _errors(res, 1, BC.reference(cs["i"])[1])
    assert all(v <= BC.TOL for v in err.values()), err


@pytest.mark.parametrize("ds,pct", BC.KAT_FILES, ids=[f"{ds}_{pct}" for ds, pct in BC.KAT_FILES])
def test_stored_answers_through_bpmf_batch(ds, pct):
    """error_full of the first 5 repeats of <ds>_<pct>_BPMF.json, the five as one batch with the draws handed over"""
    from rpsmf_amd.bpmf import bpmf_batch

    want = load_golden("impute_kat_bpmf")[f"{ds}_{pct}_error_full"][:5]
    dr = BC.kat_inputs(ds, pct, 5)
    res = bpmf_batch(dr[0]["YorigInt"], np.stack([x["M"] for x in dr]), np.stack([x["Mmiss"] for x in dr]), np.stack([x["C"] for x in dr]),
                     np.stack([x["X"] for x in dr]), [x["draws"] for x in dr], epochs=BC.KAT_EPOCHS)
    err = np.abs(res["Efull"][:, -1] - want) / np.abs(want)
    print(f"\nbpmf {ds}_{pct}: stored error_full {want}, device off by {err}; {res['elapsed_ms']:.3f} ms")
    assert list(res["status"]) == [0] * 5 and np.all(err <= BC.TOL), err


def test_stored_answers_through_bpmf_as_the_script_calls_it():
    """BPMF.py:305-375 with rpsmf_amd.bpmf.bpmf in the place of its function: seed 123, per repeat the draw, the RNG state saved, the
    call, the state restored.  The first 3 repeats of LondonAir_PM25 at 20 %."""
    import kat_replay
    from rpsmf_amd.bpmf import bpmf

    g = load_golden("impute_kat_bpmf")
    Yorig = kat_replay.fixture("pm25")["Yorig"]
    YorigInt = np.nan_to_num(Yorig, nan=0.0)
    d, n = Yorig.shape
    keep = np.random.get_state()
    np.random.seed(123)
    got = []
    for k in range(3):
        pb = H.draw_problem(Yorig, 20, BC.KAT_R)
        assert H.matrix_hash(pb["C"]) == str(g["pm25_20_hash_C"][k])
        Einit = H.RMSEM(pb["C"] @ pb["X"], YorigInt, pb["Mmiss"])
        state = np.random.get_state()
        ep, ef, rt = bpmf(pb["Y"], pb["C"], pb["X"], d, n, BC.KAT_R, pb["M"], pb["Mmiss"], YorigInt, Einit, epochs=BC.KAT_EPOCHS)
        np.random.set_state(state)
        assert ep.shape == ef.shape == rt.shape == (1, BC.KAT_EPOCHS + 1)
        assert ep[0, 0] == ef[0, 0] == Einit and np.all(np.isnan(ep[0, 1:])) and rt[0, 0] == 0 and np.all(np.diff(rt[0]) > 0)
        got.append(ef[0, BC.KAT_EPOCHS])
    np.random.set_state(keep)
    want = g["pm25_20_error_full"][:3]
    err = np.abs(np.array(got) - want) / np.abs(want)
    print(f"\nbpmf() as the script calls it, pm25 at 20 %: device off the stored error_full by {err}")
    assert np.all(err <= BC.TOL), err


def test_bpmf_raises_linalgerror_for_a_numeric_status(monkeypatch):
    """what BPMF.py:363-373 catches: bpmf() turns the replica's status into numpy.linalg.LinAlgError"""
    from rpsmf_amd import bpmf as mod

    pb, cs = BC.nonspd()
    monkeypatch.setattr(mod, "draw_bpmf", lambda *a: pb["draws"][0])
    M, Mm, C0, X0 = (np.array(pb[k][0]) for k in ("M", "Mmiss", "C0", "X0"))
    with pytest.raises(np.linalg.LinAlgError):
        mod.bpmf(pb["YorgInt"] * M, C0, X0, cs["d"], cs["n"], cs["r"], M, Mm, pb["YorgInt"], 1.5, epochs=cs["epochs"])


def test_arguments_are_unmodified_and_the_rng_moves_as_the_model_s_draws():
    from rpsmf_amd.bpmf import bpmf, bpmf_batch, draw_bpmf

    i = 3
    pb, cs = BC.problem(i), BC.CASES[i]
    args = [np.array(a, copy=True) for a in BC.device_args(pb)[:5]]
    draws = [{k: ([p.copy() for p in v] if k == "perms" else v.copy()) for k, v in rep.items()} for rep in pb["draws"]]
    res = bpmf_batch(*args, draws, **BC.device_kwargs(cs))
    assert all(np.array_equal(a, b) for a, b in zip(args, BC.device_args(pb)[:5]))
    for rep, orig in zip(draws, pb["draws"]):
        assert all(np.array_equal(p, q) for p, q in zip(rep["perms"], orig["perms"]))
        assert all(np.array_equal(rep[k], orig[k]) for k in ("bartlett", "hyper_normals", "normals"))
    assert np.array_equal(res["Efull"], _device(i)["Efull"]) and "Yrec" not in res

    M, Mm, C0, X0 = (np.array(pb[k][0], copy=True) for k in ("M", "Mmiss", "C0", "X0"))
    Y = pb["YorgInt"] * M
    keep = np.random.get_state()
    np.random.seed(99)
    drawn = draw_bpmf(cs["d"], cs["n"], cs["r"], int(M.sum()), cs["epochs"])
    after_model = np.random.get_state()
    np.random.seed(99)
    ep, ef, rt = bpmf(Y, C0, X0, cs["d"], cs["n"], cs["r"], M, Mm, pb["YorgInt"], 1.5, epochs=cs["epochs"])
    after_bpmf = np.random.get_state()
    np.random.set_state(keep)
    assert after_bpmf[0] == after_model[0] and np.array_equal(after_bpmf[1], after_model[1]) and after_bpmf[2:] == after_model[2:]
    assert np.array_equal(M, pb["M"][0]) and np.array_equal(Mm, pb["Mmiss"][0]) and np.array_equal(C0, pb["C0"][0]) and np.array_equal(X0, pb["X0"][0])
    ref = BC.run_model(pb, 0, cs, draws=drawn)
    assert np.max(np.abs(ef[0, 1:] - ref["Efull"]) / np.abs(ref["Efull"])) <= BC.TOL
