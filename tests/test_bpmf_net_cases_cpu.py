"""The net of tests/bpmf_net_cases.py is fit to judge the device by: admission, coverage and the extended-precision model, decided
by the references alone.  CPU only; about half a minute.

Admission (bpmf_net_cases.admissible, recomputed here for every case with netlib.resolve and compared with the recorded RESOLUTION):
the extended model finite, its response to a last-bit change of the inputs and the float64 model's distance from it -- both
algebras and both orders; in the sampler-alone family the factor form alone -- 16 x inside bpmf_cases.TOL.  At most one case in ten
may need a salt other than 0.
Coverage, by counting over the cases as the device runs them: every walked d, n, r and the epochs of the module's docstring, the two
workgroup geometries at n = 65, the drawn sets, the ill-conditioning of the sampler-alone family.
The model: dtype=np.longdouble reproduces the float64 model on the list of tests/bpmf_cases.py within its ADMIT_TOL, dtype=float
gives the bits bpmf_cases.reference holds, and the hand-written factorisation and solves agree with numpy.linalg."""

from collections import Counter

import numpy as np
import pytest

import bpmf_cases as BC
import bpmf_model
import bpmf_net_cases as NC

assert np.finfo(np.longdouble).eps < 1.1e-19, "these tests need an 80-bit long double: the extended model is no reference without it"

LD = np.longdouble
CASES = [NC.device_case(i) for i in range(NC.N_CASES)]
FULL = [cs for cs in CASES if cs["family"] == "full"]
SAMPLER = [cs for cs in CASES if cs["family"] == "sampler"]


@pytest.mark.parametrize("i", range(NC.N_CASES))
def test_case_is_admissible_by_the_references_alone(i):
    (salt, shortened), log = NC.resolve(i)
    ok, text = NC.admissible(CASES[i])
    print(f"\n{NC.describe(CASES[i])}: {text}" + "".join(f"\n    not admitted: {line}" for line in log))
    assert (salt, shortened) == NC.RESOLUTION.get(i, (0, 0)), (i, salt, shortened, log)
    assert ok and CASES[i]["salt"] == salt and CASES[i]["shortened"] == shortened


def test_at_most_one_case_in_ten_needs_another_salt():
    print("\nshortened or redrawn (case: (salt, times epsilon / 5)):", NC.RESOLUTION)
    assert all(0 <= i < NC.N_CASES and res != (0, 0) for i, res in NC.RESOLUTION.items())
    assert sum(salt != 0 for salt, _ in NC.RESOLUTION.values()) <= NC.N_CASES // 10
    assert all(cs["epsilon"] == NC.EPSILON0 / 5.0 ** cs["shortened"] for cs in FULL) and all(cs["epsilon"] is None for cs in SAMPLER)


def test_the_walked_sets():
    assert len(FULL) == NC.N_FULL and len(SAMPLER) == NC.N_SAMPLER and 18 <= NC.N_SAMPLER <= 24
    assert {cs["d"] for cs in FULL} >= set(NC.D_EDGES) and set(NC.D_EDGES) >= {2, 3, 4, 5, 15, 16, 17, 511, 512}
    assert {cs["n"] for cs in FULL} >= set(NC.N_EDGES) and set(NC.N_EDGES) >= {2, 3, 4, 5, 15, 16, 17, 63, 64, 65}
    per_r = Counter(cs["r"] for cs in FULL)
    assert all(per_r[r] >= 2 for r in range(2, 17)), per_r
    assert {cs["r"] for cs in SAMPLER} == set(range(2, 17))
    assert {cs["epochs"] for cs in FULL} == {1, 2, 3, 4, 5} and max(cs["epochs"] for cs in SAMPLER) == 5
    at65 = {NC.geometry(cs) for cs in FULL if cs["n"] == 65}
    assert (4, 17) in at65 and (64, 2) in at65, at65          # 17 workgroups and 2, the last with one column
    assert all(2 <= cs["d"] <= 512 and cs["n"] >= 2 and 2 <= cs["r"] <= 16 for cs in CASES)
    shapes = {(cs["d"], cs["n"], cs["r"]) for cs in FULL}          # the shapes the float64 model was seen to admit
    assert shapes >= {(2, 2, 2), (2, 3, 2), (3, 4, 2), (5, 4, 3), (4, 9, 4), (16, 64, 16), (33, 20, 9), (512, 18, 13), (8, 257, 6), (31, 100, 16), (17, 65, 3)}


def test_the_drawn_sets_and_the_masks():
    assert {cs["beta"] for cs in FULL} == set(NC.BETAS) == {0.5, 2.0, 20.0}
    assert {cs["beta"] for cs in SAMPLER} == set(NC.SAMPLER_BETAS) and max(NC.SAMPLER_BETAS) == 100.0
    assert {cs["batch"] for cs in FULL} == {1, 2, 3, 4}
    assert all(0 <= cs["native"] <= 0.5 and 0.05 <= cs["held"] <= 0.4 for cs in CASES)
    assert sum(cs["offset"] < 0 for cs in CASES) >= 8 and sum(cs["full"] for cs in CASES) >= 5 and sum(cs["one_probe"] for cs in CASES) >= 4
    for cs in CASES:
        pb = NC.problem(cs)
        M, Mm = pb["M"] != 0, pb["Mmiss"] != 0
        B, d, n = M.shape
        assert all(M[b].sum() >= 2 and Mm[b].any() for b in range(B)), cs["name"]
        assert 1 <= pb["nb"] <= 9 and pb["nb"] == min(9, max(1, int(M.reshape(B, -1).sum(axis=1).min()) // 8))
        assert all(pb["draws"][b]["normals"].shape == (cs["epochs"], 2, n + d, cs["r"]) for b in range(B))
        if cs["offset"] < 0:
            assert all(ref["mean"] < 0 for ref in NC.reference(cs["no"])[3])
        if cs["full"]:
            assert all(M[b, d // 2].all() and M[b, :, n // 2].all() for b in range(B)), cs["name"]
        elif n >= 5 + B and d >= 3:
            assert all((~M[b].any(axis=0)).any() and (~M[b].any(axis=1)).any() for b in range(B)), cs["name"]
        if cs["one_probe"]:
            assert Mm[0].sum() == 1, cs["name"]


def test_the_sampler_family_is_ill_conditioned_where_the_warm_start_never_is():
    """the spread of the column norms of the factors the sampler starts from: two decades or more in most cases of the sampler-alone
    family, against less than one after PMF's warm start"""
    def spread(F):
        norms = np.sqrt((np.asarray(F, dtype=float) ** 2).sum(axis=0))
        return float(norms.max() / norms.min())

    wide = [max(spread(NC.problem(cs)["P0"][b]) for b in range(cs["batch"])) for cs in SAMPLER if cs["r"] >= 4]
    print(f"\nsampler-alone family: largest / smallest column norm of P0 per case {[f'{w:.3g}' for w in wide]}")
    assert sum(w >= 100 for w in wide) >= len(wide) // 2 and max(wide) >= 500
    cs = FULL[9]
    pb = NC.problem(cs)
    import pmf_model

    ws = pmf_model.pmf_model(pb["YorgInt"], pb["M"][0], pb["Mmiss"][0], pb["C0"][0], pb["X0"][0], pb["draws"][0]["perms"], epochs=cs["epochs"],
                             **NC.warm_start(cs, pb))
    assert spread(ws["P"]) < 10


@pytest.mark.parametrize("i", range(len(BC.CASES)), ids=[c["name"] for c in BC.CASES])
def test_the_extended_model_reproduces_the_float64_one_and_float_keeps_its_bits(i):
    pb, cs = BC.problem(i), BC.CASES[i]
    worst = 0.0
    for b, ref in enumerate(BC.reference(i)):
        args = (pb["YorgInt"], pb["M"][b], pb["Mmiss"][b], pb["C0"][b], pb["X0"][b], pb["draws"][b])
        kw = dict(epochs=cs["epochs"], beta=BC.BETA, warm_start=cs["warm_start"])
        same = bpmf_model.bpmf_model(*args, dtype=float, **kw)
        assert all(np.array_equal(same[k], ref[k]) and np.asarray(same[k]).dtype == np.float64 for k in BC.KEYS + ("mean", "mean_rating"))
        ext = bpmf_model.bpmf_model(*args, dtype=LD, algebra="device", **kw)
        assert all(np.asarray(ext[k]).dtype == LD for k in BC.KEYS + ("mean", "mean_rating"))
        worst = max(worst, NC.distance(ref, ext), NC.distance(bpmf_model.bpmf_model(*args, algebra="device", **kw), ext))
    print(f"\n{cs['name']}: the float64 model (both algebras) is within {worst:.2e} of the extended one")
    assert worst <= BC.ADMIT_TOL


def test_the_hand_written_algebra_agrees_with_numpy_linalg():
    rng = np.random.default_rng(77)
    for r in (1, 2, 7, 16):
        G = rng.standard_normal((5, r, 2 * r))
        L = G @ np.swapaxes(G, 1, 2) + 0.1 * np.eye(r)
        B = rng.standard_normal((5, r, 2))
        U = bpmf_model.revchol(L)
        Ux = bpmf_model.revchol(L.astype(LD))
        assert Ux.dtype == LD and np.all(np.tril(np.asarray(Ux, dtype=float), -1) == 0)
        assert np.max(np.abs(Ux - U)) <= 1e-12 * np.max(np.abs(U))
        assert np.max(np.abs(Ux @ np.swapaxes(Ux, 1, 2) - L)) <= 1e-17 * r * np.max(np.abs(L))      # U U^T = L to long-double accuracy
        for solve, op in ((bpmf_model._solve_upper, lambda u: u), (bpmf_model._solve_upper_t, lambda u: np.swapaxes(u, 1, 2))):
            X = solve(Ux, B.astype(LD))
            assert X.dtype == LD and np.max(np.abs(op(Ux) @ X - B)) <= 1e-15 * np.max(np.abs(X)) * np.max(np.abs(Ux)) * r
            assert np.max(np.abs(X - solve(U, B))) <= 1e-9 * np.max(np.abs(X))
    with pytest.raises(np.linalg.LinAlgError):
        bpmf_model.revchol(np.array([[1.0, 2.0], [2.0, 1.0]], dtype=LD))
    with pytest.raises(AssertionError):
        bpmf_model.bpmf_model(None, None, None, None, None, None, dtype=LD, algebra="reference")


def test_factors_skip_the_warm_start_and_keep_the_means():
    """factors=(W, P) of the warm start's own answer gives the run with the warm start, bit for bit"""
    import pmf_model

    cs = FULL[6]
    pb = NC.problem(cs)
    args = (pb["YorgInt"], pb["M"][0], pb["Mmiss"][0], pb["C0"][0], pb["X0"][0], pb["draws"][0])
    whole = bpmf_model.bpmf_model(*args, epochs=cs["epochs"], beta=cs["beta"], algebra="device", warm_start=NC.warm_start(cs, pb))
    ws = pmf_model.pmf_model(*args[:5], pb["draws"][0]["perms"], epochs=cs["epochs"], **NC.warm_start(cs, pb))
    alone = bpmf_model.bpmf_model(*args, epochs=cs["epochs"], beta=cs["beta"], algebra="device", factors=(ws["W"], ws["P"]))
    assert all(np.array_equal(whole[k], alone[k]) for k in BC.KEYS + ("mean", "mean_rating"))
