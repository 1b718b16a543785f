"""The net of tests/pmf_net_cases.py is fit to judge the device by: admission, coverage and the extended-precision model, decided by
the references alone.  CPU only; a few seconds.

Admission (pmf_net_cases.admissible, recomputed here for every case with netlib.resolve and compared with the recorded RESOLUTION):
the extended model finite with max |W|, |P| <= 10, its response to a last-bit change of the inputs and the float64 model's distance
from it both 16 x inside pmf_cases.TOL.  At most one case in ten may need a salt other than 0.
Coverage, by counting over the cases as the device runs them: every walked d, r, n and num_batches of the module's docstring, the
workgroup geometries, the drawn sets, the structure of the masks.
The model: dtype=np.longdouble reproduces the float64 model on the list of tests/pmf_cases.py within its ADMIT_TOL, and dtype=float
gives the bits pmf_cases.reference holds."""

from collections import Counter

import numpy as np
import pytest

import pmf_cases as PC
import pmf_model
import pmf_net_cases as NC

assert np.finfo(np.longdouble).eps < 1.1e-19, "these tests need an 80-bit long double: the extended model is no reference without it"

CASES = [NC.device_case(i) for i in range(NC.N_CASES)]


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
    assert all(cs["epsilon"] == (NC.WALK[cs["no"]][4].get("epsilon", NC.EPSILON0)) / 5.0 ** cs["shortened"] for cs in CASES)


def test_the_walked_sets():
    assert [NC.row_tiles(d) for d in (1, 32, 33, 128, 129, 256, 257, 512)] == [2, 2, 8, 8, 16, 16, 32, 32]
    assert {cs["d"] for cs in CASES} >= set(NC.D_EDGES) and set(NC.D_EDGES) >= {1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512}
    assert {cs["n"] for cs in CASES} >= set(NC.N_EDGES) and set(NC.N_EDGES) >= {1, 2, 15, 16, 17, 31, 33, 63, 64, 65}
    per_r = Counter(cs["r"] for cs in CASES)
    assert all(per_r[r] >= 2 for r in range(1, 17)), per_r
    for r in NC.NK_EDGES:
        assert len({NC.row_tiles(cs["d"]) for cs in CASES if cs["r"] == r}) >= 2, r
    assert set(NC.NK_EDGES) == {4, 5, 8, 9, 12, 13}
    assert {cs["nb"] for cs in CASES} == set(NC.NB_LIST) == {1, 2, 9, 254}
    assert all(cs["n"] <= 300 and cs["d"] * cs["n"] <= 20000 and 1 <= cs["d"] <= 512 for cs in CASES)
    assert Counter(NC.row_tiles(cs["d"]) for cs in CASES).keys() == {2, 8, 16, 32}


def test_the_limit_of_254_batches_and_the_tightest_split():
    big = [cs for cs in CASES if cs["nb"] == 254]
    assert big
    for cs in big:
        N = NC.problem(cs)["M"].reshape(cs["batch"], -1).sum(axis=1)
        assert np.all(N >= 16 * 254), N
    tight = [cs for cs in CASES if cs["tight"]]
    assert tight and all(cs["epsilon"] <= 2.0 for cs in tight)
    for cs in tight:
        assert all(int(m.sum()) == cs["nb"] + 1 for m in NC.problem(cs)["M"])


def test_the_workgroup_geometries():
    """per instance: PSMF_PMF_COLS = 16 on 50 <= n <= 100 with a partial last tile; more than one workgroup with more than one tile
    per wave; the library's own choice of columns giving two workgroups on the four-wave and on the one-wave kernel"""
    for nt in (2, 8, 16, 32):
        mine = [cs for cs in CASES if NC.row_tiles(cs["d"]) == nt]
        c16 = [cs for cs in mine if cs["cols"] == 16 and 50 <= cs["n"] <= 100 and cs["n"] % 16]
        assert c16 and all(NC.geometry(cs)[1] == -(-cs["n"] // 16) > 1 for cs in c16), nt
        multi = [cs for cs in mine if NC.geometry(cs)[1] > 1 and NC.geometry(cs)[2] > 1 and cs["n"] % 16]
        assert multi, nt
    own = [cs for cs in CASES if not cs["cols"] and NC.geometry(cs)[1] > 1]
    assert {NC.waves(NC.row_tiles(cs["d"])) for cs in own} == {1, 4}
    assert NC.geometry(dict(d=20, n=300, cols=0)) == (256, 2, 4) and NC.geometry(dict(d=257, n=77, cols=0)) == (64, 2, 4)
    assert NC.geometry(dict(d=260, n=70, cols=32)) == (32, 3, 2) and NC.geometry(dict(d=30, n=100, cols=80)) == (80, 2, 2)


def test_the_drawn_sets_and_the_masks():
    assert {cs["lmd"] for cs in CASES} == set(NC.LMDS) == {0.0, 0.01, 0.3}
    assert {cs["momentum"] for cs in CASES} == set(NC.MOMENTA) == {0.0, 0.8, 0.95}
    assert {cs["epochs"] for cs in CASES} == {1, 2, 3} and {cs["batch"] for cs in CASES} == {1, 2, 3, 4}
    assert len({(cs["lmd"], cs["momentum"]) for cs in CASES}) >= 7, "lmd and momentum vary against each other"
    free = [cs for cs in CASES if "native" not in NC.WALK[cs["no"]][4]]
    assert all(0 <= cs["native"] <= 0.5 and 0.05 <= cs["held"] <= 0.4 for cs in free)
    assert min(cs["native"] for cs in free) < 0.1 and max(cs["native"] for cs in free) > 0.4
    assert {cs["epsilon"] for cs in CASES} <= {50.0, 10.0, 2.0} and 50.0 in {cs["epsilon"] for cs in CASES}
    negative = [cs for cs in CASES if cs["offset"] < 0]
    assert len(negative) >= 5 and len({NC.row_tiles(cs["d"]) for cs in negative}) == 4
    full = one = empty = 0
    for cs in CASES:
        pb = NC.problem(cs)
        M, Mm = pb["M"] != 0, pb["Mmiss"] != 0
        B, d, n = M.shape
        assert all(M[b].sum() >= cs["nb"] + 1 and Mm[b].any() for b in range(B)), cs["name"]
        assert np.all(pb["YorgInt"][M.any(axis=0)] != 0) and all(len(p) == cs["epochs"] for p in pb["perms"])
        assert all(np.array_equal(np.sort(p), np.arange(M[b].sum())) for b in range(B) for p in pb["perms"][b])
        if B > 1 and d * n >= 64:
            assert all(not np.array_equal(M[b], M[b + 1]) for b in range(B - 1)), cs["name"]
        if cs["offset"] < 0:
            assert all(ref["mean"] < 0 for ref in NC.reference(cs["no"])[3])
        if cs["full"]:
            full += 1
            assert all(M[b, d // 2].all() and M[b, :, n // 2].all() for b in range(B)), cs["name"]
        elif n >= 5 + B and d >= 3:
            empty += 1
            for b in range(B):
                cols, rows = np.flatnonzero(~M[b].any(axis=0)), np.flatnonzero(~M[b].any(axis=1))
                assert rows.size and cols.size, cs["name"]
                assert any(Mm[b][:, c].any() for c in cols) or cs["one_probe"], cs["name"]
        if cs["one_probe"]:
            one += 1
            assert Mm[0].sum() == 1, cs["name"]
    print(f"\n{full} cases with a fully observed row and column, {empty} with a row and a column without a training entry, {one} with a single probe entry")
    assert full >= 3 and one >= 3 and empty >= 25


@pytest.mark.parametrize("i", range(len(PC.CASES)), ids=[c["name"] for c in PC.CASES])
def test_the_extended_model_reproduces_the_float64_one_and_float_keeps_its_bits(i):
    pb, cs = PC.problem(i), PC.CASES[i]
    worst = 0.0
    for b, ref in enumerate(PC.reference(i)):
        args = (pb["YorgInt"], pb["M"][b], pb["Mmiss"][b], pb["C0"][b], pb["X0"][b], pb["perms"][b])
        kw = dict(epochs=cs["epochs"], epsilon=cs["epsilon"], lmd=PC.LMD, momentum=PC.MOMENTUM, num_batches=cs["nb"])
        same = pmf_model.pmf_model(*args, dtype=float, **kw)
        assert all(np.array_equal(same[k], ref[k]) and np.asarray(same[k]).dtype == np.float64 for k in PC.KEYS + ("mean", "mean_rating"))
        ext = pmf_model.pmf_model(*args, dtype=np.longdouble, **kw)
        assert all(np.asarray(ext[k]).dtype == np.longdouble for k in PC.KEYS + ("mean", "mean_rating"))
        worst = max(worst, NC.distance(ref, ext))
    print(f"\n{cs['name']}: the float64 model is within {worst:.2e} of the extended one")
    assert worst <= PC.ADMIT_TOL


def test_the_extended_model_is_not_the_float64_one():
    """the long-double run carries more than float64: its answers do not survive a round trip through float64"""
    ext = NC.reference(5)[2][0]
    assert np.any(ext["P"].astype(np.float64).astype(np.longdouble) != ext["P"])
