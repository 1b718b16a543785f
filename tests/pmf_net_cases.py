"""A seeded net of configurations for the batched PMF baseline (psmf_pmf_run, rpsmf_amd/pmf.py; psmf_pmf_batch_kernel<NT, WAVES, LDSACC>,
rpsmf_amd/csrc/psmf_pmf.hip), judged against the extended-precision model (tests/pmf_model.py with dtype=np.longdouble).  Pure Python:
tests/test_pmf_net_cases_cpu.py admits the list without a GPU, tests/test_hip_pmf_net.py runs it on the device.

WALKED, so that the coverage holds for any seed (`walk`: one row of WALK per case):
    d       both sides of every change of the batch kernel's instance (pmf_row_tiles: NT = 2 / 8 / 16 / 32 row tiles for d <= 32 / 128 /
            256 / 512, the last with its accumulators in LDS and one wave per workgroup) and of the row-tile edge 16 | 17 -- 1, 15, 16,
            17, 31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512
    r       every 1 .. 16 twice at least; 4, 5, 8, 9, 12, 13 -- either side of a change of nk = (r + 3) >> 2, the matrix-core products
            that form S -- on two different instances each
    n       1, 2, 15, 16, 17, 31, 33, 63, 64, 65: below, at and above the 16-column tile, and one tile per wave of a four-wave
            workgroup and then a fifth
    num_batches   1, 2, 9 and the limit 254 (20 x 300 with N >= 16 x 254, epsilon 2); one case with N = num_batches + 1 at epsilon 2
    per instance, PSMF_PMF_COLS = 16 on 50 <= n <= 100: several workgroups per replica, one tile each, the last one partial
    per instance, PSMF_PMF_COLS = 80 (32 on the one-wave instance): more than one workgroup per replica AND more than one tile per wave
            -- 16 columns a workgroup cannot give the second -- again with a partial last tile; and the library's own choice of columns at
            n = 300 (four waves: 256 + 44) and at 257 x 77 (one wave: 64 + 13)
    by case number: every fifth case is the sign family with the offset -40 (mu < 0); every seventh has a fully observed column and a
            fully observed row (and then no empty ones); in every ninth, replica 0 has exactly one probe entry
    n <= 300 and d n <= 20 000 throughout
DRAWN per case (`draw`, from SEED, the case number and the salt): batch 1 .. 4, every replica its own mask, factors and permutations;
    lmd in {0, 0.01, 0.3}; momentum in {0, 0.8, 0.95}; epochs 1 .. 3; the natively missing share, uniform in 0 .. 0.5 (shared by the
    replicas); the held-out share, uniform in 0.05 .. 0.4.  Data as pmf_cases.problem: offset + a rank-3 signal of standard deviation
    6 + unit noise.  Where the shape allows (n >= 5, d >= 3) every replica has a column without a training entry but with a probe
    entry, and a row without a training entry.  epsilon starts at the reference's 50.

ADMISSION, by the references alone (`admissible`): the extended model is finite with max |W|, |P| <= 10 (pmf_cases.ADMIT_MAX); its
response to a last-bit change of YorgInt, C0 and X0 (netlib.perturbed, eps = 2^-52) sits 16 x inside the device's bar pmf_cases.TOL;
the float64 model, in both summation orders, is within bar / 16 of the extended one.  No case is dropped: one that fails runs at
epsilon / 5 (`shorten`, at most twice: 50 -> 10 -> 2; small shapes diverge at 50), then from the next salt.  RESOLUTION holds the
outcome; tests/test_pmf_net_cases_cpu.py recomputes it, and allows a salt other than 0 in at most one case of ten."""

from functools import lru_cache

import numpy as np

import netlib
import pmf_cases as PC
import pmf_model

SEED = 5150
LD = np.longdouble
BAR = PC.TOL
EPS = 2.0 ** -52
KEYS = PC.KEYS
LMDS = (0.0, 0.01, 0.3)
MOMENTA = (0.0, 0.8, 0.95)
EPSILON0 = 50.0
D_EDGES = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512)
N_EDGES = (1, 2, 15, 16, 17, 31, 33, 63, 64, 65)
NK_EDGES = (4, 5, 8, 9, 12, 13)
NB_LIST = (1, 2, 9, 254)

# (d, n, r, num_batches, overrides)
WALK = (
    (1, 40, 1, 1, {}),
    (15, 17, 2, 2, {}),
    (16, 64, 3, 9, {}),
    (17, 63, 4, 9, {}),
    (31, 33, 5, 9, {}),
    (32, 31, 8, 9, {}),
    (33, 65, 9, 9, {}),
    (127, 1, 12, 2, {}),
    (128, 2, 13, 2, {}),
    (129, 15, 4, 9, {}),
    (255, 16, 5, 9, {}),
    (256, 17, 8, 9, {}),
    (257, 31, 9, 9, {}),
    (511, 33, 12, 9, {}),
    (512, 16, 13, 9, {}),
    (20, 300, 6, 254, dict(native=0.1, held=0.1, epsilon=2.0)),        # N about 4800 >= 16 x 254
    (5, 7, 3, 9, dict(tight=True, batch=1, epsilon=2.0)),              # N = num_batches + 1: eight batches of one entry
    (16, 15, 7, 2, {}),
    (17, 16, 10, 1, {}),
    (32, 65, 11, 9, {}),
    (33, 63, 14, 9, {}),
    (128, 64, 15, 9, {}),
    (129, 33, 16, 9, {}),
    (256, 2, 1, 1, {}),
    (257, 1, 2, 1, {}),
    (512, 15, 6, 2, {}),
    (511, 17, 7, 9, {}),
    (255, 31, 10, 9, {}),
    (127, 65, 11, 9, {}),
    (31, 64, 14, 9, {}),
    (15, 63, 15, 9, {}),
    (1, 33, 16, 1, {}),
    (17, 70, 13, 9, dict(cols=16)),
    (100, 90, 12, 9, dict(cols=16)),
    (200, 55, 3, 9, dict(cols=16)),
    (300, 60, 6, 9, dict(cols=16)),
    (30, 100, 8, 9, dict(cols=80)),
    (64, 150, 5, 9, dict(cols=80)),
    (130, 100, 9, 9, dict(cols=80)),
    (260, 70, 4, 9, dict(cols=32)),
    (257, 77, 10, 2, {}),
    (16, 300, 2, 9, {}),
)
N_CASES = len(WALK)


def walk():
    """(d, n, r, num_batches, overrides) of every case, in order"""
    return WALK


def row_tiles(d):
    """pmf_row_tiles of rpsmf_amd/csrc/psmf_pmf.hip: the batch kernel's instance"""
    return 2 if d <= 32 else 8 if d <= 128 else 16 if d <= 256 else 32


def waves(nt):
    return 4 if nt <= 16 else 1


def geometry(cs):
    """(columns per workgroup, workgroups per replica, most tiles a wave takes): pmf_run's choice, PSMF_PMF_COLS included"""
    w = waves(row_tiles(cs["d"]))
    cols = cs["cols"] if cs["cols"] else max(64 * w, (cs["n"] + 63) // 64)
    cols = min((cols + 15) // 16 * 16, (cs["n"] + 15) // 16 * 16)
    nwg = -(-cs["n"] // cols)
    tiles = -(-min(cols, cs["n"]) // 16)
    return cols, nwg, -(-tiles // w)


def draw(no, d, n, r, nb, over, salt=0):
    rng = np.random.default_rng([SEED, no, salt])
    cs = dict(no=no, salt=salt, d=d, n=n, r=r, nb=nb, batch=int(rng.integers(1, 5)), lmd=LMDS[int(rng.integers(3))],
              momentum=MOMENTA[int(rng.integers(3))], epochs=int(rng.integers(1, 4)), native=float(rng.uniform(0.0, 0.5)),
              held=float(rng.uniform(0.05, 0.4)), epsilon=EPSILON0, shortened=0, cols=0, tight=False)
    cs["offset"] = -40.0 if no % 5 == 3 else 40.0
    cs["full"] = no % 7 == 2 and d >= 2 and n >= 2
    cs["one_probe"] = no % 9 == 4
    cs.update(over)
    if cs["tight"]:
        cs["full"] = False
    cs["name"] = f"net{no:02d}-{d}x{n}_r{r}_nb{nb}"
    return cs


def case(i, salt=0):
    return draw(i, *WALK[i], salt=salt)


def shorten(cs):
    """the same case at a fifth of the step size; None after two"""
    if cs["shortened"] >= 2:
        return None
    return dict(cs, epsilon=cs["epsilon"] / 5.0, shortened=cs["shortened"] + 1)


def describe(cs):
    return (f"{cs['name']} x{cs['batch']} e{cs['epochs']} epsilon={cs['epsilon']:g} lmd={cs['lmd']:g} momentum={cs['momentum']:g} "
            f"native={cs['native']:.2f} held={cs['held']:.2f} offset={cs['offset']:g}")


def masks(cs, rng, least):
    """YorgInt (d, n) and M, Mmiss (batch, d, n) uint8 of a case, drawn from `rng`; every replica keeps `least` training entries and a
    probe entry at least (with cs["tight"], exactly `least` training entries).  Shared with tests/bpmf_net_cases.py."""
    d, n, B = cs["d"], cs["n"], cs["batch"]
    sig = rng.standard_normal((d, 3)) @ rng.standard_normal((3, n))
    sig *= 6.0 / max(float(sig.std()), 1e-12)
    Y = cs["offset"] + sig + rng.standard_normal((d, n))
    native = rng.random((d, n)) < cs["native"]
    empty_col, empty_row = n >= 5 and not cs["full"], d >= 3 and not cs["full"]
    empty_col = empty_col and n // 2 + B <= n
    if empty_col:
        native[0, n // 2:n // 2 + B] = False          # the probe entries of the columns without a training entry
    if cs["full"]:
        native[d // 2, :] = False
        native[:, n // 2] = False
    YorgInt = np.where(native, 0.0, Y)
    M = np.zeros((B, d, n), dtype=np.uint8)
    Mmiss = np.zeros((B, d, n), dtype=np.uint8)
    for b in range(B):
        held = (rng.random((d, n)) < cs["held"]) & ~native
        if cs["full"]:
            held[d // 2, :] = False                   # a fully observed row and a fully observed column
            held[:, n // 2] = False
        m = ~native & ~held
        if empty_col:
            c = n // 2 + b                            # a column without a training entry, but with a probe entry
            m[:, c] = False
            held[0, c] = True
        if empty_row:
            m[d - 1 - (b % 2), :] = False             # a row without a training entry (it may hold probe entries)
        if cs["one_probe"] and b == 0:
            ii, jj = np.nonzero(held)
            if ii.size == 0:
                ii, jj = np.nonzero(m)
            held[:] = False
            held[ii[0], jj[0]] = True                 # exactly one probe entry; what was held out besides is training data again
            m = ~native & ~held
            if empty_col:
                m[:, n // 2] = False
            if empty_row:
                m[d - 1, :] = False
        if not held.any():                            # (a tiny shape: a probe entry, whatever the draw)
            ii, jj = np.nonzero(m)
            held[ii[0], jj[0]], m[ii[0], jj[0]] = True, False
        while int(m.sum()) < least:                   # (a tiny shape: held-out entries back into the training set, one probe entry stays)
            ii, jj = np.nonzero(held & ~m & ~native)
            assert ii.size > 1, (cs["name"], "the shape has too few entries")
            m[ii[-1], jj[-1]], held[ii[-1], jj[-1]] = True, False
        while cs["tight"] and int(m.sum()) > least:
            ii, jj = np.nonzero(m)
            m[ii[-1], jj[-1]] = False
        M[b], Mmiss[b] = m, held
    return YorgInt, M, Mmiss


def problem(cs, perturb=None):
    """dict(YorgInt (d, n), M, Mmiss (batch, d, n) uint8, C0, X0, perms: per replica a list of `epochs` permutations).  It does not
    depend on epsilon.  `perturb` = eps: YorgInt, C0 and X0 times (1 + eps u), u uniform in [-1, 1]."""
    d, n, r, B = cs["d"], cs["n"], cs["r"], cs["batch"]
    rng = np.random.default_rng([SEED, cs["no"], cs["salt"], 1])
    YorgInt, M, Mmiss = masks(cs, rng, cs["nb"] + 1)
    perms = [[rng.permutation(int(M[b].sum())) for _ in range(cs["epochs"])] for b in range(B)]
    pb = dict(YorgInt=YorgInt, M=M, Mmiss=Mmiss, C0=rng.random((B, d, r)), X0=rng.random((B, r, n)), perms=perms)
    if perturb is not None:
        pb.update(netlib.perturbed({k: pb[k] for k in ("YorgInt", "C0", "X0")}, [SEED, cs["no"], cs["salt"], 2], perturb))
    return pb


def run_model(cs, pb, b, dtype=float, order="reference"):
    return pmf_model.pmf_model(pb["YorgInt"], pb["M"][b], pb["Mmiss"][b], pb["C0"][b], pb["X0"][b], pb["perms"][b], epochs=cs["epochs"],
                               epsilon=cs["epsilon"], lmd=cs["lmd"], momentum=cs["momentum"], num_batches=cs["nb"], order=order, dtype=dtype)


def xrelerr(a, b):
    """conftest.relerr with the difference taken in long doubles: max |a - b| / max |b|"""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), LD(1e-300)))


def distance(res, ref):
    """how far a model's answer `res` is from `ref`: Efull relative epoch by epoch, P, W and Yrec in xrelerr; the worst of them"""
    ef = np.asarray(res["Efull"], dtype=LD) - np.asarray(ref["Efull"], dtype=LD)
    return max([float(np.max(np.abs(ef) / np.abs(np.asarray(ref["Efull"], dtype=LD))))] + [xrelerr(res[k], ref[k]) for k in KEYS if k != "Efull"])


def admissible(cs):
    """(admitted, text): the rule of the module docstring, replica by replica"""
    pb, pp = problem(cs), problem(cs, perturb=EPS)
    size = resp = dist = 0.0
    for b in range(cs["batch"]):
        ext = run_model(cs, pb, b, LD)
        try:
            netlib.require_finite(ext, KEYS, f"replica {b}")
        except FloatingPointError as e:
            return False, str(e)
        size = max(size, float(np.max(np.abs(ext["W"]))), float(np.max(np.abs(ext["P"]))))
        if size > PC.ADMIT_MAX:
            return False, f"max |W|, |P| = {size:.3g} (> {PC.ADMIT_MAX})"
        resp = max(resp, distance(run_model(cs, pp, b, LD), ext))
        dist = max([dist] + [distance(run_model(cs, pb, b, float, o), ext) for o in ("reference", "sorted")])
    ok = bool(resp <= BAR / 16 and dist <= BAR / 16)          # (a NaN in either fails)
    return ok, f"max |W|, |P| = {size:.3g}; response to a last-bit change {resp:.2e}, float64 model within {dist:.2e} (both <= {BAR / 16:.2e})"


def resolve(i):
    """netlib.resolve on this net: ((salt, times shortened), log)"""
    return netlib.resolve(i, case, shorten, admissible, describe)


# What `resolve` answers where it is not (0, 0), {case: (salt, times shortened)}: recorded so that the device test need not run the
# admission; tests/test_pmf_net_cases_cpu.py recomputes every entry and every absence.
RESOLUTION = {0: (0, 1), 2: (0, 1), 3: (0, 1), 4: (0, 1), 7: (0, 1), 9: (0, 1), 22: (0, 1), 32: (0, 1)}


def device_case(i):
    """case i as the net runs it"""
    return netlib.device_case(i, case, shorten, RESOLUTION.get(i, (0, 0)))


@lru_cache(maxsize=None)
def reference(no):
    """(case, problem, the extended model's answer per replica, the float64 model's) of case `no`, computed once and shared: do not
    modify any of it"""
    cs = device_case(no)
    pb = problem(cs)
    B = range(cs["batch"])
    return cs, pb, tuple(run_model(cs, pb, b, LD) for b in B), tuple(run_model(cs, pb, b, float) for b in B)


def device_args(pb):
    return PC.device_args(pb)


def device_kwargs(cs):
    return dict(epochs=cs["epochs"], epsilon=cs["epsilon"], lmd=cs["lmd"], momentum=cs["momentum"], num_batches=cs["nb"])


def device_env(cs):
    """the environment of the case's device call"""
    return {"PSMF_PMF_COLS": str(cs["cols"])} if cs["cols"] else {}
