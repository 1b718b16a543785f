"""A seeded net of configurations for the batched BPMF baseline (psmf_bpmf_run, rpsmf_amd/bpmf.py; rpsmf_amd/csrc/psmf_bpmf.hip), judged
against the extended-precision model (tests/bpmf_model.py with dtype=np.longdouble, algebra="device").  Pure Python:
tests/test_bpmf_net_cases_cpu.py admits the list without a GPU, tests/test_hip_bpmf_net.py runs it on the device.  Two families.

THE WHOLE ENGINE (family "full": bpmf_batch, the PMF warm start and then the sweeps) --
WALKED, so that the coverage holds for any seed (`walk`: one row of WALK per case):
    d       2, 3, 4, 5, 15, 16, 17, 511, 512: below, at and above the 4 rows of a matrix-core product and the 16 rows a workgroup of
            the row kernel takes, and the limit
    n       2, 3, 4, 5, 15, 16, 17, 63, 64, 65: at n = 2, 3, 4 a wave's group of four columns is partly or wholly the branch that
            writes identity systems
    r       every 2 .. 16 twice at least: each leaves its own identity padding in the unrolled 16 x 16 factorisation
    epochs  1 .. 5 (the running average of the metric kernel is counted to 6)
    PSMF_BPMF_COLS = 4 on n = 65 (17 workgroups, the last with one column) and the library's choice on n = 65 (two workgroups, the
            second with one column)
    by case number, as tests/pmf_net_cases.py: every fifth case has the offset -40 (mu < 0), every seventh a fully observed column and
            row, in every ninth replica 0 has exactly one probe entry
DRAWN per case (`draw`): batch 1 .. 4, every replica its own mask, factors and draws (rpsmf_amd.bpmf.draw_bpmf from a seeded RNG);
    beta in {0.5, 2, 20}; the natively missing share, uniform in 0 .. 0.5; the held-out share, uniform in 0.05 .. 0.4.  Data and masks
    as pmf_net_cases.masks.  The warm start runs at epsilon = 50 with num_batches = 9 where every replica has 72 training entries,
    and with as many batches of eight entries as the smallest replica fills (one at least) where not: batches of one or two
    entries diverge even at epsilon = 2.

THE SAMPLER ALONE (family "sampler": rpsmf_amd.bpmf._sweeps on factors that are not PMF's; bpmf_model(factors=...)) --
    SAMPLER_WALK gives d, n, r and epochs; W (n x r) and P (d x r) are standard normal times a per-feature scale 10^U(-2, 1), drawn per
    replica and factor; beta walks {0.5, 2, 20, 100}: the precision matrices alpha + beta F^T F are ill-conditioned, which the factors two
    epochs of PMF produce never are.  The inverse-and-Cholesky algebra of the reference (algebra="reference") is not expected to hold
    up there and is not asked to.

ADMISSION, by the references alone (`admissible`): the extended model is finite (no pivot fails); its response to a last-bit change
of YorgInt, C0, X0 (the sampler family: W, P) and the normals (netlib.perturbed, eps = 2^-52) sits 16 x inside the device's bar
bpmf_cases.TOL; the float64 model is within bar / 16 of the extended one in both algebras and both summation orders -- in the sampler
family in algebra="device" alone, both orders.  No case is dropped: a case of the first family that fails runs its warm start at
epsilon / 5 (`shorten`, at most twice: 50 -> 10 -> 2); then, and in the sampler family at once, the next salt.  RESOLUTION holds the
outcome; tests/test_bpmf_net_cases_cpu.py recomputes it, and allows a salt other than 0 in at most one case of ten."""

from functools import lru_cache

import numpy as np

import bpmf_cases as BC
import bpmf_model
import netlib
import pmf_net_cases as PN

# The first seed from 6260 on at which every case is admitted at salt 0 with a factor 4 to spare on both admission figures -- but for the
# most ill-conditioned case of the sampler family (8 x 129, r = 16, beta = 100), which keeps a factor 1.9: the float64 model's distance
# from the extended one was seen to move by 1.6 x between BLAS builds, and the recorded RESOLUTION must hold on all of them.
SEED = 6274
LD = np.longdouble
BAR = BC.TOL
EPS = 2.0 ** -52
KEYS = BC.KEYS
BETAS = (0.5, 2.0, 20.0)
SAMPLER_BETAS = (0.5, 2.0, 20.0, 100.0)
EPSILON0 = 50.0
D_EDGES = (2, 3, 4, 5, 15, 16, 17, 511, 512)
N_EDGES = (2, 3, 4, 5, 15, 16, 17, 63, 64, 65)
FLOAT_VARIANTS = {"full": (("reference", "reference"), ("reference", "reversed"), ("device", "reference"), ("device", "reversed")),
                  "sampler": (("device", "reference"), ("device", "reversed"))}

# (d, n, r, epochs, PSMF_BPMF_COLS or 0)
WALK = (
    (2, 2, 2, 1, 0),
    (2, 3, 2, 2, 0),
    (3, 4, 2, 1, 0),
    (5, 4, 3, 3, 0),
    (4, 9, 4, 2, 0),
    (16, 64, 16, 2, 0),
    (33, 20, 9, 2, 0),
    (512, 18, 13, 1, 0),
    (8, 257, 6, 2, 0),
    (31, 100, 16, 5, 0),
    (17, 65, 3, 5, 4),
    (17, 65, 5, 2, 0),
    (15, 5, 7, 2, 0),
    (3, 15, 8, 3, 0),
    (4, 16, 10, 2, 0),
    (5, 17, 11, 1, 0),
    (15, 63, 12, 2, 0),
    (16, 2, 14, 2, 0),
    (17, 3, 15, 4, 0),
    (511, 4, 4, 2, 0),
    (512, 5, 5, 1, 0),
    (2, 64, 7, 2, 0),
    (3, 63, 8, 1, 0),
    (4, 65, 9, 3, 0),
    (5, 16, 10, 2, 0),
    (15, 15, 11, 2, 0),
    (16, 17, 12, 2, 0),
    (17, 4, 13, 3, 0),
    (511, 3, 14, 1, 0),
    (512, 2, 15, 2, 0),
    (20, 33, 3, 4, 0),
    (9, 30, 6, 2, 0),
)
# (d, n, r, epochs)
SAMPLER_WALK = (
    (2, 2, 2, 1),
    (3, 4, 3, 2),
    (5, 3, 4, 2),
    (16, 5, 5, 1),
    (15, 16, 6, 2),
    (17, 17, 7, 3),
    (4, 63, 8, 2),
    (33, 20, 9, 2),
    (64, 15, 10, 2),
    (100, 31, 11, 1),
    (511, 4, 12, 1),
    (512, 9, 13, 1),
    (20, 65, 14, 2),
    (31, 64, 15, 2),
    (40, 50, 16, 2),
    (8, 129, 16, 2),
    (5, 5, 2, 5),
    (12, 40, 3, 4),
    (25, 25, 13, 2),
    (60, 10, 5, 3),
)
N_FULL, N_SAMPLER = len(WALK), len(SAMPLER_WALK)
N_CASES = N_FULL + N_SAMPLER
FAMILIES = ("full", "sampler")


def walk():
    """(family, d, n, r, epochs, cols) of every case, in order"""
    return [("full",) + w for w in WALK] + [("sampler",) + w + (0,) for w in SAMPLER_WALK]


def geometry(cs):
    """(columns per workgroup, workgroups per replica): bpmf_run's choice, PSMF_BPMF_COLS included"""
    cols = cs["cols"] if cs["cols"] else max(64, (cs["n"] + 63) // 64)
    cols = min((cols + 3) & ~3, (cs["n"] + 3) & ~3)
    return cols, -(-cs["n"] // cols)


def draw(no, family, d, n, r, epochs, cols, salt=0):
    rng = np.random.default_rng([SEED, no, salt])
    sampler = family == "sampler"
    cs = dict(no=no, salt=salt, family=family, d=d, n=n, r=r, epochs=epochs, cols=cols, batch=int(rng.integers(1, 4 if sampler else 5)),
              native=float(rng.uniform(0.0, 0.5)), held=float(rng.uniform(0.05, 0.4)), epsilon=None if sampler else EPSILON0, shortened=0,
              tight=False)
    cs["beta"] = SAMPLER_BETAS[(no - N_FULL) % 4] if sampler else BETAS[int(rng.integers(3))]          # (the sampler family walks them)
    cs["offset"] = -40.0 if no % 5 == 3 else 40.0
    cs["full"] = no % 7 == 2
    cs["one_probe"] = no % 9 == 4
    cs["name"] = f"net{no:02d}-{family}-{d}x{n}_r{r}_e{epochs}"
    return cs


def case(i, salt=0):
    return draw(i, *walk()[i], salt=salt)


def shorten(cs):
    """the same case with its warm start at a fifth of the step size; None after two, and for the sampler alone"""
    if cs["family"] == "sampler" or cs["shortened"] >= 2:
        return None
    return dict(cs, epsilon=cs["epsilon"] / 5.0, shortened=cs["shortened"] + 1)


def describe(cs):
    return (f"{cs['name']} x{cs['batch']} beta={cs['beta']:g} epsilon={cs['epsilon']} native={cs['native']:.2f} held={cs['held']:.2f} "
            f"offset={cs['offset']:g}")


def problem(cs, perturb=None):
    """dict(YorgInt (d, n), M, Mmiss (batch, d, n) uint8, C0, X0, draws: per replica the record of draw_bpmf, nb: the warm start's
    num_batches); the sampler family has W0 (batch, n, r) and P0 (batch, d, r) besides, and C0, X0 are theirs (what the warm start
    would be handed; it does not run).  It does not depend on epsilon.  `perturb` = eps: YorgInt, C0, X0 (W0, P0) and the normals times
    (1 + eps u), u uniform in [-1, 1]."""
    d, n, r, B = cs["d"], cs["n"], cs["r"], cs["batch"]
    rng = np.random.default_rng([SEED, cs["no"], cs["salt"], 1])
    YorgInt, M, Mmiss = PN.masks(cs, rng, 2)
    draws = [BC.draw_seeded([SEED, cs["no"], cs["salt"], 10 + b], d, n, r, int(M[b].sum()), cs["epochs"]) for b in range(B)]
    pb = dict(YorgInt=YorgInt, M=M, Mmiss=Mmiss, draws=draws, nb=min(9, max(1, min(int(M[b].sum()) for b in range(B)) // 8)))
    moved = ["YorgInt", "C0", "X0"]
    if cs["family"] == "sampler":
        pb["W0"] = rng.standard_normal((B, n, r)) * 10.0 ** rng.uniform(-2.0, 1.0, (B, 1, r))
        pb["P0"] = rng.standard_normal((B, d, r)) * 10.0 ** rng.uniform(-2.0, 1.0, (B, 1, r))
        pb["C0"], pb["X0"] = pb["P0"], np.ascontiguousarray(np.transpose(pb["W0"], (0, 2, 1)))
        moved = ["YorgInt", "W0", "P0"]
    else:
        pb["C0"], pb["X0"] = rng.random((B, d, r)), rng.random((B, r, n))
    if perturb is not None:
        arrays = {k: pb[k] for k in moved}
        arrays.update({f"normals{b}": draws[b]["normals"] for b in range(B)})
        out = netlib.perturbed(arrays, [SEED, cs["no"], cs["salt"], 2], perturb)
        pb.update({k: out[k] for k in moved})
        pb["draws"] = [dict(draws[b], normals=out[f"normals{b}"]) for b in range(B)]
    return pb


def warm_start(cs, pb):
    """the warm_start keywords of bpmf_batch and of the model"""
    return dict(epsilon=cs["epsilon"], num_batches=pb["nb"])


def run_model(cs, pb, b, dtype=float, algebra="device", order="reference"):
    kw = dict(epochs=cs["epochs"], beta=cs["beta"], algebra=algebra, order=order, dtype=dtype)
    if cs["family"] == "sampler":
        kw["factors"] = (pb["W0"][b], pb["P0"][b])
    else:
        kw["warm_start"] = warm_start(cs, pb)
    with np.errstate(all="ignore"):
        return bpmf_model.bpmf_model(pb["YorgInt"], pb["M"][b], pb["Mmiss"][b], pb["C0"][b], pb["X0"][b], pb["draws"][b], **kw)


distance = PN.distance


def admissible(cs):
    """(admitted, text): the rule of the module docstring, replica by replica"""
    pb, pp = problem(cs), problem(cs, perturb=EPS)
    resp = dist = 0.0
    try:
        for b in range(cs["batch"]):
            ext = run_model(cs, pb, b, LD)
            netlib.require_finite(ext, KEYS, f"replica {b}")
            moved = run_model(cs, pp, b, LD)
            netlib.require_finite(moved, KEYS, f"replica {b}, inputs moved")
            resp = max(resp, distance(moved, ext))
            dist = max([dist] + [distance(run_model(cs, pb, b, float, a, o), ext) for a, o in FLOAT_VARIANTS[cs["family"]]])
    except (np.linalg.LinAlgError, FloatingPointError) as e:
        return False, f"{type(e).__name__}: {e}"
    ok = bool(resp <= BAR / 16 and dist <= BAR / 16)          # (a NaN in either fails)
    return ok, f"response to a last-bit change {resp:.2e}, float64 model within {dist:.2e} (both <= {BAR / 16:.2e})"


def resolve(i):
    """netlib.resolve on this net: ((salt, times shortened), log)"""
    return netlib.resolve(i, case, shorten, admissible, describe)


# What `resolve` answers where it is not (0, 0), {case: (salt, times shortened)}; tests/test_bpmf_net_cases_cpu.py recomputes every
# entry and every absence.
RESOLUTION = {5: (0, 1), 6: (0, 1), 8: (0, 1), 10: (0, 1), 11: (0, 1), 12: (0, 1), 13: (0, 1), 14: (0, 1), 15: (0, 1), 16: (0, 1), 17: (0, 1),
              18: (0, 1), 21: (0, 1), 22: (0, 1), 23: (0, 2), 24: (0, 1), 25: (0, 2), 26: (0, 1), 27: (0, 1), 29: (0, 1), 30: (0, 1), 31: (0, 2)}


def device_case(i):
    """case i as the net runs it"""
    return netlib.device_case(i, case, shorten, RESOLUTION.get(i, (0, 0)))


@lru_cache(maxsize=None)
def reference(no):
    """(case, problem, the extended model's answer per replica, the float64 model's in the same algebra) of case `no`, computed once
    and shared: do not modify any of it"""
    cs = device_case(no)
    pb = problem(cs)
    B = range(cs["batch"])
    return cs, pb, tuple(run_model(cs, pb, b, LD) for b in B), tuple(run_model(cs, pb, b, float) for b in B)


def device_env(cs):
    """the environment of the case's device call"""
    return {"PSMF_BPMF_COLS": str(cs["cols"])} if cs["cols"] else {}
