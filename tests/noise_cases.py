"""Seeded configurations of the UNMASKED handle with a non-scalar observation noise R, the problem each one runs and the float64
oracle carried across the same run parts.  Two families, both on the launched per-step engine (psmf_step.hip: psmf_sweep_solve +
psmf_serial / psmf_wave16 per timestep, the weighted Gram psmf_wgram_mfma -- PSMF_WGRAM_MFMA=0: psmf_gram_partial -- in front):

  row    cases 0 .. 35: R = rho diag(rho_rows) (nonuniform_R + psmf_set_row_noise), against oracle.lowrank_step with a vector rho;
  dense  cases 36 .. 59: a dense symmetric PSD R = U diag(lam) U^T (psmf_set_noise_rotation: the handle runs the row path in the
         eigenbasis and rotates at its boundary with psmf_rot_gemm), against oracle.literal_step with the d x d matrix, which
         forms the dense inverse the device never forms.

Pure Python: tests/test_noise_cases_cpu.py checks the coverage and the conditioning of every case without a GPU,
tests/test_hip_noise_net.py runs the same list on the device.

The axes of a case are fixed by its number alone (AXES below: every axis is its value list tiled over the family and permuted by
a fixed generator, so each value sits on floor(n / len) cases at least and the axes cross at random); the salt of the admission
redraws the horizon, the seed of the data and nothing else, so admission cannot drop an axis.  Two axes are constrained by others
and settled in `_axes`: the rank (r <= d; r <= 16 under a dense-Jacobian kind) and the filter (schedules are PSMF's).

  rows d      2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 193, 255, 256, 257, 700: the K slab (16) of psmf_rot_gemm, its 64-tile,
              the 256 workgroups of the Gram, each +-1, one multi-tile ragged size; dense cases stop at 257 (the oracle's inverse)
  rank r      1, 2, 8, 9, 16, 17, 32, 33, 48, 49, 64: every wgram_for instance edge, rpad 8 / 16 / 32 / 64, solve_lds
  storage     f32 / f64 crossed with the dtype of the uploaded series (a float32 upload is a float32-representable series)
  filter      PSMF; rPSMF, with a fixed lambda, with alpha / beta scaling
  spectrum    row: benign (0.3 + 2 U(0,1), the draw of the fixed tests), spread over 1e6, a few entries exactly 0, all equal
              but one; dense: well conditioned, low rank plus diagonal, singular PSD, block diagonal, a repeated eigenvalue
  mode        MODES: the five hook configurations, cos-phase, a dense-Jacobian kind, in-loop Adam / SGD with update_every > 1,
              rho_k / q_k schedules in front of R, a general Q, the simplified hooks with the in-loop Adam
  run shape   T <= 24, one to three parts with cuts at 1 and T - 1, an empty run, a second pass
  switches    PSMF_WGRAM_MFMA 0 / 1 on the row cases
  shards      SHARDED: six row cases (random walk, six different modes) also run as 2 and 3 row shards

Reference: pypsmf/psmf/psmf.py:85-180,287-304, rpsmf.py:116-184 (through oracle/psmf_oracle.py)."""

import numpy as np

import blocked_cases as BC
import netlib
import step_cases as SC
from blocked_cases import ADAM_LR, HOOKS, SGD_LR, gradsum_bar, mode_of, passes_of  # noqa: F401  (the device test takes them from here)
from oracle import psmf_oracle as O

N_ROW, N_DENSE = 36, 24
N_CASES = N_ROW + N_DENSE
D_LIST = (2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 193, 255, 256, 257, 700)
DENSE_D_MAX = 257
R_LIST = (1, 2, 8, 9, 16, 17, 32, 33, 48, 49, 64)
DENSE_KIND_R_MAX = 16
T_MAX = 24
FILTERS = {
    "psmf": dict(robust=False, fixed_lambda=False, alpha=1.0, beta=1.0),
    "rpsmf": dict(robust=True, fixed_lambda=False, alpha=1.0, beta=1.0),
    "rpsmf_fixed_lambda": dict(robust=True, fixed_lambda=True, alpha=1.0, beta=1.0),
    "rpsmf_scaled": dict(robust=True, fixed_lambda=False, alpha=0.95, beta=1.05),
}
IO = (("f64", "f64"), ("f64", "f32"), ("f32", "f64"), ("f32", "f32"))          # (storage, dtype of the uploaded series)
ROW_SPECTRA = ("benign", "spread_1e6", "zeros", "one_off")
DENSE_SPECTRA = ("well", "lowrank_diag", "singular", "block", "repeated")
SHAPES = ("one", "cut_1", "cut_last", "cut_both")

# hooks, dynamics, in-loop optimiser (1 Adam, 2 SGD) and its period, schedules, general Q
MODES = [
    dict(hooks="full", dyn="random_walk"),
    dict(hooks="simplified", dyn="random_walk"),          # no weighted Gram (enqueue_step), the robust quad still takes per-row kappa
    dict(hooks="no_update", dyn="random_walk"),
    dict(hooks="eta_R", dyn="random_walk"),
    dict(hooks="pbar_P", dyn="random_walk"),
    dict(hooks="full", dyn="cos_phase"),
    dict(hooks="full", dyn="cos_phase", recursive=1, update_every=3),
    dict(hooks="full", dyn="cos_phase", recursive=2, update_every=2),
    dict(hooks="full", dyn="random_walk", sched=True),
    dict(hooks="full", dyn="random_walk", general_Q=True),
    dict(hooks="simplified", dyn="cos_phase", recursive=1, update_every=3),
    dict(hooks="full", dyn="scaled_walk"),                # a dense Jacobian: r <= 16
]


def _spread(n_values, n, key):
    """indices 0 .. n_values - 1 tiled over n cases and permuted by a fixed generator"""
    return [int(k) for k in np.random.default_rng([9400] + key).permutation(np.resize(np.arange(n_values), n))]


def _axes(family, n, ds, spectra, fkey):
    ax = dict(d=_spread(len(ds), n, [fkey, 0]), mode=_spread(len(MODES), n, [fkey, 1]), filt=_spread(len(FILTERS), n, [fkey, 2]),
              io=_spread(len(IO), n, [fkey, 3]), spec=_spread(len(spectra), n, [fkey, 4]), shape=_spread(len(SHAPES), n, [fkey, 5]),
              r=_spread(len(R_LIST), n, [fkey, 6]), wgram=_spread(2, n, [fkey, 7]), second=_spread(3, n, [fkey, 8]), empty=_spread(6, n, [fkey, 9]))
    # the rank is constrained by the rows and the kind (r <= d; r <= 16 under a dense-Jacobian kind): the tightest cases choose
    # first, each the admitted rank with the fewest cases so far (ties: by the case's own permuted preference)
    r_max = [min(ds[ax["d"][j]], DENSE_KIND_R_MAX if MODES[ax["mode"][j]]["dyn"] in BC.DENSE_KINDS else max(R_LIST)) for j in range(n)]
    count, rank = {r: 0 for r in R_LIST}, {}
    for j in sorted(range(n), key=lambda j: (r_max[j], ax["r"][j], j)):
        rank[j] = min((r for r in R_LIST if r <= r_max[j]), key=lambda r: (count[r], (R_LIST.index(r) - ax["r"][j]) % len(R_LIST)))
        count[rank[j]] += 1
    out = []
    for j in range(n):
        d, mode, r = ds[ax["d"][j]], MODES[ax["mode"][j]], rank[j]
        filt = "psmf" if mode.get("sched") else list(FILTERS)[ax["filt"][j]]          # R_k / Q_k schedules: PSMF only
        spec = spectra[ax["spec"][j]]
        if spec == "repeated" and d < 3:          # (at d = 2 a repeated eigenvalue is R = c I)
            spec = "well"
        out.append(dict(family=family, d=d, r=r, mode=ax["mode"][j], filter=filt, storage=IO[ax["io"][j]][0], upload=IO[ax["io"][j]][1],
                        spectrum=spec, shape=SHAPES[ax["shape"][j]], second_pass=ax["second"][j] == 0, empty=ax["empty"][j] == 0,
                        env={"PSMF_WGRAM_MFMA": "0"} if family == "row" and ax["wgram"][j] == 0 else {}))
    return out


AXES = _axes("row", N_ROW, D_LIST, ROW_SPECTRA, 1) + _axes("dense", N_DENSE, tuple(d for d in D_LIST if d <= DENSE_D_MAX), DENSE_SPECTRA, 2)


def _sharded():
    """six row cases with fifteen rows at least and the random walk, of six different modes, float64 and float32 storage in turn"""
    out = []
    for m in [m for m, mode in enumerate(MODES) if mode["dyn"] == "random_walk"][:6]:
        cand = [i for i, a in enumerate(AXES[:N_ROW]) if a["d"] >= 15 and a["mode"] == m]
        want = ("f64", "f32")[len(out) % 2]
        out.append(next((i for i in cand if AXES[i]["storage"] == want), cand[0]))
    return tuple(sorted(out))


SHARDED = _sharded()
SHARDS = (2, 3)


# ---- the draw
def _parts(T, shape, empty):
    cuts = sorted({c for c in {"one": (), "cut_1": (1,), "cut_last": (T - 1,), "cut_both": (1, T - 1)}[shape] if 1 <= c <= T - 1})
    pts = [0] + cuts + [T]
    parts = list(zip(pts[:-1], pts[1:]))
    if empty:          # an empty run behind the first part
        parts.insert(1, (parts[0][1], parts[0][1]))
    return parts


def case(i, salt=0):
    """Configuration number i; `salt` > 0 gives the replacements the conditioning check may ask for (horizon and data alone)."""
    a = AXES[i]
    mode = MODES[a["mode"]]
    rng = np.random.default_rng([9300 + i, salt])
    cs = dict(a, i=i, salt=salt, shortened=0, masked=False, nonuniform=True, **FILTERS[a["filter"]])
    cs.update(hooks=mode["hooks"], dyn=mode["dyn"], recursive=mode.get("recursive", 0), update_every=mode.get("update_every", 1),
              sched=bool(mode.get("sched")), general_Q=bool(mode.get("general_Q")), v0=0.02 if a["storage"] == "f32" else 0.1)
    # a trigonometric f on float32 inputs: the oracle's own answer moves by more than 1e-5 / 16 within ten steps or so (step_cases)
    cs["T"] = int(rng.integers(3, 9)) if cs["dyn"] == "cos_phase" and cs["storage"] == "f32" else int(rng.integers(8, T_MAX + 1))
    cs["seed"] = int(rng.integers(1 << 30))
    cs["parts"] = _parts(cs["T"], cs["shape"], cs["empty"])
    cs["shards"] = SHARDS if i in SHARDED else ()
    return cs


def shorten(cs):
    """The same case over half the horizon (not below 2 steps); None when it cannot be halved."""
    T = max(cs["T"] // 2, 2)
    if T >= cs["T"] or cs["shortened"] >= 2:
        return None
    return dict(cs, T=T, shortened=cs["shortened"] + 1, parts=_parts(T, cs["shape"], cs["empty"]))


# ---- tolerances: the bars the suite states
def bar(cs):
    """row: step_cases.bar (1e-9, float32 storage 1e-5); dense: what tests/test_hip_dense_R.py states (1e-8, 1e-5)"""
    if cs["family"] == "row":
        return SC.bar(cs)
    return 1e-5 if cs["storage"] == "f32" else 1e-8


# ---- the problem of a case
def row_noise(cs):
    d = cs["d"]
    rng = np.random.default_rng(cs["seed"] ^ 0xD1A6)
    rho = 0.3 + 2.0 * rng.random(d)
    if cs["spectrum"] == "spread_1e6":
        rho = 10.0 ** (6.0 * rng.random(d) - 3.0)
        rho[0], rho[-1] = 1e-3, 1e3
    elif cs["spectrum"] == "zeros":          # (never all of them: tr(R) > 0)
        rho[sorted({0, d // 2, d - 1})[:max(1, min(3, d - 1))]] = 0.0
    elif cs["spectrum"] == "one_off":
        rho[:] = 0.8
        rho[d // 3] = 4.0
    return rho


def _orthogonal(rng, n):
    return np.linalg.qr(rng.standard_normal((n, n)))[0]


def dense_noise(cs):
    """the d x d symmetric PSD R of a dense case (entries off the diagonal whatever the spectrum)"""
    d = cs["d"]
    rng = np.random.default_rng(cs["seed"] ^ 0xDE5E)
    kind = cs["spectrum"]
    if kind == "well":
        A = rng.standard_normal((d, d))
        R = A @ A.T / d + 0.1 * np.eye(d)
    elif kind == "lowrank_diag":
        k = min(12, d)
        B = rng.standard_normal((d, k)) / np.sqrt(k)
        R = np.diag(0.2 + rng.random(d)) + 0.7 * (B @ B.T)
    elif kind == "singular":          # rank d // 2 (d = 2, 3: rank 1): the other eigenvalues are 0 to rounding, clipped by structure_of
        k = max(1, d // 2)
        B = rng.standard_normal((d, k))
        R = B @ B.T / k
    elif kind == "block":             # three blocks (d < 6: one 2 x 2 block and what is left on the diagonal)
        sizes = [d // 3, d // 3, d - 2 * (d // 3)] if d >= 6 else [2] + [1] * (d - 2)
        R, o = np.zeros((d, d)), 0
        for n in sizes:
            A = rng.standard_normal((n, n))
            R[o:o + n, o:o + n] = A @ A.T / n + 0.2 * np.eye(n)
            o += n
    else:                             # "repeated": half of the spectrum is one eigenvalue -- its eigenvectors are any basis of the subspace
        lam = 0.3 + 2.0 * rng.random(d)
        lam[:max(2, d // 2)] = 0.5
        U = _orthogonal(rng, d)
        R = (U * lam) @ U.T
    return 0.5 * (R + R.T)


def problem(cs, perturb=None):
    """blocked_cases.problem (Y, C0, V0, P0, Q, mu0, theta, schedules) and the noise: rho_rows (d,) of a row case, R0 (d, d) of a
    dense one.  A float32 upload is a series of float32 values, whatever the storage.  R is never perturbed."""
    pb = BC.problem(cs, perturb)
    if cs["upload"] == "f32":
        pb["Y"] = netlib.f32_round(pb["Y"])
    if cs["family"] == "row":
        pb["rho_rows"] = row_noise(cs)
    else:
        pb["R0"] = dense_noise(cs)
    return pb


def _front(rho, R):
    """the scalar in front of R that the device keeps: rho = c R"""
    if np.ndim(R) == 2:
        return float(rho[0, 0] / R[0, 0])
    j = int(np.argmax(R))
    return float(rho[j] / R[j])


def run_oracle(cs, pb, Y, C0, R, step):
    """`step` (lowrank_step with R a (d,) vector, literal_step with R a vector or a d x d matrix) over the passes and parts of the
    case, as blocked_cases.reference carries them: one record per part -- the state after it (rho: the scalar in front of R),
    y_pred of the part."""
    mode, dyn = mode_of(cs), BC.dynamics_of(pb)
    n_theta = dyn.n_theta
    st = O.State(C=C0.copy(), V=pb["V0"].copy(), mu=pb["mu0"].copy(), P=pb["P0"].copy(), Q=pb["Q"].copy(), rho=R.copy(), lam=pb["lam"],
                 theta=pb["theta"].copy(), gradsum=np.zeros(n_theta))
    out = []
    for ep in range(passes_of(cs)):
        if ep and cs["robust"]:             # rPSMF's step_reset: Q, R, lambda start again (rpsmf.py:106-114)
            st.Q, st.rho, st.lam = pb["Q"].copy(), R.copy(), pb["lam"]
        st.gradsum = np.zeros(n_theta)
        m = v = np.zeros(n_theta)
        for a, b in cs["parts"]:
            Yp = np.empty((b - a, cs["d"]))
            for k in range(a + 1, b + 1):
                Qk = None if pb["q_k"] is None else pb["q_k"][k] * pb["Q"]
                rk = None if pb["rho_k"] is None else pb["rho_k"][k] * R
                st, info = step(st, Y[k - 1], k, mode, dyn, Qk=Qk, rhok=rk, want_grad=n_theta > 0)
                Yp[k - a - 1] = info.y_pred
                if cs["recursive"] and k % cs["update_every"] == 0:          # psmf.py:299-304
                    if cs["recursive"] == 1:
                        st.theta, m, v = O.adam_update(st.theta, st.gradsum, m, v, k, lr=ADAM_LR)
                    else:
                        st.theta = O.sgd_update(st.theta, st.gradsum, lr=SGD_LR)
                    st.gradsum = np.zeros(n_theta)
            out.append(dict(ep=ep, a=a, b=b, C=st.C.copy(), V=st.V.copy(), mu=st.mu.copy(), P=st.P.copy(), Q=np.array(st.Q, dtype=float),
                            rho=_front(st.rho, R), lam=float(st.lam), theta=st.theta.copy(), gradsum=st.gradsum.copy(), y_pred=Yp))
    return out


def reference(cs, pb):
    """row: lowrank_step with the vector rho_rows; dense: literal_step with the d x d matrix (the dense inverse of psmf.py:150-152)"""
    if cs["family"] == "row":
        return run_oracle(cs, pb, pb["Y"], pb["C0"], pb["rho_rows"], O.lowrank_step)
    return run_oracle(cs, pb, pb["Y"], pb["C0"], pb["R0"], O.literal_step)


def eigen(pb, d):
    """(lam, U) of a dense case as the product decomposes R (rpsmf_amd._noise.structure_of: numpy only)"""
    from rpsmf_amd import _noise

    dense, _ = _noise.structure_of(pb["R0"], d)
    assert dense is not None, "a dense case has entries off the diagonal"
    return dense


def reference_rotated(cs, pb):
    """A dense case the way the device runs it, on the CPU: lowrank_step on (Y U, U^T C0, lam), C and y_pred rotated back.  The
    second model of a dense case: no d x d inverse, another eigenbasis wherever an eigenvalue repeats."""
    lam, U = eigen(pb, cs["d"])
    out = run_oracle(cs, pb, pb["Y"] @ U, U.T @ pb["C0"], lam, O.lowrank_step)
    for rec in out:
        rec["C"], rec["y_pred"] = U @ rec["C"], rec["y_pred"] @ U.T
    return out


STATE_KEYS = ("C", "V", "mu", "P", "y_pred")


def compared(cs):
    return STATE_KEYS + (("rho", "lam", "Q") if cs["robust"] else ())


def sensitivity(cs):
    """relerr between the oracle on the case's inputs and on inputs moved by a relative 2^-50 (float32 storage: 2^-23, after the
    rounding): (the worst over C, V, mu, P, y_pred -- rPSMF: and rho, lam, Q, which the device test compares too and which a
    singular R under the simplified hooks lets run away while C stands still -- of every part, the worst gradsum).  A dense case
    answers for its reference too: the worse of that response and of the distance between its two models, literal_step on R and
    lowrank_step in the eigenbasis (the dense inverse of a singular R + s I loses digits of its own)."""
    eps = 2.0 ** -23 if cs["storage"] == "f32" else 2.0 ** -50
    pb = problem(cs)
    ref0 = reference(cs, pb)
    ref1 = reference(cs, problem(cs, perturb=(cs["seed"] ^ 0x5EED, eps)))
    for part in ref0:
        netlib.require_finite(part, compared(cs) + ("gradsum",), f"case {cs['i']}")
    state, grad = netlib.response(ref0, ref1, compared(cs)), BC.grad_response(ref0, ref1)
    if cs["family"] == "dense":
        ref2 = reference_rotated(cs, pb)
        state, grad = max(state, netlib.response(ref0, ref2, compared(cs))), max(grad, BC.grad_response(ref0, ref2))
    return state, grad


def admissible(cs):
    try:
        state, grad = sensitivity(cs)
    except (np.linalg.LinAlgError, FloatingPointError) as e:
        return False, f"{type(e).__name__}: {e}"
    return state <= bar(cs) / 16 and grad <= gradsum_bar(cs) / 16, f"sensitivity {state:.2e} (bar {bar(cs):.0e}), gradsum {grad:.2e}"


def describe(cs):
    return f"{cs['family']} {cs['spectrum']} T={cs['T']} d={cs['d']} r={cs['r']} {cs['storage']} {cs['dyn']} {cs['hooks']}"


# What `resolve` answers for the cases it does not leave alone, {i: (salt, times shortened)}: recorded here so that the device
# test need not run the oracle three times per case; tests/test_noise_cases_cpu.py recomputes every entry (and every absence).
RESOLUTION = {10: (0, 2), 12: (0, 1), 26: (0, 1), 27: (0, 1), 33: (0, 1), 38: (0, 1), 48: (0, 1), 49: (0, 1), 54: (0, 2), 56: (0, 1), 57: (0, 1)}


def resolve(i):
    """netlib.resolve on this net (halving not below 2 steps): ((salt, times shortened), log)"""
    return netlib.resolve(i, case, shorten, admissible, describe)


def device_case(i):
    return netlib.device_case(i, case, shorten, RESOLUTION.get(i, (0, 0)))
