"""Seeded random configurations of the time-blocked engine (engine = 2 of include/psmf_hip.h), the problem each one runs and the
float64 oracle carried across the same run parts.  Pure Python: tests/test_blocked_cases_cpu.py checks the list's coverage and
the conditioning of every case without a GPU, tests/test_hip_block_engine_random.py runs the same list on the device.

`case(i)` draws over the axes the blocked engine dispatches on -- rank, rows (half of them from a list of tiny / tile-edge
values), horizon and cut points around the block length B = min(64 - r, 48), dynamics kind, hook configuration, PSMF / rPSMF,
Q = q I or a general Q, R_k / Q_k schedules, the in-loop optimiser, storage type, the environment switches that reach the
kernels the defaults cannot, row shards.  The draw is stratified: case i is aimed at the pair (filter kernel, dynamics kind)
number i mod len(TARGETS), and the other axes are redrawn until `expected_kernel` names that kernel, so that every kernel sees
every kind it can take however small N_CASES is.

`expected_kernel` / `expected_bulk` restate the dispatch as tables in the words of psmf_filter_kernel's description
(include/psmf_hip.h); the device test asserts that the handle reports the same name.
Reference: pypsmf/psmf/psmf.py:85-180,287-304, rpsmf.py:116-184, nonlinearities.py:42-150."""

import numpy as np

import netlib
from netlib import relerr  # noqa: F401  (the device tests and tools take it from here)
from oracle import psmf_oracle as O

N_CASES = 171            # 3 x len(TARGETS)
R_LIST = (1, 2, 3, 7, 8, 9, 15, 16, 17, 20, 24, 31, 32)
R_WEIGHTS = np.array([1.0] * 12 + [3.0]) / 15.0        # r = 32: the headline rank, and the only one with two-tile series blocks
ADAM_LR, SGD_LR = 1e-3, 1e-7        # (SGD steps by lr x the raw gradient sum, which grows with d)


def block_steps(r):
    return min(64 - r, 48)


def tiny_rows(r):
    return sorted({d for d in (1, 2, 3, r - 1, r, r + 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 513) if d >= 1})


def horizon_edges(B):
    return sorted({1, 2, B - 1, B, B + 1, 2 * B, 2 * B + 1, 3 * B - 1})


def cut_edges(B, T):
    """the cut points a case is biased towards (those that lie strictly inside the run)"""
    return sorted({c for c in (1, B - 1, B, B + 1, T - 1) if 1 <= c <= T - 1})


# ---- dynamics kinds: name -> (constructor of the rpsmf_amd.nonlinearities object, diagonal Jacobian?)
def _nl(name, r):
    from rpsmf_amd import nonlinearities as NL

    return {
        "random_walk": lambda: NL.RandomWalk(),
        "cos_phase": lambda: NL.CosPhase(r),
        "scaled_walk": lambda: NL.ScaledWalk(r, bias=False),
        "scaled_walk_bias": lambda: NL.ScaledWalk(r, bias=True),
        "sinusoid": lambda: NL.Sinusoid(r),
        "sinusoid_unphased": lambda: NL.Sinusoid(r, phased=False),
        "sinusoid_unscaled": lambda: NL.Sinusoid(r, scaled=False),
        "sinusoid_plain": lambda: NL.Sinusoid(r, scaled=False, phased=False),
        "fourier1": lambda: NL.FourierBasis(r, N=1),
        "fourier2": lambda: NL.FourierBasis(r, N=2),
        "fourier3": lambda: NL.FourierBasis(r, N=3),
    }[name]()


DIAGONAL_KINDS = ("random_walk", "cos_phase", "sinusoid_unscaled", "sinusoid_plain")      # df/dx is diagonal
DENSE_KINDS = ("scaled_walk", "scaled_walk_bias", "sinusoid", "sinusoid_unphased", "fourier1", "fourier2", "fourier3")
KINDS = DIAGONAL_KINDS + DENSE_KINDS
LINEAR_KINDS = ("scaled_walk", "scaled_walk_bias")        # f is affine in x: no trigonometric term

HOOKS = {        # coef_update, eta_full, pbar_predict  (psmf_config)
    "full": (True, True, True),
    "simplified": (False, False, False),        # synthetic_psmf.py:78-100: the filter5 configuration
    "no_update": (False, True, True),
    "eta_R": (True, False, True),
    "pbar_P": (True, True, False),
}

KERNELS = ("psmf_blk_filter", "psmf_blk_filter2", "psmf_blk_filter3", "psmf_blk_filter3s", "psmf_blk_filter4", "psmf_blk_filter4s",
           "psmf_blk_filter5", "psmf_blk_filter6", "psmf_blk_filter6d", "psmf_blk_filter7")


def _on(cs, name):
    return cs["env"].get(name) != "0"


def facts(cs):
    """What the dispatch looks at, by name."""
    cu, ef, pp = HOOKS[cs["hooks"]]
    f = dict(
        simplified_hooks=not (cu or ef or pp),
        full_filter=cu and ef and pp,
        diagonal_jacobian=cs["dyn"] in DIAGONAL_KINDS,
        random_walk=cs["dyn"] == "random_walk",
        q_iso=(not cs["general_Q"]) or cs["r"] == 1,        # at r = 1 every Q is q I
        schedules=cs["sched"],
        sgd_in_loop=cs["recursive"] == 2,
        small_rank=cs["r"] <= 16,
        sw_filter3=_on(cs, "PSMF_FILTER3"), sw_filter6=_on(cs, "PSMF_FILTER6"), sw_filter6_dual=_on(cs, "PSMF_FILTER6_DUAL"),
        sw_filter7=_on(cs, "PSMF_FILTER7"),
    )
    # "the default model": random walk, Q = q I, the full filter, rho and q constant over a block
    f["default_model"] = f["random_walk"] and f["q_iso"] and f["full_filter"] and not f["schedules"]
    f["filter6_rank"] = f["small_rank"] and f["sw_filter6"]
    return f


# First row whose conditions all hold names the kernel (psmf_filter_kernel, include/psmf_hip.h: codes 1 .. 10).  A condition is
# (fact, wanted value); `rank` picks between the two names of a row: (r > 16, r <= 16).
KERNEL_TABLE = [
    # the simplified hook configuration with a diagonal Jacobian (filter4's machinery: both switches on; Adam of its own, no SGD)
    (("psmf_blk_filter5", "psmf_blk_filter5"), [("simplified_hooks", True), ("diagonal_jacobian", True), ("schedules", False),
                                                 ("sgd_in_loop", False), ("sw_filter3", True)]),
    # the default model at r <= 16: filter6 with the two inversions side by side
    ((None, "psmf_blk_filter6d"), [("default_model", True), ("filter6_rank", True), ("sw_filter6_dual", True)]),
    # the default model elsewhere: the role-specialised two-inversion kernel, PSMF_FILTER3=0: the two-halves kernel
    (("psmf_blk_filter3", "psmf_blk_filter3s"), [("default_model", True), ("sw_filter3", True)]),
    (("psmf_blk_filter2", "psmf_blk_filter2"), [("default_model", True)]),
    # diagonal-Jacobian dynamics (and the random walk that schedules keep off filter3), full filter, Q = q I, where filter6 does not
    # take the rank
    (("psmf_blk_filter4", "psmf_blk_filter4s"), [("filter6_rank", False), ("full_filter", True), ("q_iso", True), ("diagonal_jacobian", True),
                                                  ("sgd_in_loop", False), ("sw_filter3", True)]),
    # every other configuration at r <= 16
    ((None, "psmf_blk_filter6"), [("filter6_rank", True)]),
    # what is left at 17 <= r <= 32
    (("psmf_blk_filter7", None), [("small_rank", False), ("sw_filter7", True)]),
    # the general blocked kernel
    (("psmf_blk_filter", "psmf_blk_filter"), []),
]


def expected_kernel(cs):
    f = facts(cs)
    for names, conds in KERNEL_TABLE:
        name = names[1 if f["small_rank"] else 0]
        if name is not None and all(f[k] == v for k, v in conds):
            return name
    raise AssertionError(cs)


def expected_bulk(cs, d_local=None):
    """(family, instantiation) of the d-sized kernels of a handle with d_local rows: the streaming psmf_blk_xgram2<n> /
    psmf_blk_apply2<n> for float32 storage with a row count that is a multiple of 4 (16-byte loads of four rows; the padded row
    length of float32 storage always is), n = 2 or 3 sixteen-column tiles of a series block; the MFMA psmf_blk_gram_mfma /
    psmf_blk_xgram_mfma / psmf_blk_apply_mfma family otherwise (no instantiation)."""
    dl = cs["d"] if d_local is None else d_local
    if _on(cs, "PSMF_BULK2") and cs["storage"] == "f32" and dl % 4 == 0:
        return "streaming", (2 if -(-block_steps(cs["r"]) // 16) <= 2 else 3)
    return "mfma", None


def kinds_of(kernel):
    """the dynamics kinds a kernel can take"""
    if kernel in ("psmf_blk_filter2", "psmf_blk_filter3", "psmf_blk_filter3s", "psmf_blk_filter6d"):
        return ("random_walk",)
    if kernel in ("psmf_blk_filter4", "psmf_blk_filter4s", "psmf_blk_filter5"):
        return DIAGONAL_KINDS
    return KINDS


# every (kernel, kind it can take) once; the four kernels of the default model (one kind each) three times
TARGETS = [(k, kind) for k in KERNELS for kind in kinds_of(k) for _ in range(3 if len(kinds_of(k)) == 1 else 1)]


# ---- the draw
def _draw(rng, kind):
    r = int(rng.choice(R_LIST, p=R_WEIGHTS))
    B = block_steps(r)
    has_theta = kind != "random_walk"
    n_theta = n_theta_of(kind, r)
    if n_theta > MAX_THETA:          # (FourierBasis at r = 32, N = 3 has 6528 parameters: N = 3 stays at r <= 17, N = 2 at r <= 20)
        return None
    robust = bool(rng.random() < 0.5)
    # (float32 storage leaves a trigonometric f little room: the oracle's own response to a last-bit change of the float32 inputs
    #  has to sit 16 x inside 1e-5, so most of the float32 cases are random walks)
    cs = dict(r=r, B=B, dyn=kind, robust=robust, storage="f32" if rng.random() < (0.3 if has_theta else (0.8 if r == 32 else 0.5)) else "f64")
    # V0 = v I: the gain of the dictionary update.  Every entry of a float32 series carries its own last-bit error and C sums
    # their effect over the steps, so float32 cases take the stiffer prior (their bar is 1e-5 whatever the horizon)
    cs["v0"] = 0.02 if cs["storage"] == "f32" else 0.1
    cs["fixed_lambda"] = bool(robust and rng.random() < 0.25)
    scaled = robust and rng.random() < 0.3
    cs["alpha"] = float(rng.choice([0.95, 1.05])) if scaled else 1.0
    cs["beta"] = float(rng.choice([0.95, 1.05])) if scaled else 1.0
    cs["general_Q"] = bool(rng.random() < 0.3)
    cs["sched"] = bool(not robust and rng.random() < 0.25)
    cs["hooks"] = str(rng.choice(list(HOOKS), p=[0.52, 0.18, 0.1, 0.1, 0.1]))
    u = rng.random()
    cs["recursive"] = (0 if u < 0.6 else (1 if u < 0.85 else 2)) if has_theta else 0
    cs["update_every"] = int(rng.choice([1, 2, 3, 5, 7])) if cs["recursive"] else 1
    env = {}
    if rng.random() < 0.25:          # a switch set that reaches a kernel the defaults cannot reach ...
        reach = ["PSMF_FILTER6_DUAL", "PSMF_FILTER6", "PSMF_FILTER3", "PSMF_FILTER7"]
        for name in rng.choice(reach, size=int(rng.integers(1, 3)), replace=False):
            env[str(name)] = "0"
        for name in ("PSMF_BULK2", "PSMF_BLOCK_CHAIN", "PSMF_BLOCK_PIPE", "PSMF_CHAIN_CARRY"):      # ... and the schedule switches
            if rng.random() < 0.25:
                env[name] = "0"
    cs["env"] = env
    # rows
    if r == 32 and cs["storage"] == "f32" and rng.random() < 0.6:
        cs["d"] = 4 * int(rng.integers(5, 1501))      # the headline path: two-tile series blocks through the streaming kernels
    elif rng.random() < 0.5:
        cs["d"] = int(rng.choice(tiny_rows(r)))
    else:
        cs["d"] = int(rng.integers(20, 6001))
        if cs["storage"] == "f32":      # the streaming d-sized kernels take multiples of 4 only: half of these, the other residues alike
            cs["d"] += int(rng.choice([0, 0, 0, 1, 2, 3])) - cs["d"] % 4
    # horizon: the filters with a coefficient update and a trigonometric f amplify a last-bit difference by orders of magnitude
    # per block, so those cases stay within a block or two
    short = has_theta and HOOKS[cs["hooks"]][0]
    edges = horizon_edges(B)
    if short:
        edges = [t for t in edges if t <= B + 1]
    if has_theta and cs["storage"] == "f32":
        # a trigonometric f on float32 inputs: the oracle's answer moves by more than 1e-5 / 16 within ten steps or so when the
        # inputs move by one float32 bit -- these cases check one short block on the float32 row stride, not a horizon
        # (the affine kinds below excepted)
        T = int(rng.choice([1, 2])) if rng.random() < 0.3 else int(rng.integers(2, 9))
        if kind in LINEAR_KINDS and T > 2:
            # the affine kinds carry a float32 bit further: these cases cross one block edge (T = B + 1, which `shorten` cannot
            # halve: one that is not admissible there is redrawn)
            T = B + 1
    elif rng.random() < 0.5:
        T = int(rng.choice(edges))
    else:
        T = int(rng.integers(2, (B + 8 if short else 200) + 1))
    if n_theta * T > MAX_THETA_STEPS:
        T = max(B + 1, MAX_THETA_STEPS // n_theta)
    cs["T"] = T
    cs["second_pass"] = bool(rng.random() < 1 / 3)
    cs["shards"] = None
    if rng.random() < 1 / 6 and cs["d"] >= 8:
        n = int(rng.integers(2, 4))
        small = int(rng.integers(1, 4))              # one shard of 1 .. 3 rows, the others uneven
        rest = cs["d"] - small
        cutsr = sorted(int(x) for x in rng.choice(np.arange(1, rest), size=n - 2, replace=False)) if n > 2 else []
        rows = [b - a for a, b in zip([0] + cutsr, cutsr + [rest])]
        rows.insert(int(rng.integers(0, n)), small)
        cs["shards"] = rows
    cs["seed"] = int(rng.integers(1 << 30))
    return cs


def _parts(rng, B, T):
    """one or two cut points (none fits into T = 1), biased to the block edges; one case in ten with an empty run between parts"""
    cuts = set()
    if T >= 2:
        want = min(int(rng.integers(1, 3)), T - 1)
        while len(cuts) < want:
            e = cut_edges(B, T)
            cuts.add(int(rng.choice(e)) if rng.random() < 0.7 else int(rng.integers(1, T)))
    pts = [0] + sorted(cuts) + [T]
    parts = list(zip(pts[:-1], pts[1:]))
    if rng.random() < 0.1:
        a = int(rng.choice(pts))
        k = next((i + 1 for i, p in enumerate(parts) if p[1] == a), 0)
        parts.insert(k, (a, a))
    return parts


def n_theta_of(kind, r):
    return _nl(kind, r).n_params


MAX_THETA, MAX_THETA_STEPS = 2000, 120000      # the oracle differentiates the callable by complex step: one call per parameter and step


def case(i, salt=0):
    """Configuration number i; `salt` > 0 gives the replacements the conditioning check may ask for."""
    target_kernel, kind = TARGETS[i % len(TARGETS)]
    rng = np.random.default_rng([7100 + i, salt])
    for _ in range(20000):
        cs = _draw(rng, kind)
        if cs is not None and expected_kernel(cs) == target_kernel:
            break
    else:
        raise AssertionError(f"no draw reaches {target_kernel} with {kind}")
    cs["parts"] = _parts(rng, cs["B"], cs["T"])
    cs["i"], cs["salt"], cs["shortened"] = i, salt, 0
    return cs


def shorten(cs):
    """The same case over half the horizon (not below B + 1), its cut points redrawn; None when it cannot be halved."""
    T = max(cs["T"] // 2, cs["B"] + 1)
    if T >= cs["T"] or cs["shortened"] >= 2:
        return None
    out = dict(cs, T=T, shortened=cs["shortened"] + 1)
    out["parts"] = _parts(np.random.default_rng([7100 + cs["i"], cs["salt"], out["shortened"]]), cs["B"], T)
    return out


# ---- tolerances: the bars the suite states for these quantities
def bar(cs):
    if cs["storage"] == "f32":
        return 1e-5
    if cs["dyn"] == "random_walk":
        return 1e-9
    return 1e-7 if cs["robust"] and expected_kernel(cs) == "psmf_blk_filter6" else 1e-8


def gradsum_bar(cs):
    return 1e-5 if cs["storage"] == "f32" else 1e-7


# ---- the problem of a case
def theta_for(nl, rng, r):
    """A theta in the regime the experiments use (beijing_psmf.py:117: 0.1 * rand): matrices near a contraction."""
    th = 0.1 * rng.random(nl.n_params)
    if type(nl).__name__ == "ScaledWalk" or getattr(nl, "scaled", False):
        th[:r * r] = (0.8 * np.eye(r) + 0.05 * rng.standard_normal((r, r))).reshape(-1)
    if type(nl).__name__ == "FourierBasis":
        for t in range(2 * nl.N):
            th[t * r * r:(t + 1) * r * r] = (0.5 * np.eye(r) + 0.05 * rng.standard_normal((r, r))).reshape(-1) / nl.N
    return th


def problem(cs, perturb=None):
    """Inputs of a case: Y (T, d), C0, V0, P0, Q, mu0, theta, schedules.
    `perturb` = (seed, eps): C0, Y and theta times (1 + eps u), u uniform in [-1, 1] -- after the rounding to float32 where the
    device stores float32 (the perturbed values are then rounded again, so both runs start from representable inputs)."""
    r, d, T = cs["r"], cs["d"], cs["T"]
    rng = np.random.default_rng(cs["seed"])
    nl = _nl(cs["dyn"], r)
    Ct = rng.standard_normal((d, r))
    x = rng.standard_normal(r)
    Y = np.empty((T, d))
    for t in range(T):
        x = 0.9 * np.sin(x + 0.3) + 0.1 * rng.standard_normal(r)
        Y[t] = Ct @ x + 0.3 * (rng.standard_t(3.0, d) if cs["robust"] else rng.standard_normal(d))
    C0 = 0.1 * rng.standard_normal((d, r))
    A = rng.standard_normal((r, r)) / np.sqrt(r)
    Q = 0.1 * np.eye(r) + (0.05 * (A @ A.T) if cs["general_Q"] else 0.0)
    mu0 = 0.2 * rng.standard_normal(r)
    theta = theta_for(nl, rng, r) if nl.n_params else np.zeros(0)
    rho_k = q_k = None
    if cs["sched"]:
        rho_k, q_k = 0.5 + rng.random(T + 1), 0.5 + rng.random(T + 1)
        q_k[1] = 1.0
    f32 = ("Y", "C0") if cs["storage"] == "f32" else ()
    if f32:
        Y, C0 = netlib.f32_round(Y), netlib.f32_round(C0)
    if perturb is not None:
        Y, C0, theta = netlib.perturbed(dict(Y=Y, C0=C0, theta=theta), *perturb, f32=f32).values()
    return dict(nl=nl, Y=Y, C0=C0, V0=cs["v0"] * np.eye(r), P0=np.eye(r), Q=Q, mu0=mu0, theta=theta, rho_k=rho_k, q_k=q_k,
                rho=1.0, lam=1.8)


def mode_of(cs):
    cu, ef, pp = HOOKS[cs["hooks"]]
    return O.Mode(robust=cs["robust"], coef_update=cu, eta_full=ef, pbar_predict=pp, alpha=cs["alpha"], beta=cs["beta"],
                  fixed_lambda=cs["fixed_lambda"])


def dynamics_of(pb):
    nl = pb["nl"]
    return O.CallableDyn(nl, nl.n_params) if nl.n_params else O.RandomWalkDyn()


def passes_of(cs):
    return 2 if cs["second_pass"] else 1


def reference(cs, pb):
    """The oracle over the passes and parts of the case.  Returns a list (one entry per part, in run order) of dicts: the state
    after the part (C, V, mu, P, Q, rho, lam, theta, gradsum), y_pred of the part, eta and N of its last step (None for an
    empty part); and the roll-out of three steps behind the last one."""
    mode, dyn = mode_of(cs), dynamics_of(pb)
    n_theta = dyn.n_theta
    Y, T = pb["Y"], cs["T"]
    st = O.State(C=pb["C0"].copy(), V=pb["V0"].copy(), mu=pb["mu0"].copy(), P=pb["P0"].copy(), Q=pb["Q"].copy(), rho=pb["rho"], lam=pb["lam"],
                 theta=pb["theta"].copy(), gradsum=np.zeros(n_theta))
    out = []
    for ep in range(passes_of(cs)):
        if ep and cs["robust"]:             # rPSMF's step_reset: Q, R, lambda start again (rpsmf.py:106-114)
            st.Q, st.rho, st.lam = pb["Q"].copy(), pb["rho"], pb["lam"]
        st.gradsum = np.zeros(n_theta)
        m = v = np.zeros(n_theta)
        for a, b in cs["parts"]:
            Yp = np.empty((b - a, cs["d"]))
            info = None
            for k in range(a + 1, b + 1):
                Qk = None if pb["q_k"] is None else pb["q_k"][k] * pb["Q"]
                rk = None if pb["rho_k"] is None else pb["rho_k"][k]
                st, info = O.lowrank_step(st, Y[k - 1], k, mode, dyn, Qk=Qk, rhok=rk, want_grad=n_theta > 0)
                Yp[k - a - 1] = info.y_pred
                if cs["recursive"] and k % cs["update_every"] == 0:          # psmf.py:299-304
                    if cs["recursive"] == 1:
                        st.theta, m, v = O.adam_update(st.theta, st.gradsum, m, v, k, lr=ADAM_LR)
                    else:
                        st.theta = O.sgd_update(st.theta, st.gradsum, lr=SGD_LR)
                    st.gradsum = np.zeros(n_theta)
            out.append(dict(ep=ep, a=a, b=b, C=st.C.copy(), V=st.V.copy(), mu=st.mu.copy(), P=st.P.copy(), Q=np.array(st.Q, dtype=float),
                            rho=float(st.rho), lam=float(st.lam), theta=st.theta.copy(), gradsum=st.gradsum.copy(), y_pred=Yp,
                            eta=None if info is None else info.eta, N=None if info is None else info.N))
    rollout = O.predict_rollout(st.C, st.mu, st.theta, dyn, T, 3)
    return out, rollout


STATE_KEYS = ("C", "V", "mu", "P", "y_pred")


def grad_response(ref0, ref1):
    """netlib.response on the gradient sums, over the parts where the oracle's is not zero (not just restarted by the optimiser)"""
    live = [(p0, p1) for p0, p1 in zip(ref0, ref1) if p0["gradsum"].size and np.max(np.abs(p0["gradsum"])) > 0]
    return netlib.response([p0 for p0, _ in live], [p1 for _, p1 in live], ("gradsum",))


def sensitivity(cs):
    """relerr between the oracle on the case's inputs and on inputs perturbed by a relative 2^-50 (float32 storage: 2^-23, after
    the rounding): the worst over C, V, mu, P, y_pred of every part, and the worst gradsum.  Raises what the oracle raises."""
    eps = 2.0 ** -23 if cs["storage"] == "f32" else 2.0 ** -50
    ref0, roll0 = reference(cs, problem(cs))
    ref1, roll1 = reference(cs, problem(cs, perturb=(cs["seed"] ^ 0x5EED, eps)))
    for part in ref0:
        netlib.require_finite(part, STATE_KEYS + ("gradsum",), f"case {cs['i']}")
    return netlib.response(ref0, ref1, STATE_KEYS), grad_response(ref0, ref1)


def admissible(cs):
    state, grad = sensitivity(cs)
    return state <= bar(cs) / 16 and grad <= gradsum_bar(cs) / 16, f"sensitivity {state:.2e} (bar {bar(cs):.0e}), gradsum {grad:.2e}"


def describe(cs):
    return f"T={cs['T']} {cs['storage']} {cs['dyn']} {cs['hooks']}"


# What `resolve` answers for the cases it does not leave alone, {i: (salt, times shortened)}: recorded here so that the device
# test need not run the oracle three times per case; tests/test_blocked_cases_cpu.py recomputes every entry (and every absence).
RESOLUTION = {16: (0, 1), 31: (0, 1), 37: (1, 0), 50: (1, 0), 97: (1, 0), 106: (1, 0), 130: (0, 1), 133: (0, 2), 151: (1, 0), 170: (1, 0)}


def resolve(i):
    """netlib.resolve on this net (halving not below B + 1): ((salt, times shortened), log)"""
    return netlib.resolve(i, case, shorten, admissible, describe)


def device_case(i):
    return netlib.device_case(i, case, shorten, RESOLUTION.get(i, (0, 0)))
