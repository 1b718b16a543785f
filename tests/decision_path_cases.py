"""Cases that drive psmf_blk_filter3 / filter3s through every exit of the step loop's inversion decision (F3_DECIDE,
rpsmf_amd/csrc/psmf_blk3.hip), at the smallest shapes that reach it.  Pure Python: tests/test_decision_path_cases_cpu.py checks
the conditioning of every case without a GPU, tests/test_hip_filter3_decision_paths.py runs the list on the device.

A case = a problem (rank, rows, PSMF / rPSMF, storage, seed; built by tests/blocked_cases.py like the cases of the random net,
with the observation noise rho_0 and the process noise q of the case) and a PATH: the diagnostic switches of DESIGN section 9
that make the decision leave by one particular exit, and what the counters of one pass must then say.  Two passes of
T = 2 B + 1 timesteps (B = the block length): the first from the initial state (its first step sweeps: nothing to start
from), the second on the carried state.  Every block's first step starts plainly (no start predictor) in every case.

    one     the residual of the start is below the tolerance at the first check: one iteration per timestep
    two     the first check fails, the second iteration is the last: two per timestep
    more    a tolerance so tight that the third barrier and its loop run: three or more per timestep
    sweep   a far bound so small that every start is given up: the direct sweep, then PSMF_NS_SKIP timesteps that sweep unasked
    any     no path asked for (d = 3: fewer rows than the rank)

Which exit a setting takes depends on the residuals the device meets, so the settings were chosen from runs of candidate
settings on an MI355X (`make_golden_decision_paths.py --probe` prints the counters of a grid of them):

  * At rho_0 = 1, q = 0.1 (the random net's problem) M changes by a tenth per step and a start is never closer than 1e-2:
    three to four iterations per timestep at the default tolerances, sweeps and failed starts in both passes.  These problems
    run the paths `more` and `sweep`.
  * At rho_0 = 1e6, q = 1e-3 (1e-4) the start predictor leaves about 1e-3: every steady step of a pass takes the same exit.
  * `one` exists with float32 storage only: accepting at the first check leaves the square of the start's residual as the
    error, 1e-6 at best here -- inside the float32 bar (1e-5), never inside the float64 one (1e-9).
  * rPSMF restarts Q, rho and lambda between the passes (rpsmf.py:106-114), so its second pass is a transient with a few
    sweeps; its `one` and `two` cases are asserted on the first pass.
"""

import numpy as np

import blocked_cases as BC

D_ROWS = 257            # not a multiple of any tile; d = 3 (fewer rows than the rank) for one case
SHAPES = {32: "psmf_blk_filter3", 20: "psmf_blk_filter3", 12: "psmf_blk_filter3s"}      # mask mode 0, mode 1, filter3s
SKIP_N = 2              # PSMF_NS_SKIP of the sweep path
QUIET = dict(rho=1e6, q=1e-3)
SWEEP_ENV = {"PSMF_NS_FAR": "1e-2", "PSMF_NS_SKIP": str(SKIP_N)}

# (robust, storage, path) -> (problem, environment, the pass whose counters show the path).  float64 storage accepts at 3e-7 by
# default, float32 at 3e-4 (fill_step_params, psmf_capi.hip).
SETTINGS = {
    (False, "f32", "one"): (QUIET, {"PSMF_NS_TOL": "1e-2"}, 1),
    (False, "f32", "two"): (QUIET, {}, 1),
    (False, "f64", "two"): (QUIET, {"PSMF_NS_TOL": "1e-4"}, 1),
    (True, "f32", "one"): (dict(rho=1e6, q=1e-4), {"PSMF_NS_TOL": "1e-3"}, 0),
    (True, "f64", "two"): (QUIET, {"PSMF_NS_TOL": "1e-4"}, 0),
    (False, "f64", "more"): ({}, {"PSMF_NS_TOL": "1e-12"}, 1),
    (True, "f64", "more"): ({}, {"PSMF_NS_TOL": "1e-12"}, 1),
    (False, "f64", "sweep"): ({}, SWEEP_ENV, 1),
    (True, "f64", "sweep"): ({}, SWEEP_ENV, 1),
    (False, "f64", "any"): ({}, {}, 1),
}


def make(name, r, robust, storage, path, d=D_ROWS, chain=True, salt=0, rho=None, q=None, env=None):
    B = BC.block_steps(r)
    pbkw, env0, on_pass = SETTINGS[(robust, storage, path)]
    env = dict(env0 if env is None else env)
    rho = pbkw.get("rho", 1.0) if rho is None else rho
    q = pbkw.get("q", 0.1) if q is None else q
    if r <= 16:
        env["PSMF_FILTER6_DUAL"] = "0"          # r <= 16 runs psmf_blk_filter6d by default; this puts filter3s in its place
    if not chain:
        env["PSMF_BLOCK_CHAIN"] = "0"           # one launch per block
    T = 2 * B + 1
    cs = dict(name=name, path=path, r=r, B=B, d=d, T=T, dyn="random_walk", robust=robust, storage=storage,
              v0=0.02 if storage == "f32" else 0.1, fixed_lambda=False, alpha=1.0, beta=1.0, general_Q=False, sched=False,
              hooks="full", recursive=0, update_every=1, env=env, second_pass=True, shards=None, parts=[(0, T)],
              # the series depends on (r, robust, storage, d) alone; the paths of one problem share its oracle run
              seed=770000 + 1000 * r + 100 * int(robust) + 10 * (storage == "f32") + (d != D_ROWS) + 7919 * salt,
              i=name, salt=salt, shortened=0, rho=float(rho), q=float(q), on_pass=on_pass)
    assert BC.expected_kernel(cs) == SHAPES[r], cs
    return cs


def problem_key(cs):
    return (cs["r"], cs["robust"], cs["storage"], cs["d"], cs["salt"], cs["rho"], cs["q"])


def problem(cs, perturb=None):
    """blocked_cases.problem with the case's observation noise rho_0 (psmf.py: R = rho I) in place of 1"""
    pb = BC.problem(cs, perturb=perturb)
    pb["rho"] = cs["rho"]
    pb["Q"] = cs["q"] * np.eye(cs["r"])
    return pb


def admissible(cs):
    """blocked_cases.admissible on `problem` above: (ok, the oracle's relative response to a last-bit change of the inputs)"""
    eps = 2.0 ** -23 if cs["storage"] == "f32" else 2.0 ** -50
    ref0, _ = BC.reference(cs, problem(cs))
    ref1, _ = BC.reference(cs, problem(cs, perturb=(cs["seed"] ^ 0x5EED, eps)))
    state = max(BC.relerr(p1[k], p0[k]) for p0, p1 in zip(ref0, ref1) for k in ("C", "V", "mu", "P", "y_pred"))
    return state <= BC.bar(cs) / 16, state


# name -> salt of the cases the conditioning check made redraw (at most one in eight; tests/test_decision_path_cases_cpu.py)
REDRAWN = {}


def cases():
    out = []

    def add(r, robust, storage, path, **kw):
        tag = f"r{r}-{'rPSMF' if robust else 'PSMF'}-{storage}-{path}" + ("-d3" if kw.get("d") == 3 else "") + ("" if kw.get("chain", True) else "-perblock")
        out.append(make(tag, r, robust, storage, path, salt=REDRAWN.get(tag, 0), **kw))

    for r in SHAPES:
        for robust, storage, path in SETTINGS:
            if path != "any":
                add(r, robust, storage, path)
    add(32, True, "f64", "two", chain=False)
    add(32, False, "f64", "sweep", chain=False)
    add(32, False, "f64", "any", d=3)
    return out


def expect(cs, passes):
    """None, or what is wrong with the counters (one dict per pass) for the path of the case"""
    for ep, cnt in enumerate(passes):
        if cnt["ns_steps"] + cnt["sweep_steps"] != cs["T"]:
            return f"pass {ep}: ns_steps + sweep_steps != T: {cnt}"
    cnt = passes[cs["on_pass"]]
    ns, sw, it, fl = cnt["ns_steps"], cnt["sweep_steps"], cnt["ns_iterations"], cnt["ns_failed"]
    first = 1 if cs["on_pass"] == 0 else 0          # the first step of the first pass sweeps: nothing to start from
    path = cs["path"]
    if path == "any":
        return None
    if path == "sweep":
        # every start fails; each failure is followed by SKIP_N unasked sweeps, fewer where its block ends first
        ok = ns == 0 and fl > 0 and fl < sw - first <= (1 + SKIP_N) * fl and it == fl
        return None if ok else f"sweep: {cnt}"
    if path == "more":
        # (failed starts count the checks they made, and are few: the problem's own transients)
        return None if it >= 3 * ns and 10 * fl <= cs["T"] else f"more: {it / max(ns, 1):.3f} iterations per iterated timestep, {cnt}"
    if sw != first or fl:
        return f"{path}: sweeps or failed starts in pass {cs['on_pass']}: {cnt}"
    # a block's first step starts without the predictor and may take an iteration or two more than the steady ones: 3 blocks
    if path == "one":
        return None if ns <= it <= ns + 6 else f"one: {it} iterations in {ns} timesteps"
    return None if 2 * ns - 3 <= it <= 2 * ns + 6 else f"two: {it} iterations in {ns} timesteps"
