"""Records tests/golden/filter3_step_paths_parent.npz: what a build of the library leaves for every case of
tests/test_hip_filter3_step_paths.py (counters of both passes, blake2b digests of every array).  Run once, on an MI355X, on the
build of the commit whose results are to be kept -- the parent of the commit that re-laid the step loop of psmf_blk_filter3:

    python tests/golden/make_golden_step_paths.py tests/golden/filter3_step_paths_parent.npz [LIBRARY]

LIBRARY: the libpsmf_hip.so to record (default: the one in rpsmf_amd/lib).  Prints, per case, the counters per timestep, whether
the case took the path it is named for, and the worst error against the float64 oracle as a fraction of the bar."""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_hip_filter3_step_paths as TS    # noqa: E402


def main():
    from rpsmf_amd import _capi as c

    if len(sys.argv) > 2:
        c.LIB_PATH = os.path.abspath(sys.argv[2])
    print("library:", c.LIB_PATH, "build id", c.load_library().psmf_build_id().decode()[:16])
    rec = {}
    for cs in TS.CASES:
        pb, ref = TS.reference(cs)
        passes = TS.drive(c, cs, pb)
        T = cs["T"]
        per = " | ".join(f"it {p['counters']['ns_iterations'] / T:.3f} sw {p['counters']['sweep_steps'] / T:.3f} fl {p['counters']['ns_failed'] / T:.3f}" for p in passes)
        worst = max(e[2] / e[3] for e in TS.errors(cs, passes, ref))
        print(f"{cs['name']:40s} T={T} env={cs['env']} :: {per} :: err/bar {worst:.3g} ::",
              TS.expect(cs, [p["counters"] for p in passes]) or "path ok", flush=True)
        for k, v in TS.record_of(passes).items():
            rec[f"{cs['name']}/{k}"] = v
    np.savez_compressed(sys.argv[1], **rec)


if __name__ == "__main__":
    main()
