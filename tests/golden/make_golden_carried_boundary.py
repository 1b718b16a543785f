"""Records tests/golden/carried_boundary_parent.npz: what a build of the library leaves for every case of
tests/test_hip_carried_boundary.py (per pass the integer counters of every run and a blake2b digest of every array).  Run once, on
an MI355X, on the build of the commit whose results are to be kept -- the parent of the commit that shortened the carried boundary:

    python tests/golden/make_golden_carried_boundary.py tests/golden/carried_boundary_parent.npz [TREE]

TREE: the root of the checkout whose built `rpsmf_amd` package is recorded (default: the one this file lies in); the cases and
the problems are this file's tree's in either case.  Prints the counters of every case."""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TREE = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else ROOT
sys.path[:0] = [TREE, os.path.dirname(HERE)]

import test_hip_carried_boundary as TB    # noqa: E402


def main():
    from rpsmf_amd import _capi as c

    assert os.path.abspath(c.__file__).startswith(TREE + os.sep), (c.__file__, TREE)
    print("library:", c.LIB_PATH, "build id", c.load_library().psmf_build_id().decode()[:16])
    rec = {}
    for cs in TB.CASES:
        passes = TB.drive(c, cs)
        print(f"{cs['name']:24s} B={cs['B']} T={cs['T']} :: " + " | ".join(str(p["counters"]) for p in passes), flush=True)
        for k, v in TB.record_of(passes).items():
            rec[f"{cs['name']}/{k}"] = v
    np.savez_compressed(sys.argv[1], **rec)


if __name__ == "__main__":
    main()
