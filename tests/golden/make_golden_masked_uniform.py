"""Writes tests/golden/masked_uniform_parent.npz: C and X of the uniform masked handle (nonuniform_R = 0) for the (40, 90, 24)
PSMF case of tests/masked_noise_cases.py with R = 10 I, float64 storage, two passes each cut in two runs, on the handle's default
route and on the launched form (tests/test_hip_masked_row_noise.py::uniform_parent_runs).  The fixture pins the BITS of the commit
before the masked Gram's count slot learnt to carry sum m_i rho_i, so it was written by running this script on an MI355X against the
library built from that commit (its rpsmf_amd package in front on PYTHONPATH):

    PYTHONPATH=<checkout of the parent commit, built> python tests/golden/make_golden_masked_uniform.py [out.npz]

Run it again only to pin a deliberate change of those bits."""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.append(os.path.dirname(TESTS))          # behind PYTHONPATH: the package under test may be another checkout's

if __name__ == "__main__":
    from rpsmf_amd import _capi as c
    from test_hip_masked_row_noise import uniform_parent_runs

    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "masked_uniform_parent.npz")
    runs = uniform_parent_runs(c)
    np.savez(out, **runs)
    print(out, {k: (str(v) if v.ndim == 0 else v.shape) for k, v in runs.items()}, "library:", c.load_library().psmf_build_id().decode()[:16])
