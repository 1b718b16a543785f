#!/usr/bin/env python
"""Generate tests/golden/impute_kat_bpmf.npz: the known answers the reference stores for its BPMF baseline.

    python tests/golden/make_golden_pmf.py REFERENCE_ROOT

Build container only (the reference does not exist on the GPU box).  Recorded results alone are written: for the nine files
ExperimentImpute/output/<dataset>_<pct>_BPMF.json whose data the fixtures impute_kat_{pm25,pm10,sp500}.npz hold -- LondonAir_PM25,
LondonAir_PM10 and sp500_closing_prices at 20 / 30 / 40 % missing -- the `error_full` of all 100 repeats and the input hashes (Y, C,
X) of every repeat, under the keys <ds>_<pct>_error_full and <ds>_<pct>_hash_{Y,C,X}; plus the seed and the parameters of each
file.  `error_predict` is NaN in every repeat (BPMF predicts nothing online) and is not stored."""

import json
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
DATASETS = {"pm25": "LondonAir_PM25", "pm10": "LondonAir_PM10", "sp500": "sp500_closing_prices"}
PCTS = (20, 30, 40)


def main(ref):
    out = {}
    for ds, dataset in DATASETS.items():
        for pct in PCTS:
            with open(os.path.join(ref, "ExperimentImpute", "output", f"{dataset}_{pct}_BPMF.json")) as fp:
                j = json.load(fp)
            assert j["method"] == "BPMF" and j["seed"] == 123 and j["missing_percentage"] == pct, (ds, pct)
            key = f"{ds}_{pct}"
            ef = np.array(j["results"]["error_full"], dtype=float)
            assert ef.shape == (100,) and np.all(np.isfinite(ef)), key
            assert all(v is None or v != v for v in j["results"]["error_predict"]), key
            out[f"{key}_error_full"] = ef
            for name in ("Y", "C", "X"):
                h = np.array(j["hashes"][name])
                assert h.shape == (100,), (key, name)
                out[f"{key}_hash_{name}"] = h
            out[f"{key}_params"] = json.dumps(j["parameters"])
    path = os.path.join(OUT, "impute_kat_bpmf.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
