"""Writes tests/golden/dc_hard_bounds.json: what LAPACK's own divide and conquer (numpy.linalg.eigh on the dense band
matrix) reaches on the whole case table of tests/hard_band.py, measured against the extended-precision reference.  CPU only.

The bound of tests/test_dc_hard.py is hard_band.BOUND_FACTOR x the worst value per metric, independent of n: it comes from
an independent implementation of the same operation, never from the code under test.

    python tests/golden/make_dc_hard_bounds.py
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hard_band as hb  # noqa: E402


def lapack_case(band, n, name):
    d, e, w_ref = hb.case(name, n, band)
    w, Z = np.linalg.eigh(hb.band_matrix(d, e, band))
    return hb.metrics(d, e, band, w, Z, w_ref)


def main():
    per_case = {}
    worst = {"E_w": 0.0, "E_r": 0.0, "E_o": 0.0}
    for band, n, name in hb.cases():
        m = lapack_case(band, n, name)
        per_case[f"band{band}-n{n}-{name}"] = [round(v, 3) for v in m]
        for k, v in zip(worst, m):
            worst[k] = max(worst[k], round(v, 3))
        print(f"band={band} n={n:5d} {name:15s} E_w={m[0]:7.2f} E_r={m[1]:7.2f} E_o={m[2]:7.2f}", flush=True)
    out = {"reference": "numpy.linalg.eigh (LAPACK D&C) on the dense band matrix vs hard_band.reference_eigenvalues",
           "unit": "eps = 2^-52 (E_w, E_r also per |T|_2)", "factor": hb.BOUND_FACTOR,
           "numpy": np.__version__, "worst": worst, "per_case": per_case}
    with open(hb.BOUNDS_JSON, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("worst:", worst)


if __name__ == "__main__":
    main()
