"""Writes tests/golden/gbatch_range_bounds.json: what LAPACK's windowed driver (scipy.linalg.eigh(A, B, subset_by_index=...,
driver="gvx"): potrf, sygst, syevx, trsm) reaches on the case table of tests/test_gbatch_range_accuracy.py, measured against the
extended-precision references of tests/hard_dense.py.  CPU only.  The peer of a windowed solver is the windowed driver; the full
drivers gv / gvd are recorded in tests/golden/batch_accuracy_bounds.json and the bound in force takes the larger of the two.

The case table (case_table below, the one the test runs): the pencils hard_dense.pencil("gev", n, f, c), f in PENCIL_A, c in
PENCIL_C, at n = 5 with (1, 5, 'A'), (2, 4, 'A'), (1, 5, 'N'); at n = 33 and 64 with hard_dense.windows(n); at n = 96 with
(1, 96, 'N') and c = 4 only.  Mode 'N' records E_w alone.

    python tests/golden/make_gbatch_range_bounds.py
"""
import json
import os
import sys

import numpy as np
import scipy
import scipy.linalg

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hard_dense as hd  # noqa: E402

BOUNDS_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gbatch_range_bounds.json")
METRICS = ("E_w", "E_r", "E_o")
WINDOWS_5 = [(1, 5, "A"), (2, 4, "A"), (1, 5, "N")]


def windows(n):
    """(il, iu, mode) at size n"""
    if n == 5:
        return list(WINDOWS_5)
    if n == 96:
        return [(1, 96, "N")]
    return hd.windows(n)


def case_table():
    """(n, family of A, c, il, iu, mode)"""
    return [(n, f, c, il, iu, mode) for n in (5, 33, 64, 96) for f in hd.PENCIL_A for c in ((4,) if n == 96 else hd.PENCIL_C)
            for il, iu, mode in windows(n)]


def case_id(case):
    n, f, c, il, iu, mode = case
    return f"gev-n{n}-{f}-c{c}-{il}-{iu}-{mode}"


def window_metrics(pc, w, Z, il):
    """(E_w, E_r, E_o) of hard_dense.pencil_metrics on the window; Z = None (mode 'N'): E_w alone, the others 0"""
    if Z is None:
        return hd.pencil_metrics(pc, w, np.zeros((pc.n, len(w))), None, il)[0], 0.0, 0.0
    return hd.pencil_metrics(pc, w, Z, None, il)[:3]


def lapack_case(case):
    n, f, c, il, iu, mode = case
    pc = hd.pencil("gev", n, f, c)
    if mode == "N":
        w = scipy.linalg.eigh(pc.A, pc.B, subset_by_index=(il - 1, iu - 1), driver="gvx", eigvals_only=True)
        return window_metrics(pc, w, None, il)
    w, Z = scipy.linalg.eigh(pc.A, pc.B, subset_by_index=(il - 1, iu - 1), driver="gvx")
    return window_metrics(pc, w, Z, il)


def main():
    per_case, worst = {}, {}
    for case in case_table():
        m = [round(float(v), 3) for v in lapack_case(case)]
        per_case[case_id(case)] = m
        group = worst.setdefault(f"c{case[2]}", {k: 0.0 for k in METRICS})
        for k, v in zip(METRICS, m):
            group[k] = max(group[k], v)
        print(case_id(case), m, flush=True)
    out = {"reference": "scipy.linalg.eigh(A, B, subset_by_index, driver='gvx') vs the extended-precision references of "
                        "tests/hard_dense.py",
           "unit": "eps = 2^-52; the normalisations of hard_dense.pencil_metrics on the columns of the window",
           "metrics": list(METRICS), "factor": hd.BOUND_FACTOR, "numpy": np.__version__, "scipy": scipy.__version__,
           "lapack": str(scipy.linalg.lapack.ilaver()) if hasattr(scipy.linalg.lapack, "ilaver") else "as linked by scipy",
           "worst": worst, "per_case": per_case}
    with open(BOUNDS_JSON, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("worst:", json.dumps(worst, indent=1))


if __name__ == "__main__":
    main()
