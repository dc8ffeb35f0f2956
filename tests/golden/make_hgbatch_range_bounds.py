"""Writes tests/golden/hgbatch_range_bounds.json: what LAPACK's windowed driver (scipy.linalg.eigh(A, B, subset_by_index=...,
driver="gvx"), complex: zhegvx -- zpotrf, zhegst, zheevx, ztrsm) reaches on the case table of
tests/test_hgbatch_range_accuracy.py, measured against the extended-precision references of tests/hard_dense.py.  CPU only.  The
peer of a windowed solver is the windowed driver; the full drivers gv / gvd are recorded in
tests/golden/batch_accuracy_bounds.json and the bound in force takes the larger of the two.

The case table (case_table below, the one the test runs): the pencils hard_dense.pencil("hgev", n, f, c), f in PENCIL_A, c in
PENCIL_C, at n = 5 (the class of 32) with (1, 5, 'A'), (2, 4, 'A'), (1, 5, 'N'); at n = 33 (the class of 64, whose window kernel
serves 8 columns in mode 'A') with windows(33): the shape of hard_dense.windows, which is fixed at a width of 16, built with a
width of 8.  Mode 'N' records E_w alone.

    python tests/golden/make_hgbatch_range_bounds.py
"""
import json
import os
import sys

import numpy as np
import scipy
import scipy.linalg

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hard_dense as hd  # noqa: E402

BOUNDS_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hgbatch_range_bounds.json")
METRICS = ("E_w", "E_r", "E_o")
SIZES = (5, 33)
WINDOWS_5 = [(1, 5, "A"), (2, 4, "A"), (1, 5, "N")]
WIDTH = 8                                        # the widest window of mode 'A' at 33 <= n <= 64


def windows(n, mw=WIDTH):
    """(il, iu, mode) at size n.  n = 5: the three windows above.  Otherwise hard_dense.windows(n) with mw in the place of its
    window_width(n): the lowest and the highest mw, (1, 1), (n, n), mw in the middle starting and ending inside a cluster of
    hard_dense.half_integer_spectrum(n) (the one nearest the middle), and (1, n) in mode 'N'"""
    if n == 5:
        return list(WINDOWS_5)
    d = hd.half_integer_spectrum(n)
    inside = [il for il in range(2, n - mw + 1) if d[il - 2] == d[il - 1] and d[il + mw - 2] == d[il + mw - 1]]
    assert inside, n
    il = min(inside, key=lambda q: abs(q - (n - mw) // 2))
    return [(1, mw, "A"), (n - mw + 1, n, "A"), (1, 1, "A"), (n, n, "A"), (il, il + mw - 1, "A"), (1, n, "N")]


def case_table():
    """(n, family of A, c, il, iu, mode)"""
    return [(n, f, c, il, iu, mode) for n in SIZES for f in hd.PENCIL_A for c in hd.PENCIL_C for il, iu, mode in windows(n)]


def case_id(case):
    n, f, c, il, iu, mode = case
    return f"hgev-n{n}-{f}-c{c}-{il}-{iu}-{mode}"


def window_metrics(pc, w, Z, il):
    """(E_w, E_r, E_o) of hard_dense.pencil_metrics on the window; Z = None (mode 'N'): E_w alone, the others 0"""
    if Z is None:
        return hd.pencil_metrics(pc, w, np.zeros((pc.n, len(w)), dtype=np.complex128), None, il)[0], 0.0, 0.0
    return hd.pencil_metrics(pc, w, Z, None, il)[:3]


def lapack_case(case):
    n, f, c, il, iu, mode = case
    pc = hd.pencil("hgev", n, f, c)
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
    out = {"reference": "scipy.linalg.eigh(A, B, subset_by_index, driver='gvx') (zhegvx) vs the extended-precision references of "
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
