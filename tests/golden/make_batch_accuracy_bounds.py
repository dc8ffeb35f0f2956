"""Writes tests/golden/batch_accuracy_bounds.json: what LAPACK (scipy.linalg.eigh, drivers ev and evd for the standard problems,
gv and gvd for the pencils; potrf for the factor) reaches on the whole case table of tests/hard_dense.py, measured against the
extended-precision references.  CPU only.  evr is left out: its orthogonality is that of MRRR (1538 eps on the graded family),
and the kernels under test are not MRRR.

The bound of tests/test_batch_accuracy.py is hard_dense.BOUND_FACTOR x the worst value per (kind, metric), for the pencils per
cond group: it comes from an independent implementation of the same operation, never from the code under test.  The window
kind uses the bounds of s: the same operation on a column subset.

"family_bounds" (empty unless a family needs it) holds bounds of a family's own, 16 x what the numpy restatement of the
kernels' algorithm class (tests/test_batch_accuracy.py::tred2_tql2) reaches where that class legitimately exceeds 16 x LAPACK,
with the reason.  The generator keeps what the committed file holds there.

    python tests/golden/make_batch_accuracy_bounds.py
"""
import json
import os
import sys

import numpy as np
import scipy
import scipy.linalg

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hard_dense as hd  # noqa: E402

DRIVERS = {"s": ("ev", "evd"), "h": ("ev", "evd"), "gev": ("gv", "gvd"), "hgev": ("gv", "gvd")}


def lapack_case(kind, case, driver):
    """the metrics LAPACK reaches on one case of the table (kind s, h, gev or hgev)"""
    if kind in ("s", "h"):
        cs = hd.case(kind, *case)
        w, Z = scipy.linalg.eigh(cs.A, driver=driver)
        return hd.metrics(cs, w, Z)
    pc = hd.pencil(kind, *case)
    U = scipy.linalg.cholesky(pc.B)             # potrf has to accept every B of the table (LinAlgError otherwise)
    w, Z = scipy.linalg.eigh(pc.A, pc.B, driver=driver)
    return hd.pencil_metrics(pc, w, Z, U)


def main():
    per_case, worst = {}, {}
    for kind, drivers in DRIVERS.items():
        names = hd.METRICS if kind in ("s", "h") else hd.PENCIL_METRICS
        for case in hd.cases(kind):
            group = worst.setdefault(kind, {})
            if kind in ("gev", "hgev"):
                group = group.setdefault(f"c{case[2]}", {})
            rec = per_case[hd.case_id(kind, case)] = {}
            for drv in drivers:
                m = [round(v, 3) for v in lapack_case(kind, case, drv)]
                rec[drv] = m
                for k, v in zip(names, m):
                    group[k] = max(group.get(k, 0.0), v)
            print(hd.case_id(kind, case), rec, flush=True)
    family_bounds = {}
    if os.path.exists(hd.BOUNDS_JSON):
        family_bounds = json.load(open(hd.BOUNDS_JSON)).get("family_bounds", {})
    out = {"reference": "scipy.linalg.eigh (LAPACK ev / evd, gv / gvd; potrf for E_f) vs the extended-precision references of "
                        "tests/hard_dense.py",
           "unit": "eps = 2^-52; the normalisations of hard_dense.metrics and hard_dense.pencil_metrics",
           "metrics": {"s": hd.METRICS, "h": hd.METRICS, "gev": hd.PENCIL_METRICS, "hgev": hd.PENCIL_METRICS},
           "factor": hd.BOUND_FACTOR, "numpy": np.__version__, "scipy": scipy.__version__, "worst": worst,
           "family_bounds": family_bounds, "per_case": per_case}
    with open(hd.BOUNDS_JSON, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("worst:", json.dumps(worst, indent=1))


if __name__ == "__main__":
    main()
