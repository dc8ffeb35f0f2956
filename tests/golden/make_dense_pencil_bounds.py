"""Writes tests/golden/dense_pencil_bounds.json: what LAPACK reaches on the case table of the dense generalised solvers
(tests/test_dense_pencil_accuracy.py), measured against the extended-precision references of tests/hard_dense.py.  CPU only.

  stages   potrf (E_f) on B = overlap(n, c); trtrs (E_t, both ops, n right-hand sides) and sygst / hegst (E_c, itype 1, upper)
           with potrf's factor, at every n of hard_dense.STAGE_SIZES and c of PENCIL_C, real and complex
  whole    scipy.linalg.eigh(A, B), drivers gv and gvd, and potrf for E_f, on hard_dense.dense_cases(kind)

The bound of a test is hard_dense.BOUND_FACTOR x the worst value per (kind, stage, metric), for the whole solves per cond group
c: it comes from an independent implementation of the same operation, never from the code under test.  The record of the
batched solvers (batch_accuracy_bounds.json) is not reused: its sizes differ, and what LAPACK reaches depends on the size.

"family_bounds" (empty unless a route needs it) holds bounds of a route's own, as "gev-spectral": {"bounds": {"c4": {"E_o":
...}}, "reason": ...}: 16 x what the numpy restatement of the route (tests/test_dense_pencil_accuracy.py) reaches where that
algorithm class legitimately exceeds 16 x LAPACK.  The generator keeps what the committed file holds there.

    python tests/golden/make_dense_pencil_bounds.py
"""
import json
import os
import sys

import numpy as np
import scipy
import scipy.linalg
import scipy.linalg.lapack

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hard_dense as hd  # noqa: E402

KINDS = ("gev", "hgev")
DRIVERS = ("gv", "gvd")


def stage_cases(what):
    """(n, c) for chol and trsm, (n, family of A, c) for reduce"""
    if what == "reduce":
        return [(n, f, c) for n in hd.STAGE_SIZES for f in hd.PENCIL_A for c in hd.PENCIL_C]
    return [(n, c) for n in hd.STAGE_SIZES for c in hd.PENCIL_C]


def stage_id(kind, what, case):
    if what == "reduce":
        return f"{kind}-reduce-n{case[0]}-{case[1]}-c{case[2]}"
    return f"{kind}-{what}-n{case[0]}-c{case[1]}"


def lapack_stage(kind, what, case):
    """{driver: [values]} of one stage case: potrf -> [E_f]; trtrs -> [E_t] per op; sygst / hegst -> [E_c]"""
    if what == "chol":
        st = hd.stage(kind, *case)
        return {"potrf": [hd.factor_error(st.B, st.U, st.bnorm)]}         # st.U is scipy.linalg.cholesky(B)
    if what == "trsm":
        st = hd.stage(kind, *case)
        n = st.n                                   # the first n right-hand sides (at n < 7 the stage holds 7)
        return {f"trtrs_{op}": [hd.solve_error(scipy.linalg.solve_triangular(st.U, st.R[:, :n], trans=op), st.X[op][:, :n])]
                for op in "NC"}
    rd = hd.reduction(kind, *case)
    gst = scipy.linalg.lapack.zhegst if kind == "hgev" else scipy.linalg.lapack.dsygst
    C, info = gst(rd.A, rd.st.U, itype=1, lower=0)
    assert info == 0
    return {"hegst" if kind == "hgev" else "sygst": [hd.reduction_error(rd, C)]}


def lapack_whole(kind, case, driver):
    """(E_w, E_r, E_o, E_f) of scipy.linalg.eigh(A, B) with potrf's factor on one pencil"""
    pc = hd.pencil(kind, *case)
    U = scipy.linalg.cholesky(pc.B)
    w, Z = scipy.linalg.eigh(pc.A, pc.B, driver=driver)
    return hd.pencil_metrics(pc, w, Z, U)


def main():
    per_case, worst = {}, {}
    for kind in KINDS:
        for what, names in hd.STAGES.items():
            group = worst.setdefault(kind, {}).setdefault(what, {})
            for case in stage_cases(what):
                rec = per_case[stage_id(kind, what, case)] = {d: [round(v, 3) for v in m]
                                                              for d, m in lapack_stage(kind, what, case).items()}
                for m in rec.values():
                    for k, v in zip(names, m):
                        group[k] = max(group.get(k, 0.0), v)
                print(stage_id(kind, what, case), rec, flush=True)
        for case in hd.dense_cases(kind):
            group = worst[kind].setdefault("whole", {}).setdefault(f"c{case[2]}", {})
            rec = per_case[hd.case_id(kind, case)] = {}
            for drv in DRIVERS:
                m = [round(v, 3) for v in lapack_whole(kind, case, drv)]
                rec[drv] = m
                for k, v in zip(hd.PENCIL_METRICS, m):
                    group[k] = max(group.get(k, 0.0), v)
            print(hd.case_id(kind, case), rec, flush=True)
    family_bounds = {}
    if os.path.exists(hd.DENSE_BOUNDS_JSON):
        family_bounds = json.load(open(hd.DENSE_BOUNDS_JSON)).get("family_bounds", {})
    out = {"reference": "scipy.linalg: cholesky (potrf), solve_triangular (trtrs), lapack.dsygst / zhegst, eigh(A, B) with drivers "
                        "gv / gvd, vs the extended-precision references of tests/hard_dense.py",
           "unit": "eps = 2^-52; the normalisations of hard_dense.factor_error, solve_error, reduction_error and pencil_metrics",
           "metrics": {"chol": hd.STAGES["chol"], "trsm": hd.STAGES["trsm"], "reduce": hd.STAGES["reduce"],
                       "whole": hd.PENCIL_METRICS},
           "factor": hd.BOUND_FACTOR, "numpy": np.__version__, "scipy": scipy.__version__, "worst": worst,
           "family_bounds": family_bounds, "per_case": per_case}
    with open(hd.DENSE_BOUNDS_JSON, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("worst:", json.dumps(worst, indent=1))


if __name__ == "__main__":
    main()
