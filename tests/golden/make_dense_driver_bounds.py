"""Writes tests/golden/dense_driver_bounds.json: what LAPACK reaches on the case table of the dense standard drivers and their
stages (tests/test_dense_driver_accuracy.py), measured against the extended-precision references of tests/hard_dense.py.  CPU
only.  Per (kind, n, family) of hard_dense.driver_problems, kind s (real symmetric) and h (complex Hermitian):

  reduce   dsytrd / zhetrd (lower = 1) with Q formed as dorgtr / zungtr form it (dorgqr / zungqr on the block c[1:, :n-1],
           bordered by a unit row and column): E_s, E_q of hard_dense.similarity_metrics, for kind s against the returned (d, e),
           for kind h against the real tridiagonal part of Q^H A Q itself (the Hermitian driver returns no (d, e))
  trbak    dormqr / zunmqr with those reflectors on the three Z of hard_dense.back_input, against the same reflectors applied
           one by one in longdouble: E_b
  whole    numpy.linalg.eigh (syevd / heevd): E_w, E_r, E_o of hard_dense.metrics

The bound of a test is hard_dense.BOUND_FACTOR x the worst value per (kind, stage, metric): it comes from an independent
implementation of the same operation, never from the code under test.  The pentadiagonal reduction (band 2) has no LAPACK
counterpart and uses the same record: the metrics do not depend on the band width.

"family_bounds" (empty unless a family needs it) holds bounds of a family's own, as "s-graded": {"bounds": {"reduce": {"E_s":
...}}, "reason": ..., "measured": ...}.  The generator keeps what the committed file holds there.

    python tests/golden/make_dense_driver_bounds.py
"""
import json
import os
import sys

import numpy as np
import scipy
import scipy.linalg.lapack as lapack

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hard_dense as hd  # noqa: E402

KINDS = ("s", "h")
LD = hd.LD


def problem_id(kind, n, family):
    return f"{kind}-n{n}-{family}"


def _sig(v):
    """4 significant digits"""
    return float(f"{v:.4g}")


def lapack_reduce(A):
    """sytrd / hetrd of the lower triangle: (d, e, c, tau), A = Q T Q^H with Q = H_1 ... H_(n-1), H_i = I - tau_i v v^H, v = (1,
    c[i+2:, i]) on the rows i + 1 .. n - 1"""
    trd = lapack.zhetrd if np.iscomplexobj(A) else lapack.dsytrd
    c, d, e, tau, info = trd(np.asfortranarray(A), lower=1)
    assert info == 0
    return d, e, c, tau


def form_q(c, tau):
    """Q as orgtr forms it from a lower reduction: orgqr on c[1:, :n-1], bordered by a unit row and column"""
    n = c.shape[0]
    Q = np.eye(n, dtype=c.dtype)
    if n > 1:
        gqr = lapack.zungqr if np.iscomplexobj(c) else lapack.dorgqr
        q1, _, info = gqr(np.asfortranarray(c[1:, :n - 1]), tau)
        assert info == 0
        Q[1:, 1:] = q1
    return Q


def apply_q(c, tau, Z):
    """Q Z by ormqr / unmqr"""
    n = c.shape[0]
    out = np.array(Z, dtype=c.dtype, order="F")
    if n > 1:
        mqr = lapack.zunmqr if np.iscomplexobj(c) else lapack.dormqr
        blk = np.asfortranarray(c[1:, :n - 1])
        _, work, info = mqr("L", "N", blk, tau, np.asfortranarray(out[1:]), -1)
        assert info == 0
        cq, _, info = mqr("L", "N", blk, tau, np.asfortranarray(out[1:]), int(work[0].real))
        assert info == 0
        out[1:] = cq
    return out


def apply_q_ld(c, tau, Z):
    """Q Z = H_1 (H_2 ( ... H_(n-1) Z)) reflector by reflector in longdouble / clongdouble"""
    T = np.clongdouble if np.iscomplexobj(c) else LD
    n = c.shape[0]
    X = np.array(Z, dtype=T)
    cl, tl = np.asarray(c, dtype=T), np.asarray(tau, dtype=T)
    for i in range(n - 2, -1, -1):
        if tl[i] == 0:
            continue
        v = np.r_[T(1), cl[i + 2:, i]]
        X[i + 1:] -= np.outer(tl[i] * v, v.conj() @ X[i + 1:])
    return X


def lapack_problem(kind, n, family):
    """{"reduce": [E_s, E_q], "trbak": [E_b per Z of hard_dense.BACK_INPUTS], "whole": [E_w, E_r, E_o]} of LAPACK on one
    problem"""
    cs = hd.case(kind, n, family)
    d, e, c, tau = lapack_reduce(cs.A)
    Q = form_q(c, tau)
    T = None if kind == "h" else np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
    red = hd.similarity_metrics(cs.A, Q, T, cs.anorm)
    bak = [hd.solve_error(apply_q(c, tau, Z), apply_q_ld(c, tau, Z))
           for Z in (hd.back_input(n, which, kind == "h") for which in hd.BACK_INPUTS)]
    w, Z = np.linalg.eigh(cs.A)
    return {"reduce": list(red), "trbak": bak, "whole": list(hd.metrics(cs, w, Z))}


def worst_of(per_case):
    """the maximum per (kind, stage, metric) over the recorded cases"""
    worst = {}
    for kind in KINDS:
        for what, names in hd.DRIVER_STAGES.items():
            rows = [per_case[problem_id(kind, n, f)][what] for n, f in hd.driver_problems(kind)]
            if what == "trbak":
                worst.setdefault(kind, {})[what] = {"E_b": max(max(r) for r in rows)}
            else:
                worst.setdefault(kind, {})[what] = {k: max(r[q] for r in rows) for q, k in enumerate(names)}
    return worst


def main():
    per_case = {}
    for kind in KINDS:
        for n, family in hd.driver_problems(kind):
            rec = per_case[problem_id(kind, n, family)] = {k: [_sig(v) for v in m]
                                                           for k, m in lapack_problem(kind, n, family).items()}
            print(problem_id(kind, n, family), rec, flush=True)
    worst = worst_of(per_case)
    family_bounds = {}
    if os.path.exists(hd.DRIVER_BOUNDS_JSON):
        family_bounds = json.load(open(hd.DRIVER_BOUNDS_JSON)).get("family_bounds", {})
    out = {"reference": "scipy.linalg.lapack dsytrd / zhetrd + dorgqr / zungqr (reduce), dormqr / zunmqr vs the same reflectors in "
                        "longdouble (trbak), numpy.linalg.eigh (whole), vs the extended-precision references of tests/hard_dense.py",
           "unit": "eps = 2^-52; the normalisations of hard_dense.similarity_metrics, solve_error and metrics",
           "metrics": {k: list(v) for k, v in hd.DRIVER_STAGES.items()}, "back_inputs": list(hd.BACK_INPUTS),
           "factor": hd.BOUND_FACTOR, "numpy": np.__version__, "scipy": scipy.__version__,
           "lapack": ".".join(str(v) for v in lapack.ilaver()), "worst": worst, "family_bounds": family_bounds,
           "per_case": per_case}
    with open(hd.DRIVER_BOUNDS_JSON, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("worst:", json.dumps(worst, indent=1))


if __name__ == "__main__":
    main()
