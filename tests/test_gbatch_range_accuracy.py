"""The window kernel of eigen_gev_batch_range (route key 26 = 1) held to LAPACK-level accuracy on the small hard pencils of
tests/hard_dense.py, after tests/test_hbatch_range_accuracy.py: hd.pencil("gev", n, f, c) for f in hd.PENCIL_A and c in
hd.PENCIL_C, the m columns judged by hd.pencil_metrics(pc, w, Z, U, il) against the 50-digit reference, E_f on the returned U.

n = 5 gets (1, 5, 'A'), (2, 4, 'A') and (1, 5, 'N') (hd.windows has no cluster to offer at 5); n = 33 and 64 the windows of
hd.windows(n), built with MW = 16 there: the lowest and the highest 16, (1, 1), (n, n), 16 in the middle starting and ending
inside a cluster of the half_integer spectrum, and (1, n) in mode 'N'; n = 96, the class without window storage, (1, 96, 'N') with
c = 4 only, as hd.cases("gev") has it.  These are the sizes whose references tests/test_batch_accuracy.py computes already.

Bounds, none invented: per metric and cond group, hd.BOUND_FACTOR (16) x max(what LAPACK's windowed driver gvx reaches on exactly
this case table: tests/golden/gbatch_range_bounds.json, written by tests/golden/make_gbatch_range_bounds.py; what gv / gvd reach
on the gev table of tests/golden/batch_accuracy_bounds.json).  E_f takes the existing gev bound.  A bound of 0 asks for exactly
0: every comparison is <=.  A pencil the acceptance test sends to the redo is judged like any other."""
import importlib.util
import json
import os

import numpy as np
import pytest

import hard_dense as hd

SIZES = (5, 33, 64, 96)


def _generator():
    spec = importlib.util.spec_from_file_location("make_gbatch_range_bounds",
                                                  os.path.join(os.path.dirname(hd.BOUNDS_JSON), "make_gbatch_range_bounds.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def _bounds(gen, c):
    """{metric: bound} of cond group c"""
    rec = json.load(open(gen.BOUNDS_JSON))
    old = hd.bounds("gev", c=c)
    out = {k: hd.BOUND_FACTOR * max(rec["worst"][f"c{c}"][k], old[k] / hd.BOUND_FACTOR) for k in gen.METRICS}
    out["E_f"] = old["E_f"]
    return out


def test_the_bounds_record_covers_the_case_table():
    """the committed JSON holds every case of the table, its worst values are the maxima of its cases per cond group, the bound in
    force is never under the existing gev bound, and gvx recomputed on two small cases is at or under the record"""
    gen = _generator()
    rec = json.load(open(gen.BOUNDS_JSON))
    assert rec["factor"] == hd.BOUND_FACTOR and rec["metrics"] == list(gen.METRICS)
    table = gen.case_table()
    assert set(rec["per_case"]) == {gen.case_id(c) for c in table} and len(table) == len(rec["per_case"])
    assert {c[0] for c in table} == set(SIZES) and {c[2] for c in table if c[0] == 96} == {4}
    for grp in hd.PENCIL_C:
        rows = [rec["per_case"][gen.case_id(c)] for c in table if c[2] == grp]
        assert rec["worst"][f"c{grp}"] == {k: max(r[q] for r in rows) for q, k in enumerate(gen.METRICS)}, grp
        bnd, old = _bounds(gen, grp), hd.bounds("gev", c=grp)
        assert all(bnd[k] >= old[k] for k in hd.PENCIL_METRICS) and bnd["E_f"] == old["E_f"]
    # (a c = 4 case that stays well under the worst of its group: B goes through LAPACK's QR and differs in its last bits from
    # machine to machine, and with it what LAPACK reaches on a pencil; and the exact case B = I at n = 5)
    for case in [(33, "random", 4, 1, 16, "A"), (5, "random", 0, 2, 4, "A")]:
        worst = rec["worst"][f"c{case[2]}"]
        for k, v in zip(gen.METRICS, gen.lapack_case(case)):
            assert round(float(v), 3) <= max(worst[k], hd.bounds("gev", c=case[2])[k] / hd.BOUND_FACTOR), (case, k, v)


def test_the_in_cluster_window_exists():
    """hard_dense.windows is built with MW = 16 at these sizes, and its fifth window starts and ends inside a cluster of the
    half_integer spectrum"""
    assert [hd.window_width(n) for n in (33, 64)] == [16, 16]
    assert [hd.windows(n)[4] for n in (33, 64)] == [(7, 22, "A"), (24, 39, "A")]
    for n in (33, 64):
        d = hd.half_integer_spectrum(n)
        il, iu, _ = hd.windows(n)[4]
        assert d[il - 2] == d[il - 1] and d[iu - 1] == d[iu]
        assert hd.windows(n)[-1] == (1, n, "N")


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_windows(gpu_lib, n):
    """every pencil of one size under each of its windows, one call per window, route 1 asserted; E_w, E_r, E_o and E_f (mode
    'N': E_w and E_f) at or under the bound of the pencil's cond group"""
    import test_gbatch_range as tr
    from test_batch_accuracy import _judge

    gen = _generator()
    table = [c for c in gen.case_table() if c[0] == n]
    pencils = list(dict.fromkeys((c[1], c[2]) for c in table))
    pcs = [hd.pencil("gev", n, f, c) for f, c in pencils]
    redone = 0
    with tr._Key(gpu_lib, 26, 1):
        for il, iu, mode in gen.windows(n):
            P = tr.RPencils([p.A for p in pcs], [p.B for p in pcs], il, iu)
            assert P.run(gpu_lib, mode=mode.encode(), z=mode == "A") == 0
            route, m, rd = tr._range_info(gpu_lib)
            assert route == 1 and m == iu - il + 1
            redone += rd
            w, Z, U, info, _ = P.results(want_z=mode == "A")
            assert (info == 0).all()
            for k, pc in enumerate(pcs):
                tag = f"{pc.family} c={pc.c} n={n} {il}..{iu} {mode}"
                assert np.isfinite(w[k]).all() and np.isfinite(U[k]).all() and (mode == "N" or np.isfinite(Z[k]).all()), tag
                assert (np.diff(w[k]) >= 0).all(), f"{tag}: w is not ascending"
                bnd = _bounds(gen, pc.c)
                if mode == "A":
                    _judge("gwindow", tag, hd.PENCIL_METRICS, hd.pencil_metrics(pc, w[k], Z[k], U[k], il), bnd)
                else:
                    v = hd.pencil_metrics(pc, w[k], np.zeros((n, m)), U[k], il)
                    _judge("gwindow", tag, ("E_w", "E_f"), (v[0], v[3]), bnd)
    print(f"BATCH-ACC gwindow n={n}: {redone} pencils redone by route 2")
