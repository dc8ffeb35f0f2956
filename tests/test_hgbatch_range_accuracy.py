"""The window kernel of eigen_hgev_batch_range (route key 26 = 1) held to LAPACK-level accuracy on the small hard pencils of
tests/hard_dense.py, after tests/test_gbatch_range_accuracy.py: hd.pencil("hgev", n, f, c) for f in hd.PENCIL_A and c in
hd.PENCIL_C, the m columns judged by hd.pencil_metrics(pc, w, Z, U, il) against the 50-digit reference, E_f on the returned U.

n = 5 (the class of 32) gets (1, 5, 'A'), (2, 4, 'A') and (1, 5, 'N'); n = 33 (the class of 64, whose kernel serves 8 columns in
mode 'A') the shape of hd.windows built with a width of 8 by the generator's windows(33): the lowest and the highest 8, (1, 1),
(33, 33), 8 in the middle starting and ending inside a cluster of the half_integer spectrum, and (1, 33) in mode 'N'.  Both sizes
are in hd.SIZES["hgev"]: their references are the ones tests/test_batch_accuracy.py computes already.

Bounds, none invented: per metric and cond group, hd.BOUND_FACTOR (16) x max(what LAPACK's windowed driver gvx (zhegvx) reaches on
exactly this case table: tests/golden/hgbatch_range_bounds.json, written by tests/golden/make_hgbatch_range_bounds.py; what gv /
gvd reach on the hgev table of tests/golden/batch_accuracy_bounds.json).  E_f takes the existing hgev bound.  A bound of 0 asks
for exactly 0: every comparison is <=.  A pencil the acceptance test sends to the redo is judged like any other."""
import importlib.util
import json
import os

import numpy as np
import pytest

import hard_dense as hd

SIZES = (5, 33)


def _generator():
    spec = importlib.util.spec_from_file_location("make_hgbatch_range_bounds",
                                                  os.path.join(os.path.dirname(hd.BOUNDS_JSON), "make_hgbatch_range_bounds.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def _bounds(gen, c):
    """{metric: bound} of cond group c"""
    rec = json.load(open(gen.BOUNDS_JSON))
    old = hd.bounds("hgev", c=c)
    out = {k: hd.BOUND_FACTOR * max(rec["worst"][f"c{c}"][k], old[k] / hd.BOUND_FACTOR) for k in gen.METRICS}
    out["E_f"] = old["E_f"]
    return out


def test_the_bounds_record_covers_the_case_table():
    """the committed JSON holds every case of the table, its worst values are the maxima of its cases per cond group, the bound in
    force is never under the existing hgev bound, and gvx recomputed on two small cases is at or under the record"""
    gen = _generator()
    rec = json.load(open(gen.BOUNDS_JSON))
    assert rec["factor"] == hd.BOUND_FACTOR and rec["metrics"] == list(gen.METRICS)
    table = gen.case_table()
    assert set(rec["per_case"]) == {gen.case_id(c) for c in table} and len(table) == len(rec["per_case"])
    assert {c[0] for c in table} == set(SIZES) == set(gen.SIZES) and set(SIZES) <= set(hd.SIZES["hgev"])
    for grp in hd.PENCIL_C:
        rows = [rec["per_case"][gen.case_id(c)] for c in table if c[2] == grp]
        assert rec["worst"][f"c{grp}"] == {k: max(r[q] for r in rows) for q, k in enumerate(gen.METRICS)}, grp
        bnd, old = _bounds(gen, grp), hd.bounds("hgev", c=grp)
        assert all(bnd[k] >= old[k] for k in hd.PENCIL_METRICS) and bnd["E_f"] == old["E_f"]
    # (a c = 4 case that stays well under the worst of its group: B goes through LAPACK's QR and differs in its last bits from
    # machine to machine, and with it what LAPACK reaches on a pencil; and the exact case B = I at n = 5)
    for case in [(33, "random", 4, 1, 8, "A"), (5, "random", 0, 2, 4, "A")]:
        assert case in table
        worst = rec["worst"][f"c{case[2]}"]
        for k, v in zip(gen.METRICS, gen.lapack_case(case)):
            assert round(float(v), 3) <= max(worst[k], hd.bounds("hgev", c=case[2])[k] / hd.BOUND_FACTOR), (case, k, v)


def test_the_in_cluster_window_exists():
    """hard_dense.windows is fixed at a width of 16; the generator's windows(33) has its shape at the width the class of 64 serves,
    8, and its fifth window starts and ends inside a cluster of the half_integer spectrum"""
    gen = _generator()
    n = 33
    assert gen.WIDTH == 8 and hd.window_width(n) == 16
    wins = gen.windows(n)
    assert wins[:4] == [(1, 8, "A"), (26, 33, "A"), (1, 1, "A"), (33, 33, "A")] and wins[-1] == (1, n, "N") and len(wins) == 6
    il, iu, mode = wins[4]
    d = hd.half_integer_spectrum(n)
    assert mode == "A" and iu - il + 1 == 8 and 1 < il and iu < n
    assert d[il - 2] == d[il - 1] and d[iu - 1] == d[iu]
    assert gen.windows(5) == [(1, 5, "A"), (2, 4, "A"), (1, 5, "N")]
    assert all(iu - il + 1 <= (16 if k <= 32 else 8) for k in SIZES for il, iu, md in gen.windows(k) if md == "A")


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_windows(gpu_lib, n):
    """every pencil of one size under each of its windows, one call per window, route 1 asserted; E_w, E_r, E_o and E_f (mode
    'N': E_w and E_f) at or under the bound of the pencil's cond group.  Measured worst on an MI355X over both sizes (bound in
    force): see DESIGN section 8q."""
    import test_hgbatch_range as tr
    from test_batch_accuracy import _judge

    gen = _generator()
    table = [c for c in gen.case_table() if c[0] == n]
    pencils = list(dict.fromkeys((c[1], c[2]) for c in table))
    pcs = [hd.pencil("hgev", n, f, c) for f, c in pencils]
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
                    _judge("hgwindow", tag, hd.PENCIL_METRICS, hd.pencil_metrics(pc, w[k], Z[k], U[k], il), bnd)
                else:
                    v = hd.pencil_metrics(pc, w[k], np.zeros((n, m), dtype=np.complex128), U[k], il)
                    _judge("hgwindow", tag, ("E_w", "E_f"), (v[0], v[3]), bnd)
    print(f"BATCH-ACC hgwindow n={n}: {redone} pencils redone by route 2")
