"""The window kernel of eigen_h_batch_range (route key 26 = 1) held to LAPACK-level accuracy on the small hard Hermitian
matrices of tests/hard_dense.py, after test_windows of tests/test_batch_accuracy.py: every family of hard_dense.FAMILIES as
hd.case("h", n, family), the m columns judged column by column and entry by entry against the extended-precision reference.

n = 32, 33 and 64 (both sides of the edge between the n-classes 32 and 64, and the top of the widest class with window storage)
get the windows of hard_dense.windows(n), which are built with MW = 16 there: the lowest and the highest 16, (1, 1), (n, n), 16
in the middle starting and ending inside a cluster of the half_integer family, and (1, n) in mode 'N'.  n = 65 and 96, the class
without window storage, get (1, n, 'N').

Bounds: hd.bounds("h", family=...), 16 x what LAPACK reaches on the h table of tests/golden/batch_accuracy_bounds.json (E_w 172,
E_r 264, E_o 424); none is invented here.  A matrix the acceptance test sends to the redo is judged like any other."""
import numpy as np
import pytest

import hard_dense as hd

SIZES_A = (32, 33, 64)
SIZES_N = (65, 96)


def test_the_in_cluster_window_exists():
    """hard_dense.windows is built with MW = 16 at these sizes, and its fifth window starts and ends inside a cluster of the
    half_integer spectrum: at il = 8, 7 and 24"""
    assert [hd.window_width(n) for n in SIZES_A] == [16, 16, 16]
    assert [hd.windows(n)[4] for n in SIZES_A] == [(8, 23, "A"), (7, 22, "A"), (24, 39, "A")]
    for n in SIZES_A:
        d = hd.half_integer_spectrum(n)
        il, iu, _ = hd.windows(n)[4]
        assert d[il - 2] == d[il - 1] and d[iu - 1] == d[iu]
        assert hd.windows(n)[-1] == (1, n, "N")


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES_A + SIZES_N)
def test_windows(gpu_lib, n):
    import test_hbatch_range as tr
    from test_batch_accuracy import _check_standard

    css = [hd.case("h", n, f) for f in hd.FAMILIES]
    wins = hd.windows(n) if n in SIZES_A else [(1, n, "N")]
    redone = 0
    with tr._Key(gpu_lib, 26, 1):
        for il, iu, mode in wins:
            B = tr.RBatch([cs.A for cs in css], il, iu)
            assert B.run(gpu_lib, mode=mode.encode(), z=mode == "A") == 0
            route, m, rd = tr._range_info(gpu_lib)
            assert route == 1 and m == iu - il + 1
            redone += rd
            w, Z, info = B.results(want_z=mode == "A")
            assert (info == 0).all()
            for k, cs in enumerate(css):
                _check_standard("h", f"{cs.family} n={n} {il}..{iu} {mode}", cs, w[k], Z[k] if mode == "A" else None, il,
                                label="hwindow")
    print(f"BATCH-ACC hwindow n={n}: {redone} matrices redone by route 2")
