"""Value-window eigensolves (eigen_sx_range_v / eigen_s_range_v / KMATH_EIGEN_GEV_RANGE_V, an EXTENSION: LAPACK's
range = 'V') and their stage entry eigx_band_count_dev.  The reference is LAPACK on the CPU: numpy.linalg.eigvalsh and
scipy.linalg.eigh(A, B).  Bounds are midpoints of gaps of the reference spectrum wider than 1e-8 max|lambda| (asserted where
a bound is placed), so a bound is at least 5e-9 max|lambda| from any eigenvalue, far above n eps ||A||, and m and il must
equal the reference's exactly.  GPU tests are marked; the CPU tests at the end check the ctypes table, the export, the
wrappers' argument checks and the Fortran module text."""
import ctypes as C
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from c_header import prototype as _prototype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "known_answers.json")))
GATE_RES = GOLD["gates"]["residual"]
GATE_ORTH = GOLD["gates"]["orthogonality"]
EPS = np.finfo(np.float64).eps
FLANG = os.environ.get("FC", "/opt/rocm/lib/llvm/bin/flang")
SOLVER_SYMBOLS = ["eigx_sx_range_v", "eigx_s_range_v", "eigx_sx_range_v_dev", "eigx_s_range_v_dev"]
GEV_SYMBOLS = ["eigx_gev_range_v", "eigx_gev_range_v_dev"]
SEEDS = {97: 1, 400: 2, 1500: 3}
INF = float("inf")
FILL = 7.0


def _dev():
    import torch

    return torch.device("cuda:0")


def _band_matrix(d, e, band):
    """tests/test_range.py::_band_matrix"""
    n = len(d)
    T = np.diag(d)
    for b in range(1, min(band, n - 1) + 1):
        T += np.diag(e[b - 1, b:n], b) + np.diag(e[b - 1, b:n], -b)
    return T


def _windows(n, m):
    """tests/test_range.py::_windows"""
    mid = max(1, (n - m) // 2)
    return [(1, m), (n - m + 1, n), (mid, mid + m - 1), (n // 3 + 1, n // 3 + 1), (1, n)]


# ------------------------------------------------------------------------------------------------ inputs, computed once
@functools.lru_cache(maxsize=None)
def _matrix(n):
    from eigenexa_amd import layout

    A = layout.random_symmetric(n, seed=SEEDS[n])
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def _spectrum(n):
    w = np.linalg.eigvalsh(_matrix(n))
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _clustered():
    from eigenexa_amd import layout

    A, _ = layout.reference_matrix(333, 6)
    A.setflags(write=False)
    w = np.linalg.eigvalsh(A)
    w.setflags(write=False)
    return A, w


@functools.lru_cache(maxsize=None)
def _pencil(n):
    import scipy.linalg
    from eigenexa_amd import layout

    A, B = _matrix(n), layout.random_hpd(n, real=True)
    B.setflags(write=False)
    w = scipy.linalg.eigh(A, B, eigvals_only=True)
    w.setflags(write=False)
    return A, B, w


@functools.lru_cache(maxsize=None)
def _full_solve(n, route, clustered=False):
    """the library's full solve, shared by the tests that compare a window against its slice"""
    import eigenexa_amd as ee
    from eigenexa_amd import api

    A = _clustered()[0] if clustered else _matrix(n)
    a = np.asfortranarray(np.triu(A))
    z = np.zeros((n, n), order="F")
    w = np.zeros(n)
    (ee.eigen_sx if route == "sx" else ee.eigen_s)(n, n, a, n, w, z, n)
    assert api.last_status() == 0
    w.setflags(write=False)
    return w


def _mid(wref, k):
    """midpoint of the gap between eigenvalues k and k + 1 (1-based) of the reference; the gap is wide enough to count in"""
    gap = wref[k] - wref[k - 1]
    assert gap > 1e-8 * np.abs(wref).max(), (k, gap)
    return 0.5 * (wref[k - 1] + wref[k])


def _bounds(wref, il, iu):
    """[vl, vu) holding exactly eigenvalues il .. iu of the reference: mid-gap points; half the spectrum's width beyond an
    end of the spectrum; the window [1, n] is (-Inf, +Inf)"""
    n = len(wref)
    if il == 1 and iu == n:
        return -INF, INF
    span = 0.5 * max(wref[-1] - wref[0], np.abs(wref).max())
    vl = wref[0] - span if il == 1 else _mid(wref, il - 1)
    vu = wref[-1] + span if iu == n else _mid(wref, iu)
    return vl, vu


@pytest.fixture
def all_sizes(gpu_lib):
    """size rule off (eigx_tune key 17 = 100 %), as in test_range.py"""
    old = gpu_lib.eigx_tune(17, 100)
    yield gpu_lib
    gpu_lib.eigx_tune(17, old)


def _fn(route, index=False):
    import eigenexa_amd as ee

    if index:
        return ee.eigen_sx_range if route == "sx" else ee.eigen_s_range
    return ee.eigen_sx_range_v if route == "sx" else ee.eigen_s_range_v


def _solve_v(A, route, vl, vu, mmax, mode="A", status=0):
    """host form with one guard entry / column beyond mmax; returns ((m, il), w, z, a) with w, z whole"""
    from eigenexa_amd import api

    n = A.shape[0]
    a = np.asfortranarray(np.triu(A))
    z = np.full((n, mmax + 1), FILL, order="F")
    w = np.full(mmax + 1, FILL)
    got = _fn(route)(n, vl, vu, a, n, w, z, n, mode=mode, mmax=mmax)
    assert api.last_status() == status
    return got, w, z, a


def _solve_i(A, route, il, iu):
    from eigenexa_amd import api

    n = A.shape[0]
    m = iu - il + 1
    a = np.asfortranarray(np.triu(A))
    z = np.zeros((n, m), order="F")
    w = np.zeros(m)
    _fn(route, index=True)(n, il, iu, a, n, w, z, n)
    assert api.last_status() == 0
    return w, z


def _check_pairs(A, w, Z, wfull_slice, scale, what):
    from eigenexa_amd import layout

    werr = np.abs(w - wfull_slice).max()
    res, orth = layout.accuracy_metrics(A, w, Z)
    print(f"  {what}: |w - w_full| = {werr:.2e} (bound {1e-12 * scale:.2e}), residual {res:.3e}, orthogonality {orth:.3e}")
    assert werr < 1e-12 * scale
    assert res < GATE_RES and orth < GATE_ORTH


# ------------------------------------------------------------------------------------------------ 1. stage
def _count_points(wref, npts, rng):
    """npts sorted mid-gap points of the reference spectrum (a point below and one above it included)"""
    big = np.abs(wref).max()
    gaps = np.nonzero(np.diff(wref) > 1e-8 * big)[0]
    cand = np.concatenate([[wref[0] - 1e-3 * big], 0.5 * (wref[gaps] + wref[gaps + 1]), [wref[-1] + 1e-3 * big]])
    return np.sort(rng.choice(cand, size=npts, replace=npts > len(cand)))


def _check_counts(lib, n, band, d, e, lde, wref, what):
    import torch

    rng = np.random.default_rng(1000 * n + band)
    for npts in (1, 2, 257, 1000):
        x = _count_points(wref, npts, rng)
        special = {}
        if npts >= 257:   # the specials sit in both workgroups of 257, the last one in its only useful lane
            special = {3: -INF, 64: np.nan, 130: -1e300, 255: 1e300, 256: INF}
        xs = x.copy()
        for k, v in special.items():
            xs[k] = v
        xd = torch.from_numpy(xs).to(_dev())
        cd = torch.full((npts + 1,), -77, dtype=torch.int32, device=_dev())
        assert lib.eigx_band_count_dev(n, d.data_ptr(), e.data_ptr(), lde, band, npts, xd.data_ptr(), cd.data_ptr()) == 0
        c = cd.cpu().numpy()
        assert c[npts] == -77                                   # nothing past npts is written
        want = np.array([-1 if np.isnan(v) else int((wref < v).sum()) for v in xs])
        bad = np.nonzero(c[:npts] != want)[0]
        print(f"  {what} npts={npts}: {len(bad)} counts differ from (w_ref < x).sum()")
        assert len(bad) == 0, (xs[bad][:5], c[:npts][bad][:5], want[bad][:5])
        plain = np.array([k not in special for k in range(npts)])
        assert (np.diff(c[:npts][plain]) >= 0).all()            # non-decreasing over the sorted mid-gap points
    # the specials alone: one workgroup, most lanes idle
    xs = np.array([-INF, wref[0] - 1.0 - abs(wref[0]), 1e300, np.nan, -1e300, INF, wref[-1] + 1.0 + abs(wref[-1])])
    xd = torch.from_numpy(xs).to(_dev())
    cd = torch.zeros(len(xs), dtype=torch.int32, device=_dev())
    assert lib.eigx_band_count_dev(n, d.data_ptr(), e.data_ptr(), lde, band, len(xs), xd.data_ptr(), cd.data_ptr()) == 0
    assert cd.cpu().tolist() == [0, 0, n, -1, 0, n, n]


@pytest.mark.gpu
@pytest.mark.parametrize("band", [1, 2])
@pytest.mark.parametrize("n", [1, 2, 3, 97, 1025, 2049])
def test_band_count_stage(gpu_lib, band, n):
    """eigx_band_count_dev on the band matrix eigx_band_reduce_dev makes of a random matrix: counts at mid-gap points of
    LAPACK's spectrum of the assembled band matrix equal (w_ref < x).sum() exactly; +-Inf, +-1e300 give 0 / n, NaN -1"""
    import torch
    from eigenexa_amd import layout

    A = layout.random_symmetric(n, seed=200 + n + band)
    lda = n + (n & 1)
    a = torch.zeros(n, lda, dtype=torch.float64, device=_dev())
    a[:, :n] = torch.from_numpy(np.ascontiguousarray(A.T)).to(_dev())
    d = torch.zeros(n, dtype=torch.float64, device=_dev())
    e = torch.zeros(2 * n, dtype=torch.float64, device=_dev())
    assert gpu_lib.eigx_band_reduce_dev(n, a.data_ptr(), lda, d.data_ptr(), e.data_ptr(), n, 48, band) == 0
    T = _band_matrix(d.cpu().numpy(), e.cpu().numpy().reshape(2, n), band)
    _check_counts(gpu_lib, n, band, d, e, n, np.linalg.eigvalsh(T), f"band {band} n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("band", [1, 2])
def test_band_count_zero_couplings(gpu_lib, band):
    """a hand-made block-diagonal band matrix, n = 64: 2 x 2 blocks [[c, 1], [1, c]] with c = 10 k and no coupling between
    them (band 2: no second off-diagonal at all).  At x = c both leading diagonal entries of the pentadiagonal window
    vanish exactly (the 2 x 2 block pivot); the eigenvalues are c - 1, c + 1, so x = c is a mid-gap point"""
    import torch
    import eigenexa_amd as ee

    n, lde = 64, 64
    dh = np.repeat(10.0 * np.arange(n // 2), 2)
    eh = np.zeros((2, lde))
    eh[0, 1::2] = 1.0                       # e(i, 1) = T(i - 1, i): inside the blocks only
    T = _band_matrix(dh, eh, band)
    wref = np.linalg.eigvalsh(T)
    assert np.abs(wref - np.sort(np.concatenate([dh[::2] - 1, dh[::2] + 1]))).max() < 1e-12
    d = torch.from_numpy(dh).to(_dev())
    e = torch.from_numpy(eh.reshape(-1).copy()).to(_dev())
    xs = np.sort(np.concatenate([dh[::2], dh[2::2] - 5.0]))      # the block centres and the points between the blocks
    xd = torch.from_numpy(xs).to(_dev())
    cd = torch.zeros(len(xs), dtype=torch.int32, device=_dev())
    assert gpu_lib.eigx_band_count_dev(n, d.data_ptr(), e.data_ptr(), lde, band, len(xs), xd.data_ptr(), cd.data_ptr()) == 0
    c = cd.cpu().numpy()
    assert (c == [(wref < v).sum() for v in xs]).all()
    assert (np.diff(c) >= 0).all()
    assert (ee.band_count(d, e.reshape(2, lde), band, xd).cpu().numpy() == c).all()    # the Python wrapper
    _check_counts(gpu_lib, n, band, d, e, lde, wref, f"block-diagonal band {band}")
    for bad in [(0, lde, band, 3), (n, lde, band, 0), (n, lde, 3, 3), (n, n - 1, band, 3)]:
        assert gpu_lib.eigx_band_count_dev(bad[0], d.data_ptr(), e.data_ptr(), bad[1], bad[2], bad[3], xd.data_ptr(),
                                           cd.data_ptr()) == -2
    assert gpu_lib.eigx_band_count_dev(n, None, e.data_ptr(), lde, band, 3, xd.data_ptr(), cd.data_ptr()) == -2
    assert gpu_lib.eigx_band_count_dev(n, d.data_ptr(), e.data_ptr(), lde, band, 3, xd.data_ptr(), None) == -2


# ------------------------------------------------------------------------------------------------ 2. whole solves
@pytest.mark.gpu
@pytest.mark.parametrize("route", ["sx", "s"])
@pytest.mark.parametrize("n", [97, 400, 1500])
def test_value_windows_match_index_windows(all_sizes, route, n):
    """value windows placed around the index windows of test_range.py: (m, il) exact, w against the slice of the full solve,
    the two gates, the guard entry / column beyond m untouched with mmax = m + 1, and w, z bit-identical to the index call"""
    import eigenexa_amd as ee

    A, wref = _matrix(n), _spectrum(n)
    wf = _full_solve(n, route)
    scale = max(1.0, np.abs(wf).max())
    for il, iu in _windows(n, n // 5):
        m = iu - il + 1
        vl, vu = _bounds(wref, il, iu)
        got, w, z, a = _solve_v(A, route, vl, vu, m + 1)
        assert got == (m, il), (got, m, il)
        assert ee.range_info().m == m
        assert w[m] == FILL and (z[:, m] == FILL).all()
        _check_pairs(A, w[:m], z[:, :m], wf[il - 1:iu], scale, f"{route} n={n} [{vl:.4g}, {vu:.4g}) = [{il}, {iu}]")
        assert np.abs(w[:m] - wref[il - 1:iu]).max() < 1e-12 * scale
        assert a[0, 0] != 0 and a[1, 0] > 0 and a[2, 0] == -1.0   # a(1:3,1) = flops, seconds, -1
        wi, zi = _solve_i(A, route, il, iu)
        assert (wi == w[:m]).all() and (zi == z[:, :m]).all()


# ------------------------------------------------------------------------------------------------ 3. empty, overflow, count
@pytest.mark.gpu
@pytest.mark.parametrize("route", ["sx", "s"])
def test_empty_window_overflow_and_count_only(all_sizes, route):
    import eigenexa_amd as ee
    from eigenexa_amd import api

    n = 400
    A, wref = _matrix(n), _spectrum(n)
    wf = _full_solve(n, route)
    scale = max(1.0, np.abs(wf).max())
    # bounds inside one gap
    k = 123
    assert wref[k] - wref[k - 1] > 1e-8 * np.abs(wref).max()
    g = wref[k] - wref[k - 1]
    got, w, z, a = _solve_v(A, route, wref[k - 1] + 0.25 * g, wref[k - 1] + 0.75 * g, 5)
    assert got == (0, k + 1)
    assert (w == FILL).all() and (z == FILL).all()
    info = ee.range_info()
    assert info.m == 0 and info.path == 0
    assert a[1, 0] > 0 and a[2, 0] == -1.0 and (a[3:, 0] == 0).all() and (a[:, 1:] == np.triu(A)[:, 1:]).all()
    # the window does not fit: status -9, m and il right, nothing written; the retry by index gives the reference window
    il, iu = 150, 189
    m = iu - il + 1
    vl, vu = _bounds(wref, il, iu)
    got, w, z, a = _solve_v(A, route, vl, vu, m - 1, status=-9)
    assert got == (m, il)
    assert (w == FILL).all() and (z == FILL).all() and (a == np.triu(A)).all()
    wi, zi = _solve_i(A, route, got[1], got[1] + got[0] - 1)
    _check_pairs(A, wi, zi, wf[il - 1:iu], scale, f"{route} retry by index [{il}, {iu}]")
    assert np.abs(wi - wref[il - 1:iu]).max() < 1e-12 * scale
    # count only: w = z = None
    a = np.asfortranarray(np.triu(A))
    assert _fn(route)(n, vl, vu, a, n, None, None, n, mode="C") == (m, il)
    assert api.last_status() == 0 and ee.range_info().m == m and ee.range_info().path == 0
    a = np.asfortranarray(np.triu(A))
    assert _fn(route)(n, -INF, vu, a, n, None, None, n, mode="C", mmax=0) == (iu, 1)
    a = np.asfortranarray(np.triu(A))
    assert _fn(route)(n, vl, INF, a, n, None, None, n, mode="C") == (n - il + 1, il)
    # eigenvalues only, z = None
    a = np.asfortranarray(np.triu(A))
    w = np.full(m + 1, FILL)
    assert _fn(route)(n, vl, vu, a, n, w, None, n, mode="N") == (m, il)
    assert api.last_status() == 0 and w[m] == FILL
    assert np.abs(w[:m] - wref[il - 1:iu]).max() < 1e-12 * scale


# ------------------------------------------------------------------------------------------------ 4. every path
@pytest.mark.gpu
@pytest.mark.parametrize("route", ["sx", "s"])
def test_value_window_on_every_path(gpu_lib, route):
    """the type-6 matrix of the reference's benchmark (clusters at 0, 0.2 .. 1.0 of 33, 66, 68, 66, 67, 33): [0.3, 0.7) is
    m = 134 from il = 100, through the subset path, the size rule's full D&C and the forced fallback"""
    import eigenexa_amd as ee

    n = 333
    A, wref = _clustered()
    assert ((wref >= 0.3) & (wref < 0.7)).sum() == 134 and (wref < 0.3).sum() == 99
    wf = _full_solve(n, route, clustered=True)
    scale = max(1.0, np.abs(wf).max())
    old17 = gpu_lib.eigx_tune(17, 100)
    old19 = gpu_lib.eigx_tune(19, 6)
    try:
        for key17, key19, path in [(100, 6, 1), (5, 6, 3), (100, 0, 2)]:
            gpu_lib.eigx_tune(17, key17)
            gpu_lib.eigx_tune(19, key19)
            got, w, z, _ = _solve_v(A, route, 0.3, 0.7, 140)
            info = ee.range_info()
            print(f"  keys 17 / 19 = {key17} / {key19}: path {info.path}, cond(L) {info.cond:.3g}")
            assert got == (134, 100)
            assert info.path == path and info.m == 134
            assert (w[134:] == FILL).all() and (z[:, 134:] == FILL).all()
            _check_pairs(A, w[:134], z[:, :134], wf[99:233], scale, f"{route} path {path}")
    finally:
        gpu_lib.eigx_tune(17, old17)
        gpu_lib.eigx_tune(19, old19)


# ------------------------------------------------------------------------------------------------ 5. end point on a cluster
@pytest.mark.gpu
@pytest.mark.parametrize("route", ["sx", "s"])
def test_end_point_on_a_cluster(all_sizes, route):
    """vl = 0.4 exactly, on the 68-fold cluster: the count may cut the cluster anywhere"""
    n = 333
    A, wref = _clustered()
    wf = _full_solve(n, route, clustered=True)
    scale = max(1.0, np.abs(wf).max())
    tol = 1e-12 * scale
    vl, vu = 0.4, 0.7
    got, w, z, _ = _solve_v(A, route, vl, vu, 140)
    m, il = got
    print(f"  {route}: m = {m}, il = {il}")
    assert 99 <= il - 1 <= 167
    assert il + m - 1 == 233
    _check_pairs(A, w[:m], z[:, :m], wf[il - 1:il - 1 + m], scale, f"{route} [0.4, 0.7)")
    inside = wref[(wref >= vl + tol) & (wref < vu - tol)]          # further than tol inside: all returned
    assert all(np.abs(w[:m] - v).min() <= tol for v in np.unique(inside))
    assert ((wref >= vl + tol) & (wref < vu - tol)).sum() <= m <= ((wref >= vl - tol) & (wref < vu + tol)).sum()
    assert (w[:m] >= vl - tol).all() and (w[:m] < vu + tol).all()   # none further than tol outside
    assert (w[m:] == FILL).all() and (z[:, m:] == FILL).all()


# ------------------------------------------------------------------------------------------------ 6. scaling
@pytest.mark.gpu
@pytest.mark.parametrize("route", ["sx", "s"])
@pytest.mark.parametrize("f", [1e120, 1e-120])
def test_value_window_scaling(all_sizes, route, f):
    """the matrix times 1e120 / 1e-120 (outside [1e-90, 1e90]: rescaled inside), the bounds scaled alike"""
    from eigenexa_amd import layout

    n = 97
    A, wref = _matrix(n), _spectrum(n)
    scale = max(1.0, np.abs(wref).max())
    for il, iu in _windows(n, n // 5):
        m = iu - il + 1
        vl, vu = _bounds(wref, il, iu)
        got, w, z, _ = _solve_v(A * f, route, vl * f, vu * f, m + 1)
        assert got == (m, il)
        assert np.abs(w[:m] / f - wref[il - 1:iu]).max() < 1e-12 * scale
        res, orth = layout.accuracy_metrics(A, w[:m] / f, z[:, :m])
        assert res < GATE_RES and orth < GATE_ORTH
        assert w[m] == FILL and (z[:, m] == FILL).all()


# ------------------------------------------------------------------------------------------------ 7. device API
def _to_dev(M, ld):
    """column-major image of M with leading dimension ld: tensor (cols, ld), t[j, i] = M(i, j)"""
    import torch

    t = torch.zeros(M.shape[1], ld, dtype=torch.float64, device=_dev())
    t[:, :M.shape[0]] = torch.from_numpy(np.ascontiguousarray(M.T)).to(_dev())
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["sx", "s"])
@pytest.mark.parametrize("odd", [False, True])
def test_value_window_device_api(all_sizes, route, odd):
    """torch tensors on the GPU, even and odd lda: the answers of the host form, and a bit-identical repeat"""
    import torch
    from eigenexa_amd import api, layout

    n = 400
    A, wref = _matrix(n), _spectrum(n)
    il, iu = 301, 380
    m = iu - il + 1
    vl, vu = _bounds(wref, il, iu)
    goth, wh, zh, _ = _solve_v(A, route, vl, vu, m + 1)
    assert goth == (m, il)
    lda = n + 1 if odd else n + 2
    runs = []
    for rep in range(2):
        a = _to_dev(np.triu(A), lda)
        z = torch.full((m + 1, lda), FILL, dtype=torch.float64, device=_dev())
        w = torch.full((m + 1,), FILL, dtype=torch.float64, device=_dev())
        if rep == 0:
            got = _fn(route)(n, vl, vu, a, lda, w, z, lda)       # mmax from w and the columns of z
            assert api.last_status() == 0
        else:
            fn = all_sizes.eigx_sx_range_v_dev if route == "sx" else all_sizes.eigx_s_range_v_dev
            mm, ii = C.c_int(-1), C.c_int(-1)
            assert fn(n, vl, vu, m + 1, C.byref(mm), C.byref(ii), a.data_ptr(), lda, w.data_ptr(), z.data_ptr(), lda, 48, 128,
                      b"A") == 0
            got = (mm.value, ii.value)
        assert got == (m, il)
        runs.append((w.cpu().numpy(), z[:, :n].T.cpu().numpy()))
        st = a[0, :3].cpu().numpy()
        assert st[1] > 0 and st[2] == -1.0
    (w0, z0), (w1, z1) = runs
    assert (w0 == w1).all() and (z0 == z1).all()
    assert w0[m] == FILL and (z0[:, m] == FILL).all()
    # the host form stages the matrix with a leading dimension of its own: the same answers to the tolerance of the solves
    scale = max(1.0, np.abs(wref).max())
    assert np.abs(w0[:m] - wh[:m]).max() < 1e-12 * scale and np.abs(w0[:m] - wref[il - 1:iu]).max() < 1e-12 * scale
    res, orth = layout.accuracy_metrics(A, w0[:m], z0[:, :m])
    assert res < GATE_RES and orth < GATE_ORTH


# ------------------------------------------------------------------------------------------------ 8. generalised
def _solve_gev_v(A, B, vl, vu, mmax, mode="A", status=0):
    import eigenexa_amd as ee
    from eigenexa_amd import api

    n = A.shape[0]
    a = np.asfortranarray(np.triu(A))
    b = np.asfortranarray(np.triu(B))
    z = np.full((n, mmax + 1), FILL, order="F")
    w = np.full(mmax + 1, FILL)
    got = ee.KMATH_EIGEN_GEV_RANGE_V(n, vl, vu, a, n, b, n, w, z, n, mode=mode, mmax=mmax)
    assert api.last_status() == status
    return got, w, z, a, b


@pytest.mark.gpu
@pytest.mark.parametrize("nb", ["default", 64])
@pytest.mark.parametrize("n", [97, 400])
def test_generalised_value_windows(all_sizes, n, nb):
    """KMATH_EIGEN_GEV_RANGE_V against scipy.linalg.eigh(A, B) at the tolerances of tests/test_gev_range.py (scale =
    max(1, max|w_ref|): eigenvalues to 1e-12 scale, ||A Z - B Z W||_F < 1e-12 scale n, ||Z^T B Z - I||_F < 1e-12 n);
    nb = 64: eigx_tune key 20, several panels in the triangular stages"""
    import eigenexa_amd as ee

    A, B, wref = _pencil(n)
    scale = max(1.0, np.abs(wref).max())
    old20 = all_sizes.eigx_tune(20, 64) if nb == 64 else None
    try:
        for il, iu in _windows(n, n // 5):
            m = iu - il + 1
            vl, vu = _bounds(wref, il, iu)
            got, w, z, _, b = _solve_gev_v(A, B, vl, vu, m + 1)
            assert got == (m, il)
            assert w[m] == FILL and (z[:, m] == FILL).all()
            Z = z[:, :m]
            werr = np.abs(w[:m] - wref[il - 1:iu]).max()
            res = np.linalg.norm(A @ Z - B @ Z * w[:m])
            orth = np.linalg.norm(Z.T @ B @ Z - np.eye(m))
            print(f"  n={n} [{il}, {iu}]: |w - w_ref| = {werr:.2e}, ||AZ - BZW|| = {res:.2e}, ||Z^T B Z - I|| = {orth:.2e}")
            assert werr < 1e-12 * scale and res < 1e-12 * scale * n and orth < 1e-12 * n
            U = np.triu(b)
            assert np.linalg.norm(U.T @ U - B) < 1e-12 * n * np.linalg.norm(B)   # b holds U with B = U^T U
        # empty window: b still holds U, nothing else is written
        k = n // 2
        g = wref[k] - wref[k - 1]
        assert g > 1e-8 * np.abs(wref).max()
        got, w, z, _, b = _solve_gev_v(A, B, wref[k - 1] + 0.25 * g, wref[k - 1] + 0.75 * g, 3)
        assert got == (0, k + 1) and (w == FILL).all() and (z == FILL).all()
        assert ee.range_info().m == 0 and ee.range_info().path == 0
        U = np.triu(b)
        assert np.linalg.norm(U.T @ U - B) < 1e-12 * n * np.linalg.norm(B)
        # the window does not fit
        il, iu = n // 4, n // 4 + 19
        vl, vu = _bounds(wref, il, iu)
        got, w, z, a, b = _solve_gev_v(A, B, vl, vu, 19, status=-9)
        assert got == (20, il) and (w == FILL).all() and (z == FILL).all()
        assert (a == np.triu(A)).all() and (b == np.triu(B)).all()   # host arrays as passed: ready for the retry by index
        # modes N and C
        got, w, z, _, _ = _solve_gev_v(A, B, vl, vu, 20, mode="N")
        assert got == (20, il) and (z == FILL).all() and w[20] == FILL
        assert np.abs(w[:20] - wref[il - 1:iu]).max() < 1e-12 * scale
        a = np.asfortranarray(np.triu(A))
        b = np.asfortranarray(np.triu(B))
        assert ee.KMATH_EIGEN_GEV_RANGE_V(n, vl, vu, a, n, b, n, None, None, n, mode="C") == (20, il)
    finally:
        if old20 is not None:
            all_sizes.eigx_tune(20, old20)


@pytest.mark.gpu
def test_generalised_statuses_and_device_form(all_sizes):
    """B not positive definite: -7; bad bounds at the C-ABI: -2; the device form gives the host form's answer"""
    import torch
    import eigenexa_amd as ee
    from eigenexa_amd import api

    n = 97
    A, B, wref = _pencil(n)
    il, iu = 30, 49
    m = iu - il + 1
    vl, vu = _bounds(wref, il, iu)
    got, _, _, _, _ = _solve_gev_v(A, B - 20.0 * np.eye(n), vl, vu, m, status=-7)
    assert got is None
    a = np.asfortranarray(np.triu(A))
    b = np.asfortranarray(np.triu(B))
    z = np.zeros((n, m), order="F")
    w = np.zeros(m)
    mm, ii = C.c_int(), C.c_int()
    fn = all_sizes.eigx_gev_range_v

    def call(vl_, vu_, mmax, pm, pi, mode):
        return fn(n, vl_, vu_, mmax, pm, pi, a.ctypes.data, n, b.ctypes.data, n, w.ctypes.data, z.ctypes.data, n, mode)

    assert call(vu, vl, m, C.byref(mm), C.byref(ii), b"A") == -2
    assert call(vl, vl, m, C.byref(mm), C.byref(ii), b"A") == -2
    assert call(float("nan"), vu, m, C.byref(mm), C.byref(ii), b"A") == -2
    assert call(vl, vu, 0, C.byref(mm), C.byref(ii), b"A") == -2
    assert call(vl, vu, m, None, C.byref(ii), b"A") == -2
    assert call(vl, vu, m, C.byref(mm), None, b"A") == -2
    assert call(vl, vu, m, C.byref(mm), C.byref(ii), b"X") == -2
    assert (a == np.triu(A)).all() and (b == np.triu(B)).all()
    goth, wh, zh, _, _ = _solve_gev_v(A, B, vl, vu, m)
    assert goth == (m, il)
    ld = n + 1   # 98: the device form asks for even leading dimensions
    ad, bd = _to_dev(np.triu(A), ld), _to_dev(np.triu(B), ld)
    zd = torch.full((m, ld), FILL, dtype=torch.float64, device=_dev())
    wd = torch.full((m,), FILL, dtype=torch.float64, device=_dev())
    assert ee.KMATH_EIGEN_GEV_RANGE_V(n, vl, vu, ad, ld, bd, ld, wd, zd, ld) == (m, il)
    assert api.last_status() == 0
    scale = max(1.0, np.abs(wref).max())
    wg, Z = wd.cpu().numpy(), zd[:, :n].T.cpu().numpy()
    assert np.abs(wg - wh[:m]).max() < 1e-12 * scale and np.abs(wg - wref[il - 1:iu]).max() < 1e-12 * scale
    assert np.linalg.norm(A @ Z - B @ Z * wg) < 1e-12 * scale * n and np.linalg.norm(Z.T @ B @ Z - np.eye(m)) < 1e-12 * n
    U = np.triu(bd[:, :n].T.cpu().numpy())
    assert np.linalg.norm(U.T @ U - B) < 1e-12 * n * np.linalg.norm(B)


# ------------------------------------------------------------------------------------------------ 9. statuses
@pytest.mark.gpu
def test_value_window_statuses(gpu_lib):
    """vl >= vu, a NaN bound, mmax = 0, NULL m / il and mode 'X' are EIGX_ERR_BAD_ARG (-2) at the C-ABI and touch nothing; a
    NaN in the upper triangle is EIGX_ERR_NONFINITE (-5) with w(1:mmax) = NaN and m = 0"""
    from eigenexa_amd import api

    n = 97
    A = _matrix(n)
    a = np.asfortranarray(np.triu(A))
    z = np.zeros((n, 10), order="F")
    w = np.zeros(10)
    mm, ii = C.c_int(), C.c_int()
    pa, pw, pz = a.ctypes.data, w.ctypes.data, z.ctypes.data
    nan = float("nan")
    for fn in (gpu_lib.eigx_sx_range_v, gpu_lib.eigx_s_range_v):
        assert fn(n, 1.0, 0.5, 10, C.byref(mm), C.byref(ii), pa, n, pw, pz, n, 48, 128, b"A") == -2
        assert fn(n, 0.5, 0.5, 10, C.byref(mm), C.byref(ii), pa, n, pw, pz, n, 48, 128, b"A") == -2
        assert fn(n, nan, 0.5, 10, C.byref(mm), C.byref(ii), pa, n, pw, pz, n, 48, 128, b"A") == -2
        assert fn(n, 0.0, nan, 10, C.byref(mm), C.byref(ii), pa, n, pw, pz, n, 48, 128, b"A") == -2
        assert fn(n, 0.0, 0.5, 0, C.byref(mm), C.byref(ii), pa, n, pw, pz, n, 48, 128, b"A") == -2
        assert fn(n, 0.0, 0.5, 10, None, C.byref(ii), pa, n, pw, pz, n, 48, 128, b"A") == -2
        assert fn(n, 0.0, 0.5, 10, C.byref(mm), None, pa, n, pw, pz, n, 48, 128, b"A") == -2
        assert fn(n, 0.0, 0.5, 10, C.byref(mm), None, pa, n, None, None, n, 48, 128, b"C") == -2
        assert fn(n, 0.0, 0.5, 10, C.byref(mm), C.byref(ii), pa, n, pw, pz, n, 48, 128, b"X") == -2
        assert fn(n, 0.0, 0.5, 10, C.byref(mm), C.byref(ii), pa, n, pw, None, n, 48, 128, b"A") == -2
        assert fn(n, 0.0, 0.5, 10, C.byref(mm), C.byref(ii), pa, n - 1, pw, pz, n, 48, 128, b"A") == -2
        assert fn(0, 0.0, 0.5, 10, C.byref(mm), C.byref(ii), pa, n, pw, pz, n, 48, 128, b"A") == -2
    assert (a == np.triu(A)).all() and (w == 0).all() and (z == 0).all()
    Bad = np.array(A)
    Bad[3, 7] = np.nan
    Bad[20, 11] = np.inf        # lower triangle: never read
    for route in ("sx", "s"):
        a = np.asfortranarray(Bad.copy())
        w = np.full(9, FILL)
        z = np.full((n, 8), FILL, order="F")
        got = _fn(route)(n, -1.0, 1.0, a, n, w, z, n, mmax=8)
        assert api.last_status() == -5 and got is None
        assert np.isnan(w[:8]).all() and w[8] == FILL and (z == FILL).all()
        mm = C.c_int(5)
        fn = gpu_lib.eigx_sx_range_v if route == "sx" else gpu_lib.eigx_s_range_v
        a = np.asfortranarray(Bad.copy())
        assert fn(n, -1.0, 1.0, 8, C.byref(mm), C.byref(ii), a.ctypes.data, n, w.ctypes.data, z.ctypes.data, n, 48, 128,
                  b"A") == -5
        assert mm.value == 0


@pytest.mark.gpu
def test_value_window_before_init():
    """a fresh process that never called eigen_init: EIGX_ERR_NOT_INITIALIZED (-1) from every value-window entry"""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "range_v_worker.py"), "noinit"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK noinit" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_value_window_refuses_several_ranks():
    """two ranks on the one card: the value-window entries print the refusal and return EIGX_ERR_BAD_ARG on both"""
    import socket

    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = os.path.join(os.path.dirname(__file__), "range_v_worker.py")
    env = dict(os.environ)
    env.setdefault("EIGX_SELFTEST_ROUNDS", "40")
    procs = [subprocess.Popen([sys.executable, script, "ranks", str(r), "2", str(port)], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True, env=env) for r in range(2)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=300)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"OK rank {r}/2" in o, o[-3000:]
        assert "one GPU only" in o


# ------------------------------------------------------------------------------------------------ 10. Fortran
@pytest.mark.gpu
def test_fortran_value_window_caller(gpu_lib, tmp_path):
    """a Fortran program calls eigen_sx_range_v of module eigen_libs_mod and the external KMATH_EIGEN_GEV_RANGE_V on Frank
    n = 200 (the pencil of tests/fortran/gev_range_caller.F90); the bounds are mid-gap points of the closed-form spectrum"""
    if not os.path.exists(FLANG):
        pytest.skip("no flang")
    from eigenexa_amd import layout

    n, il, iu = 200, 161, 190
    lam = layout.frank_eigenvalues(n)
    vl, vu = _mid(lam, il - 1), _mid(lam, iu)
    lib = os.path.join(ROOT, "eigenexa_amd", "lib")
    mod = os.path.join(ROOT, "eigenexa_amd", "fortran", "eigen_libs_mod.F90")
    src = os.path.join(ROOT, "tests", "fortran", "range_v_caller.F90")
    subprocess.check_call([FLANG, "-cpp", "-O2", "-c", mod, "-o", "eigen_libs_mod.o"], cwd=tmp_path)
    subprocess.check_call([FLANG, "-cpp", "-O2", "-c", src, "-o", "range_v_caller.o"], cwd=tmp_path)
    subprocess.check_call([FLANG, "-o", "range_v_caller", "range_v_caller.o", "eigen_libs_mod.o", f"-L{lib}",
                           "-leigenexa_amd", f"-Wl,-rpath,{lib}"], cwd=tmp_path)
    out = subprocess.run([str(tmp_path / "range_v_caller"), repr(float(vl)), repr(float(vu))], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    for name in ("eigen_sx_range_v", "KMATH_EIGEN_GEV_RANGE_V"):
        r = re.search(name + r" m =\s*(-?\d+)\s+il =\s*(-?\d+)\s+max rel eigenvalue error =\s*([0-9.eEdD+-]+)", out.stdout)
        assert r, out.stdout
        assert (int(r.group(1)), int(r.group(2))) == (iu - il + 1, il)
        assert float(r.group(3).replace("D", "E").replace("d", "e")) < GOLD["gates"]["frank_rel_err"]
    r = re.search(r"overflow m =\s*(-?\d+)\s+il =\s*(-?\d+)\s+untouched =\s*([TF])", out.stdout)
    assert r and (int(r.group(1)), int(r.group(2)), r.group(3)) == (iu - il + 1, il, "T"), out.stdout


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", SOLVER_SYMBOLS + GEV_SYMBOLS + ["eigx_band_count_dev"])
def test_header_prototypes_match_the_ctypes_table(name):
    from eigenexa_amd import _lib

    params = _prototype(name)
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is C.c_int and len(argtypes) == len(params)
    for p, t in zip(params, argtypes):
        if p.startswith("char "):
            assert t is C.c_char
        elif p.startswith("double ") and "*" not in p:
            assert t is C.c_double
        elif p in ("int* m", "int* il"):
            assert t == C.POINTER(C.c_int)
        elif "*" in p:
            assert t is C.c_void_p
        else:
            assert p.startswith("int ") and t is C.c_int
    names = [p.split()[-1].replace("_dev", "") for p in params]
    if name in SOLVER_SYMBOLS:
        assert names == ["n", "vl", "vu", "mmax", "m", "il", "a", "lda", "w", "z", "ldz", "m_forward", "m_backward", "mode"]
    elif name in GEV_SYMBOLS:
        assert names == ["n", "vl", "vu", "mmax", "m", "il", "a", "lda", "b", "ldb", "w", "z", "ldz", "mode"]
    else:
        assert names == ["n", "d", "e", "lde", "band", "npts", "x", "cnt"]


def test_library_exports_the_value_window_entries():
    from eigenexa_amd import _lib

    lib = C.CDLL(_lib.LIB_PATH)
    for name in SOLVER_SYMBOLS + GEV_SYMBOLS + ["eigx_band_count_dev"]:
        assert hasattr(lib, name), name
    txt = open(os.path.join(ROOT, "include", "eigenexa_amd.h")).read()
    assert re.search(r"#define\s+EIGX_ERR_WINDOW\s+\(-9\)", txt)


def test_python_wrappers_reject_bad_value_windows_before_the_library(monkeypatch, capsys):
    """vl >= vu, NaN bounds, a mode outside A / N / C, mmax < 1, a missing z with mode A: status -2, one warning line and
    None, without loading the library"""
    import eigenexa_amd as ee
    from eigenexa_amd import _lib, api

    def boom():
        raise AssertionError("the library must not be touched")

    monkeypatch.setattr(_lib, "load", boom)
    a = np.zeros((10, 10), order="F")
    z = np.zeros((10, 10), order="F")
    w = np.zeros(10)
    nan = float("nan")
    cases = [(10, 1.0, 0.5, z, "A", None), (10, 0.5, 0.5, z, "A", None), (10, nan, 1.0, z, "A", None),
             (10, 0.0, nan, z, "A", None), (10, INF, INF, z, "A", None), (10, 0.0, 1.0, z, "X", None),
             (10, 0.0, 1.0, z, "S", None), (10, 0.0, 1.0, None, "A", None), (10, 0.0, 1.0, z, "A", 0), (0, 0.0, 1.0, z, "A", None),
             (10, 1.0, 0.5, None, "C", None)]
    for fn in (ee.eigen_sx_range_v, ee.eigen_s_range_v):
        for n, vl, vu, zz, mode, mmax in cases:
            api._state["last_status"] = 0
            assert fn(n, vl, vu, a, 10, w, zz, 10, mode=mode, mmax=mmax) is None
            assert api.last_status() == -2
    for n, vl, vu, zz, mode, mmax in cases:
        api._state["last_status"] = 0
        assert ee.KMATH_EIGEN_GEV_RANGE_V(n, vl, vu, a, 10, a, 10, w, zz, 10, mode=mode, mmax=mmax) is None
        assert api.last_status() == -2
    err = capsys.readouterr().err
    assert err.count("invalid window") == 3 * len(cases)
    assert {"eigen_sx_range_v", "eigen_s_range_v", "KMATH_EIGEN_GEV_RANGE_V", "band_count"} <= set(dir(ee))


def test_fortran_module_binds_the_value_window_entries():
    src = open(os.path.join(ROOT, "eigenexa_amd", "fortran", "eigen_libs_mod.F90")).read()
    for name in ("eigx_sx_range_v", "eigx_s_range_v", "eigx_gev_range_v"):
        assert f'bind(C, name="{name}")' in src
    assert "public :: eigen_sx_range_v, eigen_s_range_v" in src
    assert re.search(r"^subroutine KMATH_EIGEN_GEV_RANGE_V\(n, vl, vu, mmax, m, il, a, lda, b, ldb, w, z, ldz, mode\)", src, re.M)
    for name in ("eigen_sx_range_v", "eigen_s_range_v"):
        assert re.search(r"subroutine " + name + r"\(n, vl, vu, mmax, m, il, a, lda, w, z, ldz, m_forward, m_backward, mode\)", src)
