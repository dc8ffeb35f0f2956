"""Hermitian range solves (eigen_h_range / eigen_h_range_v / KMATH_EIGEN_HGEV_RANGE_V, an EXTENSION: LAPACK's range = 'I'
and 'V' for the complex solvers).  The reference is scipy.linalg.eigh on the CPU.  Tolerances and gates are those already
used for eigen_h and KMATH_EIGEN_HGEV_RANGE:
  eigen_h (tests/test_gpu_parity.py::test_eigen_h_reference_driver_checks, ::_herm_check): eigenvalues to
    1e-13 n max|lambda|; ||A Z - Z W||_F / (n eps ||A||_F) < gates.residual, ||Z^H Z - I||_F / (n eps) < gates.orthogonality;
  KMATH_EIGEN_HGEV_RANGE (tests/test_hgev_range.py::_gates): with scale = max(1, max|w_ref|), eigenvalues to 1e-12 scale,
    ||A Z - B Z W||_F < 1e-12 scale n, ||Z^H B Z - I||_F < 1e-12 n, ||U^H U - B||_F < 1e-12 n ||B||_F.
Value bounds are midpoints of gaps of the reference spectrum wider than 1e-8 max|lambda| (asserted where a bound is placed,
as in tests/test_range_v.py), so m and il must equal the reference's exactly.  Wherever an entry promises not to read them,
the strict lower triangle and Im of the diagonal hold NaN.  GPU tests are marked; the CPU tests at the end check the ctypes
table, the export, the wrappers' argument checks and the Fortran module text."""
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
H_INDEX = ["eigx_h_range", "eigx_h_range_dev"]
H_VALUE = ["eigx_h_range_v", "eigx_h_range_v_dev"]
HGEV_VALUE = ["eigx_hgev_range_v", "eigx_hgev_range_v_dev"]
INF = float("inf")
FILL = 7.0
MF, MB = 48, 128      # eigen_h's default panel widths (eigen_NB_f, eigen_NB_b)


def _dev():
    import torch

    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ inputs, computed once
@functools.lru_cache(maxsize=None)
def _matrix(n):
    from eigenexa_amd import layout

    A = layout.random_hermitian(n, seed=100 + n)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def _spectrum(n):
    import scipy.linalg

    w = scipy.linalg.eigh(_matrix(n), eigvals_only=True)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _pencil(n):
    """tests/test_hgev_range.py::_pencil"""
    import scipy.linalg
    from eigenexa_amd import layout

    A, B = layout.random_hermitian(n, seed=3), layout.random_hpd(n)
    A.setflags(write=False)
    B.setflags(write=False)
    w = scipy.linalg.eigh(A, B, eigvals_only=True)
    w.setflags(write=False)
    return A, B, w


@functools.lru_cache(maxsize=None)
def _frank_pencil(n):
    """tests/test_hgev.py::_frank_pencil (unitary Q): A = G M G^H, B = G G^H, the spectrum is Frank's"""
    import scipy.linalg
    from eigenexa_amd import layout

    rng = np.random.default_rng(5)
    s = np.exp(1j * rng.uniform(0, 2 * np.pi, n))
    M = s.conj()[:, None] * layout.frank(n) * s[None, :]
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    G = Q * np.sqrt(rng.uniform(1.0, 10.0, n))[None, :]
    A = G @ M @ G.conj().T
    B = G @ G.conj().T
    A, B = (A + A.conj().T) / 2, (B + B.conj().T) / 2
    w = scipy.linalg.eigh(A, B, eigvals_only=True)
    for x in (A, B, w):
        x.setflags(write=False)
    return A, B, w


def _nan_lower(M):
    """tests/test_hgev_range.py::_nan_lower: the upper triangle of M, NaN strictly below it and in Im of the diagonal"""
    n = M.shape[0]
    out = np.where(np.triu(np.ones((n, n), dtype=bool)), M, np.nan + 1j * np.nan)
    d = np.empty(n, dtype=np.complex128)
    d.real, d.imag = M.real.diagonal(), np.nan
    out[np.diag_indices(n)] = d
    return np.asfortranarray(out)


def _to_dev(M, ld):
    """column-major image of M (rows x cols) with leading dimension ld: tensor (cols, ld), t[j, i] = M(i, j)"""
    import torch

    t = torch.zeros(M.shape[1], ld, dtype=torch.complex128, device=_dev())
    t[:, :M.shape[0]] = torch.from_numpy(np.ascontiguousarray(M.T)).to(_dev())
    return t


def _from_dev(t, rows):
    return t[:, :rows].T.cpu().numpy()


def _mid(wref, k):
    """tests/test_range_v.py::_mid: midpoint of the gap between eigenvalues k and k + 1 (1-based) of the reference"""
    gap = wref[k] - wref[k - 1]
    assert gap > 1e-8 * np.abs(wref).max(), (k, gap)
    return 0.5 * (wref[k - 1] + wref[k])


def _bounds(wref, il, iu):
    """tests/test_range_v.py::_bounds: [vl, vu) holding exactly eigenvalues il .. iu of the reference"""
    n = len(wref)
    if il == 1 and iu == n:
        return -INF, INF
    span = 0.5 * max(wref[-1] - wref[0], np.abs(wref).max())
    vl = wref[0] - span if il == 1 else _mid(wref, il - 1)
    vu = wref[-1] + span if iu == n else _mid(wref, iu)
    return vl, vu


def _windows(n, m):
    """tests/test_range.py::_windows"""
    mid = max(1, (n - m) // 2)
    return [(1, m), (n - m + 1, n), (mid, mid + m - 1), (n // 3 + 1, n // 3 + 1), (1, n)]


def _check_pairs(A, w, Z, wref_window, what):
    """the eigenvalue tolerance and the two gates of eigen_h (see the head of this file) over the m columns"""
    n = A.shape[0]
    m = len(w)
    tol = 1e-13 * n * np.abs(wref_window).max() if m else 0.0
    werr = np.abs(w - wref_window).max()
    anorm = np.linalg.norm(A)
    res = np.linalg.norm(A @ Z - Z * w[None, :]) / (n * EPS * anorm) if anorm > 0 else 0.0
    orth = np.linalg.norm(Z.conj().T @ Z - np.eye(m)) / (n * EPS)
    print(f"  {what}: |w - w_ref| = {werr:.2e} (bound {tol:.2e}), residual {res:.3e}, unitarity {orth:.3e}")
    assert werr <= tol
    assert res < GATE_RES and orth < GATE_ORTH


def _wtol(n, wref):
    return 1e-13 * n * np.abs(wref).max()


def _hgev_gates(A, B, w, Z, wref_window, scale, what):
    """tests/test_hgev_range.py::_gates"""
    n = A.shape[0]
    m = len(w)
    werr = np.abs(w - wref_window).max()
    res = np.linalg.norm(A @ Z - B @ Z * w)
    orth = np.linalg.norm(Z.conj().T @ B @ Z - np.eye(m))
    print(f"  {what}: |w - w_ref| = {werr:.2e} (gate {1e-12 * scale:.2e}), ||AZ - BZW|| = {res:.2e} (gate {1e-12 * scale * n:.2e}), "
          f"||Z^H B Z - I|| = {orth:.2e} (gate {1e-12 * n:.2e})")
    assert werr < 1e-12 * scale
    assert res < 1e-12 * scale * n
    assert orth < 1e-12 * n


@pytest.fixture
def all_sizes(gpu_lib):
    """size rule off (eigx_tune key 17 = 100 %), as in test_range.py"""
    old = gpu_lib.eigx_tune(17, 100)
    yield gpu_lib
    gpu_lib.eigx_tune(17, old)


# keys 17 / 19 that force a path, and the path eigx_range_info then reports
PATHS = {1: (100, None), 3: (0, None), 2: (100, 0)}


@pytest.fixture(params=[1, 3, 2])
def forced_path(gpu_lib, request):
    key17, key19 = PATHS[request.param]
    old17 = gpu_lib.eigx_tune(17, key17)
    old19 = gpu_lib.eigx_tune(19, key19) if key19 is not None else None
    yield gpu_lib, request.param
    gpu_lib.eigx_tune(17, old17)
    if old19 is not None:
        gpu_lib.eigx_tune(19, old19)


def _index_dev(lib, A, il, iu, mode, ld, fn="eigx_h_range_dev", guard=True):
    """the device entry on the NaN-poisoned upper triangle, w and z with one guard entry / column: (rc, w, z, a(1:2,1))"""
    import torch

    n = A.shape[0]
    m = iu - il + 1
    a = _to_dev(_nan_lower(A), ld)
    z = torch.full((m + 1, ld), FILL, dtype=torch.complex128, device=_dev())
    w = torch.full((m + 1,), FILL, dtype=torch.float64, device=_dev())
    rc = getattr(lib, fn)(n, il, iu, a.data_ptr(), ld, w.data_ptr(), z.data_ptr() if mode == b"A" else None, ld, MF, MB, mode)
    return rc, w.cpu().numpy(), _from_dev(z, n), a[0, :2].cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. index windows
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 97, 129, 130, 400])
def test_index_windows_on_every_path(forced_path, n):
    """eigx_h_range_dev, leading dimension n + 1 (odd for even n): the windows [1,1], [n,n], [1,n], an interior one of 10 and
    one of 65 columns, modes 'A' and 'N', with key 17 forcing the subset path (1), key 17 = 0 the full D&C (3), key 19 = 0
    the refusal by the acceptance test (2).  A window of one column cannot be refused (cond(L) of a 1 x 1 factor is 1): it
    stays on path 1.  Eigenvalues against scipy, the two gates over the m columns, guards beyond m untouched"""
    import eigenexa_amd as ee

    lib, path = forced_path
    A, wref = _matrix(n), _spectrum(n)
    wins = {(1, 1), (n, n), (1, n)}
    if n >= 97:
        wins |= {(n // 3, n // 3 + 9), (n // 4, n // 4 + 64)}
    ld = n + 1
    for il, iu in sorted(wins):
        m = iu - il + 1
        for mode in (b"A", b"N"):
            rc, w, z, st = _index_dev(lib, A, il, iu, mode, ld)
            assert rc == 0
            info = ee.range_info()
            assert info.m == m
            assert w[m] == FILL and (z[:, m] == FILL).all()
            assert st[0].real != 0 and st[0].imag == 0 and (n < 2 or (st[1].real > 0 and st[1].imag == 0))   # a(1,1) = flops, a(2,1) = seconds
            if mode == b"N":
                assert (z == FILL).all()
                assert np.abs(w[:m] - wref[il - 1:iu]).max() <= _wtol(n, wref)
                continue
            assert info.path == (path if (m > 1 or path != 2) else 1), (info, path, il, iu)
            _check_pairs(A, w[:m], z[:, :m], wref[il - 1:iu], f"n={n} [{il}, {iu}] path {info.path}")
            assert np.abs(w[:m] - wref[il - 1:iu]).max() <= _wtol(n, wref)


# ------------------------------------------------------------------------------------------------ 2. the full D&C's eigenvalues
@pytest.mark.gpu
@pytest.mark.parametrize("n", [130, 400])
def test_path_3_and_mode_n_eigenvalues_are_those_of_eigen_h(gpu_lib, n):
    """path 3 is the band_dc_dev call of eigx_h_dev(nvec = iu, 'A'): w is bit-identical to w[il-1:iu] of that solve; mode 'N'
    is bit-identical to the same slice of eigx_h_dev(mode 'N')"""
    import torch
    import eigenexa_amd as ee

    A = _matrix(n)
    ld = n + 2
    il, iu = n // 3, n // 3 + 40
    m = iu - il + 1
    full = {}
    for mode in (b"A", b"N"):
        a = _to_dev(_nan_lower(A), ld)
        z = torch.zeros(iu, ld, dtype=torch.complex128, device=_dev())
        w = torch.zeros(n, dtype=torch.float64, device=_dev())
        assert gpu_lib.eigx_h_dev(n, iu, a.data_ptr(), ld, w.data_ptr(), z.data_ptr(), ld, MF, MB, mode) == 0
        full[mode] = w.cpu().numpy()
    old17 = gpu_lib.eigx_tune(17, 0)
    try:
        rc, w, _, _ = _index_dev(gpu_lib, A, il, iu, b"A", ld)
        assert rc == 0 and ee.range_info().path == 3
        assert (w[:m] == full[b"A"][il - 1:iu]).all()
        rc, w, _, _ = _index_dev(gpu_lib, A, il, iu, b"N", ld)
        assert rc == 0
        assert (w[:m] == full[b"N"][il - 1:iu]).all()
    finally:
        gpu_lib.eigx_tune(17, old17)


# ------------------------------------------------------------------------------------------------ 3. value windows
def _solve_v(A, vl, vu, mmax, mode="A", status=0):
    """host form with one guard entry / column beyond mmax; returns ((m, il), w, z, a) with w, z whole"""
    import eigenexa_amd as ee
    from eigenexa_amd import api

    n = A.shape[0]
    a = _nan_lower(A)
    z = np.full((n, mmax + 1), FILL, dtype=np.complex128, order="F")
    w = np.full(mmax + 1, FILL)
    got = ee.eigen_h_range_v(n, vl, vu, a, n, w, z if mode == "A" else None, n, mode=mode, mmax=mmax)
    assert api.last_status() == status
    return got, w, z, a


def _solve_i(A, il, iu, mode="A"):
    import eigenexa_amd as ee
    from eigenexa_amd import api

    n = A.shape[0]
    m = iu - il + 1
    a = _nan_lower(A)
    z = np.zeros((n, m), dtype=np.complex128, order="F")
    w = np.zeros(m)
    ee.eigen_h_range(n, il, iu, a, n, w, z if mode == "A" else None, n, mode=mode)
    assert api.last_status() == 0
    return w, z


def _same_bits(x, y):
    """the same bytes (NaN payloads and signed zeros included)"""
    return x.shape == y.shape and x.dtype == y.dtype and np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [97, 400, 1500])
def test_value_windows_match_index_windows(all_sizes, n):
    """(m, il) exact against scipy; w and z bit-identical to the index call il .. iu; the eigen_h tolerance and gates; the
    guard entry / column beyond m untouched with mmax = m + 1.  n = 1500: three windows of 150, to stay quick"""
    import eigenexa_amd as ee

    A, wref = _matrix(n), _spectrum(n)
    wins = _windows(n, n // 5) if n < 1500 else _windows(n, 150)[:3]
    for il, iu in wins:
        m = iu - il + 1
        vl, vu = _bounds(wref, il, iu)
        got, w, z, a = _solve_v(A, vl, vu, m + 1)
        assert got == (m, il), (got, m, il)
        assert ee.range_info().m == m
        assert w[m] == FILL and (z[:, m] == FILL).all()
        _check_pairs(A, w[:m], z[:, :m], wref[il - 1:iu], f"n={n} [{vl:.4g}, {vu:.4g}) = [{il}, {iu}]")
        assert a[0, 0].real != 0 and a[1, 0].real > 0          # a(1,1) = flops, a(2,1) = seconds
        wi, zi = _solve_i(A, il, iu)
        assert _same_bits(wi, w[:m]) and _same_bits(zi, z[:, :m])


@pytest.mark.gpu
def test_infinite_and_huge_bounds(all_sizes):
    """vl = -Inf, vu = +Inf, both, and bounds at +-1e300, n = 97: the windows scipy's spectrum gives, bit-identical to the
    index calls"""
    n = 97
    A, wref = _matrix(n), _spectrum(n)
    k = 40
    v = _mid(wref, k)
    for vl, vu, il, iu in [(-INF, v, 1, k), (v, INF, k + 1, n), (-INF, INF, 1, n), (-1e300, v, 1, k), (v, 1e300, k + 1, n)]:
        m = iu - il + 1
        got, w, z, _ = _solve_v(A, vl, vu, m + 1)
        assert got == (m, il), (vl, vu, got)
        assert w[m] == FILL and (z[:, m] == FILL).all()
        _check_pairs(A, w[:m], z[:, :m], wref[il - 1:iu], f"[{vl:.4g}, {vu:.4g})")
        wi, zi = _solve_i(A, il, iu)
        assert _same_bits(wi, w[:m]) and _same_bits(zi, z[:, :m])


@pytest.mark.gpu
def test_empty_window_overflow_count_only_and_mode_n(all_sizes):
    import eigenexa_amd as ee
    from eigenexa_amd import api

    n = 400
    A, wref = _matrix(n), _spectrum(n)
    # bounds inside one gap: m = 0, EIGX_OK, w and z untouched, the two statistics written
    k = 123
    g = wref[k] - wref[k - 1]
    assert g > 1e-8 * np.abs(wref).max()
    got, w, z, a = _solve_v(A, wref[k - 1] + 0.25 * g, wref[k - 1] + 0.75 * g, 5)
    assert got == (0, k + 1)
    assert (w == FILL).all() and (z == FILL).all()
    info = ee.range_info()
    assert info.m == 0 and info.path == 0
    assert a[1, 0].real > 0 and _same_bits(a[:, 1:], _nan_lower(A)[:, 1:])
    # the window does not fit: status -9, m and il right, nothing written; the retry by index gives the reference window
    il, iu = 150, 189
    m = iu - il + 1
    vl, vu = _bounds(wref, il, iu)
    got, w, z, a = _solve_v(A, vl, vu, m - 1, status=-9)
    assert got == (m, il)
    assert (w == FILL).all() and (z == FILL).all() and _same_bits(a, _nan_lower(A))
    wi, zi = _solve_i(A, got[1], got[1] + got[0] - 1)
    _check_pairs(A, wi, zi, wref[il - 1:iu], f"retry by index [{il}, {iu}]")
    # count only: w = z = None
    assert ee.eigen_h_range_v(n, vl, vu, _nan_lower(A), n, None, None, n, mode="C") == (m, il)
    assert api.last_status() == 0 and ee.range_info().m == m and ee.range_info().path == 0
    assert ee.eigen_h_range_v(n, -INF, vu, _nan_lower(A), n, None, None, n, mode="C", mmax=0) == (iu, 1)
    assert ee.eigen_h_range_v(n, vl, INF, _nan_lower(A), n, None, None, n, mode="C") == (n - il + 1, il)
    # eigenvalues only, z = None: the index call's, bit for bit
    got, w, z, _ = _solve_v(A, vl, vu, m, mode="N")
    assert got == (m, il) and w[m] == FILL and (z == FILL).all()
    assert np.abs(w[:m] - wref[il - 1:iu]).max() <= _wtol(n, wref)
    wi, _ = _solve_i(A, il, iu, mode="N")
    assert _same_bits(wi, w[:m])


@pytest.mark.gpu
@pytest.mark.parametrize("f", [1e60, 1e-60])
def test_value_window_scaling(all_sizes, f):
    """the matrix times 1e60 / 1e-60 (inside eigen_h's documented overflow limit of about 1e77), the bounds scaled alike"""
    n = 97
    A, wref = _matrix(n), _spectrum(n)
    for il, iu in _windows(n, n // 5):
        m = iu - il + 1
        vl, vu = _bounds(wref, il, iu)
        got, w, z, _ = _solve_v(A * f, vl * f, vu * f, m + 1)
        assert got == (m, il)
        assert w[m] == FILL and (z[:, m] == FILL).all()
        _check_pairs(A, w[:m] / f, z[:, :m], wref[il - 1:iu], f"f={f:g} [{il}, {iu}]")


@pytest.mark.gpu
def test_value_window_device_api(all_sizes):
    """torch tensors on the GPU, odd leading dimension: the Python wrapper (mmax from w and the columns of z) and the C entry
    give the same bits, those of the index entry on the resolved window"""
    import torch
    import eigenexa_amd as ee
    from eigenexa_amd import api

    n = 400
    A, wref = _matrix(n), _spectrum(n)
    il, iu = 301, 380
    m = iu - il + 1
    vl, vu = _bounds(wref, il, iu)
    ld = n + 1
    runs = []
    for rep in range(2):
        a = _to_dev(_nan_lower(A), ld)
        z = torch.full((m + 1, ld), FILL, dtype=torch.complex128, device=_dev())
        w = torch.full((m + 1,), FILL, dtype=torch.float64, device=_dev())
        if rep == 0:
            got = ee.eigen_h_range_v(n, vl, vu, a, ld, w, z, ld)
            assert api.last_status() == 0
        else:
            mm, ii = C.c_int(-1), C.c_int(-1)
            assert all_sizes.eigx_h_range_v_dev(n, vl, vu, m + 1, C.byref(mm), C.byref(ii), a.data_ptr(), ld, w.data_ptr(),
                                                z.data_ptr(), ld, MF, MB, b"A") == 0
            got = (mm.value, ii.value)
        assert got == (m, il)
        runs.append((w.cpu().numpy(), _from_dev(z, n)))
    (w0, z0), (w1, z1) = runs
    assert _same_bits(w0, w1) and _same_bits(z0, z1)
    assert w0[m] == FILL and (z0[:, m] == FILL).all()
    rc, wi, zi, _ = _index_dev(all_sizes, A, il, iu, b"A", ld)
    assert rc == 0 and _same_bits(wi, w0) and _same_bits(zi, z0)
    _check_pairs(A, w0[:m], z0[:, :m], wref[il - 1:iu], f"device [{il}, {iu}]")


# ------------------------------------------------------------------------------------------------ 4. generalised
def _solve_hgev_v(A, B, vl, vu, mmax, mode="A", status=0):
    import eigenexa_amd as ee
    from eigenexa_amd import api

    n = A.shape[0]
    a, b = _nan_lower(A), _nan_lower(B)
    z = np.full((n, mmax + 1), FILL, dtype=np.complex128, order="F")
    w = np.full(mmax + 1, FILL)
    got = ee.KMATH_EIGEN_HGEV_RANGE_V(n, vl, vu, a, n, b, n, w, z if mode == "A" else None, n, mode=mode, mmax=mmax)
    assert api.last_status() == status
    return got, w, z, a, b


def _holds_u(b, B):
    n = B.shape[0]
    U = np.triu(np.nan_to_num(b, nan=0.0))
    return np.linalg.norm(U.conj().T @ U - B) < 1e-12 * n * np.linalg.norm(B)


@pytest.mark.gpu
@pytest.mark.parametrize("n,nb", [(97, "default"), (400, "default"), (400, 64)])
def test_generalised_value_windows(all_sizes, n, nb):
    """KMATH_EIGEN_HGEV_RANGE_V against scipy.linalg.eigh(A, B) with the gates of tests/test_hgev_range.py, on its random
    pencil and on the Frank-spectrum pencil of tests/test_hgev.py; agreement with KMATH_EIGEN_HGEV_RANGE on the resolved
    window to the same eigenvalue tolerance and gates -- NOT bit for bit: the index entry runs eigen_h with nvec = iu, the
    value entry the range solve.  nb = 64: eigx_tune key 20 (once, at n = 400: several panels in the triangular stages)"""
    import eigenexa_amd as ee
    from eigenexa_amd import api

    old20 = all_sizes.eigx_tune(20, 64) if nb == 64 else None
    try:
        for kind, (A, B, wref) in (("random", _pencil(n)), ("frank", _frank_pencil(n))):
            scale = max(1.0, np.abs(wref).max())
            wins = _windows(n, n // 5) if kind == "random" else [(n - n // 5 + 1, n)]
            for il, iu in wins:
                m = iu - il + 1
                vl, vu = _bounds(wref, il, iu)
                got, w, z, _, b = _solve_hgev_v(A, B, vl, vu, m + 1)
                assert got == (m, il)
                assert w[m] == FILL and (z[:, m] == FILL).all()
                _hgev_gates(A, B, w[:m], z[:, :m], wref[il - 1:iu], scale, f"{kind} n={n} [{il}, {iu}]")
                assert _holds_u(b, B)
                a, b = _nan_lower(A), _nan_lower(B)
                zi = np.zeros((n, m), dtype=np.complex128, order="F")
                wi = np.zeros(m)
                ee.KMATH_EIGEN_HGEV_RANGE(n, il, iu, a, n, b, n, wi, zi, n)
                assert api.last_status() == 0
                _hgev_gates(A, B, wi, zi, wref[il - 1:iu], scale, f"{kind} n={n} [{il}, {iu}] by index")
                assert np.abs(wi - w[:m]).max() < 1e-12 * scale
        A, B, wref = _pencil(n)
        scale = max(1.0, np.abs(wref).max())
        # empty window: b still holds U, nothing else is written
        k = n // 2
        g = wref[k] - wref[k - 1]
        assert g > 1e-8 * np.abs(wref).max()
        got, w, z, _, b = _solve_hgev_v(A, B, wref[k - 1] + 0.25 * g, wref[k - 1] + 0.75 * g, 3)
        assert got == (0, k + 1) and (w == FILL).all() and (z == FILL).all()
        assert ee.range_info().m == 0 and ee.range_info().path == 0
        assert _holds_u(b, B)
        # the window does not fit: host arrays as passed
        il, iu = n // 4, n // 4 + 19
        vl, vu = _bounds(wref, il, iu)
        got, w, z, a, b = _solve_hgev_v(A, B, vl, vu, 19, status=-9)
        assert got == (20, il) and (w == FILL).all() and (z == FILL).all()
        assert _same_bits(a, _nan_lower(A)) and _same_bits(b, _nan_lower(B))
        # modes N and C
        got, w, z, _, b = _solve_hgev_v(A, B, vl, vu, 20, mode="N")
        assert got == (20, il) and (z == FILL).all() and w[20] == FILL and _holds_u(b, B)
        assert np.abs(w[:20] - wref[il - 1:iu]).max() < 1e-12 * scale
        assert ee.KMATH_EIGEN_HGEV_RANGE_V(n, vl, vu, _nan_lower(A), n, _nan_lower(B), n, None, None, n, mode="C") == (20, il)
        assert api.last_status() == 0
    finally:
        if old20 is not None:
            all_sizes.eigx_tune(20, old20)


@pytest.mark.gpu
def test_generalised_real_input_and_identity_b(all_sizes):
    """real symmetric input against KMATH_EIGEN_GEV_RANGE_V, and B = I against eigen_h_range_v: the same (m, il), eigenvalues
    to the tolerance of the two solvers, the gates"""
    import scipy.linalg
    import eigenexa_amd as ee
    from eigenexa_amd import api, layout

    n = 97
    Ar, Br = layout.random_symmetric(n, seed=1), layout.random_hpd(n, real=True)
    wref = scipy.linalg.eigh(Ar, Br, eigvals_only=True)
    scale = max(1.0, np.abs(wref).max())
    il, iu = 30, 49
    m = iu - il + 1
    vl, vu = _bounds(wref, il, iu)
    a, b = np.asfortranarray(np.triu(Ar)), np.asfortranarray(np.triu(Br))
    zr = np.zeros((n, m), order="F")
    wr = np.zeros(m)
    assert ee.KMATH_EIGEN_GEV_RANGE_V(n, vl, vu, a, n, b, n, wr, zr, n) == (m, il) and api.last_status() == 0
    Ac, Bc = Ar.astype(np.complex128), Br.astype(np.complex128)
    got, w, z, _, _ = _solve_hgev_v(Ac, Bc, vl, vu, m)
    assert got == (m, il)
    assert np.abs(w[:m] - wr).max() < 1e-12 * scale
    _hgev_gates(Ac, Bc, w[:m], z[:, :m], wref[il - 1:iu], scale, "real input")
    # B = I
    A, wref = _matrix(n), _spectrum(n)
    vl, vu = _bounds(wref, il, iu)
    goth, wh, zh, _ = _solve_v(A, vl, vu, m)
    got, w, z, _, _ = _solve_hgev_v(A, np.eye(n, dtype=np.complex128), vl, vu, m)
    assert got == goth == (m, il)
    assert np.abs(w[:m] - wh[:m]).max() <= _wtol(n, wref)
    _check_pairs(A, w[:m], z[:, :m], wref[il - 1:iu], "B = I")


@pytest.mark.gpu
def test_generalised_statuses_and_device_form(all_sizes):
    """B not positive definite: -7 and *m left alone; bad bounds at the C-ABI: -2, nothing touched; the device form gives the
    host form's answer and leaves U in b"""
    import torch
    import eigenexa_amd as ee
    from eigenexa_amd import api

    n = 97
    A, B, wref = _pencil(n)
    scale = max(1.0, np.abs(wref).max())
    il, iu = 30, 49
    m = iu - il + 1
    vl, vu = _bounds(wref, il, iu)
    got, _, _, _, _ = _solve_hgev_v(A, B - 20.0 * np.eye(n), vl, vu, m, status=-7)
    assert got is None
    a, b = _nan_lower(A), _nan_lower(B - 20.0 * np.eye(n))
    z = np.zeros((n, m), dtype=np.complex128, order="F")
    w = np.zeros(m)
    mm, ii = C.c_int(5), C.c_int(6)
    fn = all_sizes.eigx_hgev_range_v
    assert fn(n, vl, vu, m, C.byref(mm), C.byref(ii), a.ctypes.data, n, b.ctypes.data, n, w.ctypes.data, z.ctypes.data, n, b"A") == -7
    assert (mm.value, ii.value) == (5, 6)
    a, b = _nan_lower(A), _nan_lower(B)

    def call(vl_, vu_, mmax, pm, pi, mode):
        return fn(n, vl_, vu_, mmax, pm, pi, a.ctypes.data, n, b.ctypes.data, n, w.ctypes.data, z.ctypes.data, n, mode)

    assert call(vu, vl, m, C.byref(mm), C.byref(ii), b"A") == -2
    assert call(vl, vl, m, C.byref(mm), C.byref(ii), b"A") == -2
    assert call(float("nan"), vu, m, C.byref(mm), C.byref(ii), b"A") == -2
    assert call(vl, vu, 0, C.byref(mm), C.byref(ii), b"A") == -2
    assert call(vl, vu, m, None, C.byref(ii), b"A") == -2
    assert call(vl, vu, m, C.byref(mm), None, b"A") == -2
    assert call(vl, vu, m, C.byref(mm), C.byref(ii), b"X") == -2
    assert call(vl, vu, m, C.byref(mm), C.byref(ii), b"S") == -2
    assert _same_bits(a, _nan_lower(A)) and _same_bits(b, _nan_lower(B)) and (w == 0).all() and (z == 0).all()
    assert (mm.value, ii.value) == (5, 6)
    goth, wh, zh, _, _ = _solve_hgev_v(A, B, vl, vu, m)
    assert goth == (m, il)
    ld = n + 2
    ad, bd = _to_dev(_nan_lower(A), ld), _to_dev(_nan_lower(B), ld)
    zd = torch.full((m, ld), FILL, dtype=torch.complex128, device=_dev())
    wd = torch.full((m,), FILL, dtype=torch.float64, device=_dev())
    assert ee.KMATH_EIGEN_HGEV_RANGE_V(n, vl, vu, ad, ld, bd, ld, wd, zd, ld) == (m, il)
    assert api.last_status() == 0
    wg, Z = wd.cpu().numpy(), _from_dev(zd, n)
    assert np.abs(wg - wh[:m]).max() < 1e-12 * scale
    _hgev_gates(A, B, wg, Z, wref[il - 1:iu], scale, "device form")
    assert _holds_u(_from_dev(bd, n), B)


# ------------------------------------------------------------------------------------------------ 5. statuses
@pytest.mark.gpu
def test_statuses(gpu_lib):
    """bad il / iu, vl >= vu, a NaN bound, mmax < 1, NULL m / il and the modes 'X' and 'S' are EIGX_ERR_BAD_ARG (-2) at the
    C-ABI and touch nothing; a NaN in the significant triangle is EIGX_ERR_NONFINITE (-5) with w = NaN and m = 0"""
    import eigenexa_amd as ee
    from eigenexa_amd import api

    n = 97
    A = _matrix(n)
    a = _nan_lower(A)
    z = np.zeros((n, 10), dtype=np.complex128, order="F")
    w = np.zeros(10)
    mm, ii = C.c_int(5), C.c_int(6)
    pa, pw, pz = a.ctypes.data, w.ctypes.data, z.ctypes.data
    nan = float("nan")
    fi, fv = gpu_lib.eigx_h_range, gpu_lib.eigx_h_range_v
    for il, iu, mode, za in [(0, 5, b"A", pz), (5, n + 1, b"A", pz), (6, 5, b"A", pz), (1, 5, b"X", pz), (1, 5, b"S", pz),
                             (1, 5, b"C", pz), (1, 5, b"A", None)]:
        assert fi(n, il, iu, pa, n, pw, za, n, MF, MB, mode) == -2
    assert fi(n, 1, 5, pa, n - 1, pw, pz, n, MF, MB, b"A") == -2
    assert fi(n, 1, 5, pa, n, pw, pz, n - 1, MF, MB, b"A") == -2
    assert fi(n, 1, 5, None, n, pw, pz, n, MF, MB, b"A") == -2
    assert fi(n, 1, 5, pa, n, None, pz, n, MF, MB, b"A") == -2
    assert fi(0, 1, 5, pa, n, pw, pz, n, MF, MB, b"A") == -2
    pm, pi = C.byref(mm), C.byref(ii)
    for vl, vu, mmax, qm, qi, mode, za in [(1.0, 0.5, 10, pm, pi, b"A", pz), (0.5, 0.5, 10, pm, pi, b"A", pz),
                                           (nan, 0.5, 10, pm, pi, b"A", pz), (0.0, nan, 10, pm, pi, b"A", pz),
                                           (0.0, 0.5, 0, pm, pi, b"A", pz), (0.0, 0.5, 10, None, pi, b"A", pz),
                                           (0.0, 0.5, 10, pm, None, b"A", pz), (0.0, 0.5, 10, pm, None, b"C", None),
                                           (0.0, 0.5, 10, pm, pi, b"X", pz), (0.0, 0.5, 10, pm, pi, b"S", pz),
                                           (0.0, 0.5, 10, pm, pi, b"A", None)]:
        assert fv(n, vl, vu, mmax, qm, qi, pa, n, pw, za, n, MF, MB, mode) == -2
    assert fv(n, 0.0, 0.5, 10, pm, pi, pa, n - 1, pw, pz, n, MF, MB, b"A") == -2
    assert fv(0, 0.0, 0.5, 10, pm, pi, pa, n, pw, pz, n, MF, MB, b"A") == -2
    assert _same_bits(a, _nan_lower(A)) and (w == 0).all() and (z == 0).all() and (mm.value, ii.value) == (5, 6)
    Bad = np.array(A)
    Bad[3, 7] = np.nan
    a = _nan_lower(Bad)
    w = np.full(9, FILL)
    z = np.full((n, 8), FILL, dtype=np.complex128, order="F")
    ee.eigen_h_range(n, 2, 9, a, n, w, z, n)
    assert api.last_status() == -5
    assert np.isnan(w[:8]).all() and w[8] == FILL and (z == FILL).all()
    w[:] = FILL
    assert ee.eigen_h_range_v(n, -1.0, 1.0, _nan_lower(Bad), n, w, z, n, mmax=8) is None
    assert api.last_status() == -5
    assert np.isnan(w[:8]).all() and w[8] == FILL and (z == FILL).all()
    a = _nan_lower(Bad)
    assert fv(n, -1.0, 1.0, 8, pm, pi, a.ctypes.data, n, w.ctypes.data, z.ctypes.data, n, MF, MB, b"A") == -5
    assert mm.value == 0
    Bad = np.array(A)
    Bad[5, 5] = np.inf         # Re of the diagonal is read
    w[:] = FILL
    ee.eigen_h_range(n, 2, 9, _nan_lower(Bad), n, w, z, n, mode="N")
    assert api.last_status() == -5 and np.isnan(w[:8]).all() and w[8] == FILL


# ------------------------------------------------------------------------------------------------ 6, 7. fresh processes
def _worker(*argv, timeout=300):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "h_range_worker.py"), *argv],
                          capture_output=True, text=True, timeout=timeout)


def _pad_ld(n):
    """csrc/eigx_common.h pad_ld below 2048 doubles: an odd multiple of 32"""
    l = (n + 31) // 32
    assert l * 32 < 2048
    return (l | 1) * 32


@pytest.mark.gpu
def test_subset_path_memory():
    """a process whose only solve is eigen_h_range at n = 1024, m = 32 on the subset path: the pool holds no D&C buffer of
    the outer problem (dc.* below one n x n matrix: what it holds serves the m x m Rayleigh-Ritz problem), and the planes
    h.Zri are sized for m columns: 2 (pad_ld(n + 2) (m + 1) + skew) doubles (h_tridiagonal_stage's formula with zcap = m),
    plus the pool's 1/16 + 256 bytes of slack"""
    n, m = 1024, 32
    r = _worker("memory", str(n), str(m))
    assert r.returncode == 0, r.stdout + r.stderr
    g = re.search(r"MEMORY path=(\d+) dc=(\d+) zri=(\d+) held=(\d+)", r.stdout)
    assert g, r.stdout + r.stderr
    path, dc, zri, held = (int(v) for v in g.groups())
    want = 8 * 2 * (_pad_ld(n + 2) * (m + 1) + 1040)
    print(f"  n={n} m={m}: dc.* {dc} B, h.Zri {zri} B (formula {want} B), held {held} B")
    assert path == 1
    assert dc < n * n * 8
    assert 0 < zri <= want + want // 16 + 256


@pytest.mark.gpu
def test_before_init():
    """a fresh process that never called eigen_init: EIGX_ERR_NOT_INITIALIZED (-1) from all six entries"""
    r = _worker("noinit")
    assert r.returncode == 0 and "OK noinit" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_refuses_several_ranks():
    """two ranks on the one card: all six entries print the refusal and return EIGX_ERR_BAD_ARG on both"""
    import socket

    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = os.path.join(os.path.dirname(__file__), "h_range_worker.py")
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
        assert o.count("one GPU only") >= 6


# ------------------------------------------------------------------------------------------------ 8. Fortran
@pytest.mark.gpu
def test_fortran_caller(gpu_lib, tmp_path):
    """a Fortran program calls eigen_h_range_v and eigen_h_range of module eigen_libs_mod and the external
    KMATH_EIGEN_HGEV_RANGE_V on the Frank spectrum, n = 200; the bounds are mid-gap points of the closed-form spectrum"""
    if not os.path.exists(FLANG):
        pytest.skip("no flang")
    from eigenexa_amd import layout

    n, il, iu = 200, 161, 190
    lam = layout.frank_eigenvalues(n)
    vl, vu = _mid(lam, il - 1), _mid(lam, iu)
    lib = os.path.join(ROOT, "eigenexa_amd", "lib")
    mod = os.path.join(ROOT, "eigenexa_amd", "fortran", "eigen_libs_mod.F90")
    src = os.path.join(ROOT, "tests", "fortran", "h_range_caller.F90")
    subprocess.check_call([FLANG, "-cpp", "-O2", "-c", mod, "-o", "eigen_libs_mod.o"], cwd=tmp_path)
    subprocess.check_call([FLANG, "-cpp", "-O2", "-c", src, "-o", "h_range_caller.o"], cwd=tmp_path)
    subprocess.check_call([FLANG, "-o", "h_range_caller", "h_range_caller.o", "eigen_libs_mod.o", f"-L{lib}",
                           "-leigenexa_amd", f"-Wl,-rpath,{lib}"], cwd=tmp_path)
    out = subprocess.run([str(tmp_path / "h_range_caller"), repr(float(vl)), repr(float(vu))], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    for name in ("eigen_h_range_v", "eigen_h_range", "KMATH_EIGEN_HGEV_RANGE_V"):
        r = re.search(name + r" m =\s*(-?\d+)\s+il =\s*(-?\d+)\s+max rel eigenvalue error =\s*([0-9.eEdD+-]+)", out.stdout)
        assert r, out.stdout
        assert (int(r.group(1)), int(r.group(2))) == (iu - il + 1, il)
        assert float(r.group(3).replace("D", "E").replace("d", "e")) < GOLD["gates"]["frank_rel_err"]
    r = re.search(r"overflow m =\s*(-?\d+)\s+il =\s*(-?\d+)\s+untouched =\s*([TF])", out.stdout)
    assert r and (int(r.group(1)), int(r.group(2)), r.group(3)) == (iu - il + 1, il, "T"), out.stdout


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", H_INDEX + H_VALUE + HGEV_VALUE)
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
    if name in H_INDEX:
        assert names == ["n", "il", "iu", "a", "lda", "w", "z", "ldz", "m_forward", "m_backward", "mode"]
    elif name in H_VALUE:
        assert names == ["n", "vl", "vu", "mmax", "m", "il", "a", "lda", "w", "z", "ldz", "m_forward", "m_backward", "mode"]
    else:
        assert names == ["n", "vl", "vu", "mmax", "m", "il", "a", "lda", "b", "ldb", "w", "z", "ldz", "mode"]


def test_library_exports_the_hermitian_range_entries():
    from eigenexa_amd import _lib

    lib = C.CDLL(_lib.LIB_PATH)
    for name in H_INDEX + H_VALUE + HGEV_VALUE:
        assert hasattr(lib, name), name
    txt = open(os.path.join(ROOT, "include", "eigenexa_amd.h")).read()
    for name in H_INDEX + H_VALUE + HGEV_VALUE:
        head = txt[:txt.index("int " + name + "(")]
        assert "EXTENSION" in head[head.rindex("/*"):] and "8g" in head[head.rindex("/*"):]


def test_python_wrappers_reject_bad_windows_before_the_library(monkeypatch, capsys):
    """bad il / iu, vl >= vu, NaN bounds, a mode outside A / N (/ C), mmax < 1, a missing z with mode A: status -2, one
    warning line and None, without loading the library"""
    import eigenexa_amd as ee
    from eigenexa_amd import _lib, api

    def boom():
        raise AssertionError("the library must not be touched")

    monkeypatch.setattr(_lib, "load", boom)
    a = np.zeros((10, 10), dtype=np.complex128, order="F")
    z = np.zeros((10, 10), dtype=np.complex128, order="F")
    w = np.zeros(10)
    nan = float("nan")
    icases = [(10, 0, 5, z, "A"), (10, 5, 11, z, "A"), (10, 6, 5, z, "A"), (10, 1, 5, z, "X"), (10, 1, 5, z, "S"),
              (10, 1, 5, z, "C"), (10, 1, 5, None, "A"), (0, 1, 1, z, "A"), (10, None, 5, z, "A")]
    for n, il, iu, zz, mode in icases:
        api._state["last_status"] = 0
        assert ee.eigen_h_range(n, il, iu, a, 10, w, zz, 10, mode=mode) is None
        assert api.last_status() == -2
    vcases = [(10, 1.0, 0.5, z, "A", None), (10, 0.5, 0.5, z, "A", None), (10, nan, 1.0, z, "A", None),
              (10, 0.0, nan, z, "A", None), (10, INF, INF, z, "A", None), (10, 0.0, 1.0, z, "X", None),
              (10, 0.0, 1.0, z, "S", None), (10, 0.0, 1.0, None, "A", None), (10, 0.0, 1.0, z, "A", 0), (0, 0.0, 1.0, z, "A", None),
              (10, 1.0, 0.5, None, "C", None)]
    for n, vl, vu, zz, mode, mmax in vcases:
        api._state["last_status"] = 0
        assert ee.eigen_h_range_v(n, vl, vu, a, 10, w, zz, 10, mode=mode, mmax=mmax) is None
        assert api.last_status() == -2
        api._state["last_status"] = 0
        assert ee.KMATH_EIGEN_HGEV_RANGE_V(n, vl, vu, a, 10, a, 10, w, zz, 10, mode=mode, mmax=mmax) is None
        assert api.last_status() == -2
    err = capsys.readouterr().err
    assert err.count("invalid window") == len(icases) + 2 * len(vcases)
    assert {"eigen_h_range", "eigen_h_range_v", "KMATH_EIGEN_HGEV_RANGE_V"} <= set(dir(ee))


def test_fortran_module_binds_the_hermitian_range_entries():
    src = open(os.path.join(ROOT, "eigenexa_amd", "fortran", "eigen_libs_mod.F90")).read()
    for name in ("eigx_h_range", "eigx_h_range_v", "eigx_hgev_range_v"):
        assert f'bind(C, name="{name}")' in src
    assert "public :: eigen_h_range, eigen_h_range_v" in src
    assert re.search(r"^subroutine KMATH_EIGEN_HGEV_RANGE_V\(n, vl, vu, mmax, m, il, a, lda, b, ldb, w, z, ldz, mode\)", src, re.M)
    assert re.search(r"subroutine eigen_h_range\(n, il, iu, a, lda, w, z, ldz, m_forward, m_backward, mode\)", src)
    assert re.search(r"subroutine eigen_h_range_v\(n, vl, vu, mmax, m, il, a, lda, w, z, ldz, m_forward, m_backward, mode\)", src)
