"""KMATH_EIGEN_HGEV_RANGE (an EXTENSION: the reference has no complex, Cholesky-route or index-range generalised solver):
blocked Hermitian Cholesky B = U^H U, complex triangular solves by block inversion, C = U^-H A U^-1, eigen_h of C,
Z = U^-1 Y.  Matrices and tolerances are those of tests/test_gev_range.py and tests/test_hgev.py: with
scale = max(1, max|w_ref|), eigenvalues to 1e-12 scale, ||A Z - B Z W||_F < 1e-12 scale n, ||Z^H B Z - I||_F < 1e-12 n,
||U^H U - B||_F < 1e-12 n ||B||_F, max|U - U_ref| < 1e-12 n max|U_ref|, solves ||op(U) X - R||_F < 1e-12 n ||U|| ||X||,
reduction ||U^H C U - A||_F < 1e-12 n ||A||_F.  GPU tests are marked; the CPU tests at the end check the ctypes table, the
export and the wrapper's argument checks."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from c_header import prototype as _prototype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLANG = os.environ.get("FC", "/opt/rocm/lib/llvm/bin/flang")
HGEVR_SYMBOLS = ["eigx_hgev_range", "eigx_hgev_range_dev", "eigx_zchol_dev", "eigx_ztrsm_upper_dev", "eigx_hgev_reduce_dev"]
STAGE_N = [1, 2, 5, 63, 64, 65, 130, 517, 1100]
NB_KEYS = [64, 128, "default"]


def _dev():
    import torch

    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ inputs, computed once
@functools.lru_cache(maxsize=None)
def _pencil(n, kind="hpd"):
    """A = random_hermitian(n, seed=3); B = random_hpd(n) (spectrum in [1, 10]), or Q diag(logspace(0, -4, n)) Q^H with a
    seeded unitary Q (cond 1e4).  Read-only."""
    from eigenexa_amd import layout

    A = layout.random_hermitian(n, seed=3)
    if kind == "hpd":
        B = layout.random_hpd(n)
    else:
        rng = np.random.default_rng(11)
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
        B = (Q * np.logspace(0, -4, n)) @ Q.conj().T
        B = (B + B.conj().T) / 2
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


@functools.lru_cache(maxsize=None)
def _reference(n, kind="hpd"):
    import scipy.linalg

    A, B = _pencil(n, kind)
    w = scipy.linalg.eigh(A, B, eigvals_only=True)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _factor(n):
    U = np.linalg.cholesky(_pencil(n)[1]).conj().T.copy()
    U.setflags(write=False)
    return U


def _nan_lower(M):
    """the upper triangle of M, NaN strictly below it and in Im of the diagonal (neither may matter)"""
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


@pytest.fixture(params=NB_KEYS)
def tri_nb(gpu_lib, request):
    """eigx_tune key 20 (outer block width of the triangular stages) at 64, 128 and its default"""
    if request.param == "default":
        yield gpu_lib
        return
    old = gpu_lib.eigx_tune(20, request.param)
    assert old >= 64
    yield gpu_lib
    gpu_lib.eigx_tune(20, old)


def _windows(n, m):
    """the windows of tests/test_gev_range.py::_windows"""
    mid = max(1, (n - m) // 2)
    return [(1, m), (n - m + 1, n), (mid, mid + m - 1), (n // 3 + 1, n // 3 + 1), (1, n)]


def _gates(A, B, w, Z, wref_window, scale, what):
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


# ------------------------------------------------------------------------------------------------ stages
@pytest.mark.gpu
@pytest.mark.parametrize("n", STAGE_N)
def test_zcholesky_stage(tri_nb, n):
    """eigx_zchol_dev: leading dimension n + 2, NaN below the diagonal and in Im of the diagonal; U read from the upper
    triangle only, Im of its diagonal exactly 0"""
    B = _pencil(n)[1]
    ld = n + 2
    b = _to_dev(_nan_lower(B), ld)
    assert tri_nb.eigx_zchol_dev(n, b.data_ptr(), ld) == 0
    out = _from_dev(b, n)
    assert np.isfinite(out[np.triu_indices(n)]).all()
    assert (out.imag.diagonal() == 0.0).all()
    U = np.triu(np.nan_to_num(out, nan=0.0))
    Uref = _factor(n)
    e1 = np.linalg.norm(U.conj().T @ U - B)
    e2 = np.abs(U - Uref).max()
    print(f"  n={n}: ||U^H U - B|| = {e1:.2e} (gate {1e-12 * n * np.linalg.norm(B):.2e}), max|U - U_ref| = {e2:.2e} "
          f"(gate {1e-12 * n * np.abs(Uref).max():.2e})")
    assert e1 < 1e-12 * n * np.linalg.norm(B)
    assert e2 < 1e-12 * n * np.abs(Uref).max()


@pytest.mark.gpu
def test_zcholesky_stage_breakdown(tri_nb):
    """an indefinite B, and a B whose first non-positive pivot lies in the LAST diagonal block: EIGX_ERR_NOT_SPD"""
    from eigenexa_amd import layout

    Bi = layout.random_hermitian(50, seed=4) - np.eye(50)
    assert np.linalg.eigvalsh(Bi)[0] < 0
    b = _to_dev(_nan_lower(Bi), 52)
    assert tri_nb.eigx_zchol_dev(50, b.data_ptr(), 52) == -7
    B = np.array(_pencil(130)[1])
    B[129, 129] = -1.0
    b = _to_dev(_nan_lower(B), 132)
    assert tri_nb.eigx_zchol_dev(130, b.data_ptr(), 132) == -7
    b = _to_dev(_nan_lower(_pencil(130)[1]), 132)
    assert tri_nb.eigx_zchol_dev(130, b.data_ptr(), 132) == 0      # the flag does not stick


@pytest.mark.gpu
@pytest.mark.parametrize("n", STAGE_N)
def test_ztriangular_solve_stage(tri_nb, n):
    """eigx_ztrsm_upper_dev, op = none / conjugate transpose, nrhs = 1, 7, 64, n; below the diagonal u_dev holds NaN"""
    U = _factor(n)
    ld = n + 2
    Un = np.asfortranarray(np.where(np.triu(np.ones((n, n), dtype=bool)), U, np.nan + 1j * np.nan))
    u = _to_dev(Un, ld)
    rng = np.random.default_rng(5 + n)
    for nrhs in sorted({1, 7, 64, n}):
        R = rng.standard_normal((n, nrhs)) + 1j * rng.standard_normal((n, nrhs))
        for trans in ("N", "C"):
            x = _to_dev(R, ld)
            assert tri_nb.eigx_ztrsm_upper_dev(trans.encode(), n, nrhs, u.data_ptr(), ld, x.data_ptr(), ld) == 0
            X = _from_dev(x, n)
            assert np.isfinite(X).all()
            err = np.linalg.norm((U if trans == "N" else U.conj().T) @ X - R)
            gate = 1e-12 * n * np.linalg.norm(U) * np.linalg.norm(X)
            print(f"  n={n} nrhs={nrhs} op={trans}: ||op(U) X - R|| = {err:.2e} (gate {gate:.2e})")
            assert err < gate
    assert tri_nb.eigx_ztrsm_upper_dev(b"X", n, 1, u.data_ptr(), ld, u.data_ptr(), ld) == -2
    assert tri_nb.eigx_ztrsm_upper_dev(b"T", n, 1, u.data_ptr(), ld, u.data_ptr(), ld) == -2


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 65, 517, 1100])
def test_zreduction_stage(tri_nb, n):
    """eigx_hgev_reduce_dev: ||U^H C U - A||_F < 1e-12 n ||A||_F with C taken from its upper triangle (Re of the diagonal)"""
    A = _pencil(n)[0]
    U = _factor(n)
    ld = n + 2
    a = _to_dev(_nan_lower(A), ld)
    u = _to_dev(_nan_lower(U), ld)
    assert tri_nb.eigx_hgev_reduce_dev(n, a.data_ptr(), ld, u.data_ptr(), ld) == 0
    out = _from_dev(a, n)
    assert np.isfinite(out[np.triu_indices(n)]).all()
    Cs = np.triu(np.nan_to_num(out, nan=0.0), 1)
    Cm = Cs + Cs.conj().T + np.diag(out.real.diagonal())
    err = np.linalg.norm(U.conj().T @ Cm @ U - A)
    print(f"  n={n}: ||U^H C U - A|| = {err:.2e} (gate {1e-12 * n * np.linalg.norm(A):.2e})")
    assert err < 1e-12 * n * np.linalg.norm(A)


# ------------------------------------------------------------------------------------------------ whole solves, host API
def _solve_host(A, B, il, iu, mode="A", z_none=False):
    import eigenexa_amd as ee
    from eigenexa_amd import api

    n = A.shape[0]
    m = iu - il + 1
    a = _nan_lower(A)
    b = _nan_lower(B)
    z = None if z_none else np.full((n, m + 1), 7.0 + 7.0j, order="F")   # one guard column
    w = np.full(m + 1, 7.0)
    ee.KMATH_EIGEN_HGEV_RANGE(n, il, iu, a, n, b, n, w, z, n, mode=mode)
    assert api.last_status() == 0
    assert w[m] == 7.0
    if z is not None:
        assert (z[:, m] == 7.0 + 7.0j).all()
        if mode == "N":
            assert (z == 7.0 + 7.0j).all()
    return w[:m], (None if z is None else z[:, :m]), b


def _check_u_on_exit(b, B):
    n = B.shape[0]
    assert (b.imag.diagonal() == 0.0).all()
    U = np.triu(np.nan_to_num(b, nan=0.0))
    assert np.linalg.norm(U.conj().T @ U - B) < 1e-12 * n * np.linalg.norm(B)   # b holds U with B = U^H U


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 5, 130, 517])
def test_whole_solve_matches_scipy(gpu_lib, n):
    """host API against scipy.linalg.eigh(A, B) on the windows of test_gev_range.py with m = min(n, 24)"""
    A, B = _pencil(n)
    wref = _reference(n)
    scale = max(1.0, np.abs(wref).max())
    m = min(n, 24)
    for il, iu in sorted(set(_windows(n, m))):
        w, Z, b = _solve_host(A, B, il, iu)
        _gates(A, B, w, Z, wref[il - 1:iu], scale, f"n={n} [{il}, {iu}]")
        _check_u_on_exit(b, B)
    il, iu = 1, m
    wa, _, _ = _solve_host(A, B, il, iu)
    wn, _, _ = _solve_host(A, B, il, iu, mode="N")
    w0, _, _ = _solve_host(A, B, il, iu, mode="N", z_none=True)
    assert np.abs(wn - wa).max() < 1e-12 * scale and (w0 == wn).all()


@pytest.mark.gpu
@pytest.mark.parametrize("window", [(1, 52), (1, 517)])
def test_ill_conditioned_b(gpu_lib, window):
    """B = Q diag(logspace(0, -4, n)) Q^H, cond 1e4: the same gates"""
    n = 517
    A, B = _pencil(n, "cond1e4")
    wref = _reference(n, "cond1e4")
    scale = max(1.0, np.abs(wref).max())
    il, iu = window
    w, Z, _ = _solve_host(A, B, il, iu)
    _gates(A, B, w, Z, wref[il - 1:iu], scale, f"cond 1e4 n={n} [{il}, {iu}]")


# ------------------------------------------------------------------------------------------------ conjugation checks
@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 130])
def test_real_input_agrees_with_kmath_eigen_gev_range(gpu_lib, n):
    """real A, B in complex storage: the eigenvalues of KMATH_EIGEN_GEV_RANGE to 1e-12 scale"""
    import eigenexa_amd as ee
    from eigenexa_amd import api, layout

    A = layout.random_symmetric(n, seed=3)
    B = layout.random_hpd(n, seed=8, real=True)
    for il, iu in [(1, n), (2, min(n, 24))]:
        m = iu - il + 1
        w, Z, _ = _solve_host(A.astype(np.complex128), B.astype(np.complex128), il, iu)
        a, b = np.asfortranarray(np.triu(A)), np.asfortranarray(np.triu(B))
        wg, zg = np.zeros(m), np.zeros((n, m), order="F")
        ee.KMATH_EIGEN_GEV_RANGE(n, il, iu, a, n, b, n, wg, zg, n)
        assert api.last_status() == 0
        scale = max(1.0, np.abs(wg).max())
        print(f"  n={n} [{il}, {iu}]: |w - w_gev_range| = {np.abs(w - wg).max():.2e} (gate {1e-12 * scale:.2e})")
        assert np.abs(w - wg).max() < 1e-12 * scale


@pytest.mark.gpu
@pytest.mark.parametrize("n", [7, 260])
def test_identity_b_agrees_with_eigen_h(gpu_lib, n):
    import eigenexa_amd as ee
    from eigenexa_amd import api, layout

    A = layout.random_hermitian(n, seed=9)
    w, Z, b = _solve_host(A, np.eye(n, dtype=np.complex128), 1, n)
    assert (np.triu(np.nan_to_num(b, nan=0.0)) == np.eye(n)).all()     # U = I exactly
    ah = np.asfortranarray(A.copy())
    wh, zh = np.zeros(n), np.zeros((n, n), dtype=np.complex128, order="F")
    ee.eigen_h(n, n, ah, n, wh, zh, n)
    assert api.last_status() == 0
    scale = max(1.0, np.abs(wh).max())
    assert np.abs(w - wh).max() < 1e-12 * scale


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 130])
def test_purely_imaginary_off_diagonals(gpu_lib, n):
    """A = D1 + i K1, B = D2 + i K2 with K real antisymmetric: every off-diagonal entry is purely imaginary, so a missing
    conjugate anywhere turns the pencil into that of the transposed matrices' negatives instead of hiding in rounding"""
    import scipy.linalg

    rng = np.random.default_rng(21)
    K1 = rng.standard_normal((n, n))
    K1 = np.triu(K1, 1) - np.triu(K1, 1).T
    K2 = rng.uniform(-0.5, 0.5, (n, n))
    K2 = np.triu(K2, 1) - np.triu(K2, 1).T
    A = np.diag(rng.standard_normal(n)) + 1j * K1
    B = np.diag(n * rng.uniform(1.0, 2.0, n)) + 1j * K2          # diagonally dominant: positive definite
    wref = scipy.linalg.eigh(A, B, eigvals_only=True)
    scale = max(1.0, np.abs(wref).max())
    for il, iu in [(1, n), (2, min(n, 24))]:
        w, Z, b = _solve_host(A, B, il, iu)
        _gates(A, B, w, Z, wref[il - 1:iu], scale, f"imaginary off-diagonals n={n} [{il}, {iu}]")
        _check_u_on_exit(b, B)


@pytest.mark.gpu
def test_agrees_with_kmath_eigen_hgev(gpu_lib):
    """the same pencil through KMATH_EIGEN_HGEV (two eigen_h solves, three products): eigenvalues to 1e-12 scale, the
    B-orthogonal projector onto the lowest 52 vectors to 1e-10 n (two different methods are compared, the gate of
    test_agrees_with_kmath_eigen_gev)"""
    import eigenexa_amd as ee
    from eigenexa_amd import api

    n = 517
    A, B = _pencil(n)
    w1, Z1, _ = _solve_host(A, B, 1, n)
    a, b = _nan_lower(A), _nan_lower(B)
    Z2 = np.zeros((n, n), dtype=np.complex128, order="F")
    w2 = np.zeros(n)
    ee.KMATH_EIGEN_HGEV(n, a, n, b, n, w2, Z2, n)
    assert api.last_status() == 0
    scale = max(1.0, np.abs(_reference(n)).max())
    P1 = Z1[:, :52] @ Z1[:, :52].conj().T @ B
    P2 = Z2[:, :52] @ Z2[:, :52].conj().T @ B
    dp = np.linalg.norm(P1 - P2)
    print(f"  |w - w_hgev| = {np.abs(w1 - w2).max():.2e} (gate {1e-12 * scale:.2e}), projector difference = {dp:.2e} "
          f"(gate {1e-10 * n:.2e})")
    assert np.abs(w1 - w2).max() < 1e-12 * scale
    assert dp < 1e-10 * n


# ------------------------------------------------------------------------------------------------ device API
def _gpu_gates(A, B, w, Z, n, m, scale, what):
    import torch

    wc = w.to(torch.complex128)
    res = torch.linalg.norm(A @ Z - (B @ Z) * wc[None, :]).item()
    orth = torch.linalg.norm(Z.conj().T @ B @ Z - torch.eye(m, dtype=torch.complex128, device=_dev())).item()
    print(f"  {what}: ||AZ - BZW|| = {res:.2e} (gate {1e-12 * scale * n:.2e}), ||Z^H B Z - I|| = {orth:.2e} (gate {1e-12 * n:.2e})")
    assert res < 1e-12 * scale * n and orth < 1e-12 * n
    assert bool((w[1:] >= w[:-1]).all())


@pytest.mark.gpu
def test_device_api(gpu_lib):
    """torch tensors, n = 1200 with ld = n + 2, windows [1, 120] and [1, n]; the gates computed on the GPU; a repeat call
    is bit-identical; timers [1..4] are >= 0 and sum to at most [0]"""
    import torch
    import eigenexa_amd as ee
    from eigenexa_amd import api

    n = 1200
    A, B = _pencil(n)
    Ad, Bd = torch.from_numpy(np.array(A)).to(_dev()), torch.from_numpy(np.array(B)).to(_dev())
    ld = n + 2
    an, bn = _nan_lower(A), _nan_lower(B)
    ws = {}
    for il, iu in [(1, 120), (1, n)]:
        m = iu - il + 1
        results = []
        for rep in range(2):
            a = _to_dev(an, ld)
            b = _to_dev(bn, ld)
            z = torch.zeros(m, ld, dtype=torch.complex128, device=_dev())
            w = torch.zeros(m, dtype=torch.float64, device=_dev())
            ee.KMATH_EIGEN_HGEV_RANGE(n, il, iu, a, ld, b, ld, w, z, ld)
            assert api.last_status() == 0
            t = (C.c_double * 16)()
            gpu_lib.eigx_get_timers(t)
            assert all(t[i] >= 0 for i in range(1, 5)) and t[0] > 0, list(t)[:5]
            assert t[1] + t[2] + t[3] + t[4] <= t[0] * (1 + 1e-12), list(t)[:5]
            results.append((w, z))
        (wa, za), (wb, zb) = results
        assert torch.equal(wa, wb) and torch.equal(za[:, :n], zb[:, :n])
        ws[m] = wa
        scale = max(1.0, wa.abs().max().item())
        _gpu_gates(Ad, Bd, wa, za[:, :n].T, n, m, scale, f"n={n} [{il}, {iu}]")
    assert (ws[120] - ws[n][:120]).abs().max().item() < 1e-12 * max(1.0, ws[n].abs().max().item())


@pytest.mark.gpu
def test_gates_at_n4096(gpu_lib):
    """N = 4096, window [1, 410]: matrices made on the GPU and the gates computed there (as test_hgev_n4096_on_the_gpu)"""
    import torch
    import eigenexa_amd as ee
    from eigenexa_amd import api

    n, il, iu = 4096, 1, 410
    m = iu - il + 1
    dev = _dev()
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    S = torch.randn(n, n, dtype=torch.complex128, device=dev, generator=g)
    A = (S + S.conj().T) / 2
    X = torch.randn(n, n, dtype=torch.complex128, device=dev, generator=g)
    B = X @ X.conj().T / n + torch.eye(n, dtype=torch.complex128, device=dev)
    B = (B + B.conj().T) / 2
    del S, X
    upper = torch.triu(torch.ones(n, n, dtype=torch.bool, device=dev))
    nan = torch.full((n, n), complex(float("nan"), float("nan")), dtype=torch.complex128, device=dev)
    a = torch.where(upper, A, nan).T.contiguous()
    b = torch.where(upper, B, nan).T.contiguous()
    del nan, upper
    z = torch.zeros(m, n, dtype=torch.complex128, device=dev)
    w = torch.zeros(m, dtype=torch.float64, device=dev)
    ee.KMATH_EIGEN_HGEV_RANGE(n, il, iu, a, n, b, n, w, z, n)
    assert api.last_status() == 0
    scale = max(1.0, w.abs().max().item())
    _gpu_gates(A, B, w, z.T, n, m, scale, f"n={n} [{il}, {iu}]")


# ------------------------------------------------------------------------------------------------ statuses
@pytest.mark.gpu
def test_statuses(gpu_lib, capfd):
    """NaN in the significant triangle of a or of b: -5 and w(1:m) = NaN; bad windows, modes, pointers and leading
    dimensions: -2 with nothing touched; B indefinite: -7 and the message of KMATH_EIGEN_HGEV"""
    import eigenexa_amd as ee
    from eigenexa_amd import api, layout

    n = 50
    A, B = _pencil(n)
    z = np.zeros((n, n), dtype=np.complex128, order="F")
    for which in ("a", "b"):
        a = np.asfortranarray(np.triu(A))
        b = np.asfortranarray(np.triu(B))
        (a if which == "a" else b)[3, 7] = np.nan
        w = np.full(9, 7.0)
        ee.KMATH_EIGEN_HGEV_RANGE(n, 2, 9, a, n, b, n, w, z, n)
        assert api.last_status() == -5
        assert np.isnan(w[:8]).all() and w[8] == 7.0
    a = np.asfortranarray(np.triu(A))
    b = np.asfortranarray(np.triu(B))
    w = np.zeros(n)
    pa, pb, pw, pz = a.ctypes.data, b.ctypes.data, w.ctypes.data, z.ctypes.data
    for fn in (gpu_lib.eigx_hgev_range, gpu_lib.eigx_hgev_range_dev):   # (the checks come before any pointer is used)
        assert fn(n, 0, 5, pa, n, pb, n, pw, pz, n, b"A") == -2
        assert fn(n, 3, n + 1, pa, n, pb, n, pw, pz, n, b"A") == -2
        assert fn(n, 6, 5, pa, n, pb, n, pw, pz, n, b"A") == -2
        assert fn(n, 1, 5, pa, n, pb, n, pw, pz, n, b"X") == -2
        assert fn(n, 1, 5, pa, n, pb, n, pw, None, n, b"A") == -2
        assert fn(n, 1, 5, pa, n, None, n, pw, pz, n, b"A") == -2
        assert fn(n, 1, 5, pa, n - 1, pb, n, pw, pz, n, b"A") == -2
        assert fn(n, 1, 5, pa, n, pb, n - 1, pw, pz, n, b"A") == -2
        assert fn(n, 1, 5, pa, n, pb, n, pw, pz, n - 1, b"A") == -2
        assert fn(0, 1, 1, pa, n, pb, n, pw, pz, n, b"A") == -2
    assert (a == np.triu(A)).all() and (b == np.triu(B)).all()     # nothing was touched
    Bi = np.asfortranarray(layout.random_hermitian(n, seed=4) - np.eye(n))
    capfd.readouterr()
    ee.KMATH_EIGEN_HGEV_RANGE(n, 1, 5, a, n, Bi, n, w, z, n)
    assert api.last_status() == -7
    assert "Matrix B is not positive definite!" in capfd.readouterr().err
    # and a good call afterwards still works
    wg, Zg, _ = _solve_host(A, B, 1, 5)
    assert np.abs(wg - _reference(n)[:5]).max() < 1e-12 * max(1.0, np.abs(_reference(n)).max())


def _run_worker(*args, timeout=300):
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "hgev_range_worker.py"), *args],
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.mark.gpu
def test_before_eigen_init():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert "OK uninit" in _run_worker("uninit")


@pytest.mark.gpu
def test_workspace_bound():
    """a fresh process: after one eigx_hgev_range_dev at n = 1024, window [1, 64], default NB, the "hgevr." buffers hold at
    most (in doubles) 8 n^2 (the planes of U, A and C and the interleaved C: four complex matrices) + 2 n iu (Y) +
    6 NB (n + NB) (both planes of the block inverses, of their assembly workspace and of the solve panel) + n, times 1.15
    for the padded leading dimensions (at most 64 doubles on 1024) and the pool's 1/16 slack, and 1 MiB"""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n, iu = 1024, 64
    m = re.search(r"MEMORY hgevr=(\d+) held=(\d+) nb=(\d+)", _run_worker("memory", str(n), str(iu)))
    assert m
    hgevr, nb = int(m.group(1)), int(m.group(3))
    bound = int(1.15 * 8 * (8 * n * n + 2 * n * iu + 6 * nb * (n + nb) + n)) + 2 ** 20
    print(f"  n={n}: hgevr.* {hgevr} B, bound {bound} B")
    assert 0 < hgevr <= bound


@pytest.mark.gpu
def test_refuses_several_ranks():
    """two ranks on the one card: both print the line and return EIGX_ERR_BAD_ARG, and exit cleanly"""
    import socket

    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = os.path.join(os.path.dirname(__file__), "hgev_range_worker.py")
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
        assert o.count("one GPU only") == 1, o[-3000:]


# ------------------------------------------------------------------------------------------------ Fortran
@pytest.mark.gpu
def test_fortran_hgev_range_caller(gpu_lib, tmp_path):
    """a Fortran program calls KMATH_EIGEN_HGEV_RANGE on a pencil with Frank's spectrum, n = 200, window [3, 40]; the
    eigenvalues it prints are compared with Frank's, computed here"""
    if not os.path.exists(FLANG):
        pytest.skip("no flang")
    import json

    from eigenexa_amd import layout

    GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "known_answers.json")))
    lib = os.path.join(ROOT, "eigenexa_amd", "lib")
    mod = os.path.join(ROOT, "eigenexa_amd", "fortran", "eigen_libs_mod.F90")
    src = os.path.join(ROOT, "tests", "fortran", "hgev_range_caller.F90")
    subprocess.check_call([FLANG, "-cpp", "-O2", "-c", mod, "-o", "eigen_libs_mod.o"], cwd=tmp_path)
    subprocess.check_call([FLANG, "-cpp", "-O2", "-c", src, "-o", "hgev_range_caller.o"], cwd=tmp_path)
    subprocess.check_call([FLANG, "-o", "hgev_range_caller", "hgev_range_caller.o", "eigen_libs_mod.o", f"-L{lib}",
                           "-leigenexa_amd", f"-Wl,-rpath,{lib}"], cwd=tmp_path)
    out = subprocess.run([str(tmp_path / "hgev_range_caller")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)

    def val(label):
        m = re.search(label + r"\s*=\s*([0-9.eEdD+-]+)", out.stdout)
        assert m, out.stdout
        return float(m.group(1).replace("D", "E").replace("d", "e"))

    n, il, iu = 200, 3, 40
    lam = np.sort(layout.frank_eigenvalues(n))
    scale = max(1.0, val(r"max \|w\|"))
    rel = GOLD["gates"]["frank_rel_err"]
    assert abs(val("first eigenvalue of the window") - lam[il - 1]) < rel * lam[il - 1]
    assert abs(val("last eigenvalue of the window") - lam[iu - 1]) < rel * lam[iu - 1]
    assert val("max rel eigenvalue error") < rel
    assert val("residual norm") < 1e-12 * scale * n
    assert val("B-orthogonality norm") < 1e-12 * n
    assert val("mode N difference") < 1e-12 * scale


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", HGEVR_SYMBOLS)
def test_header_prototypes_match_the_ctypes_table(name):
    from eigenexa_amd import _lib

    params = _prototype(name)
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is C.c_int and len(argtypes) == len(params)
    for p, t in zip(params, argtypes):
        if p.startswith("char "):
            assert t is C.c_char
        elif "*" in p:
            assert t is C.c_void_p
        else:
            assert p.startswith("int ") and t is C.c_int
    # the argument lists of the real siblings
    sibling = {"eigx_hgev_range": "eigx_gev_range", "eigx_hgev_range_dev": "eigx_gev_range_dev", "eigx_zchol_dev": "eigx_chol_dev",
               "eigx_ztrsm_upper_dev": "eigx_trsm_upper_dev", "eigx_hgev_reduce_dev": "eigx_gev_reduce_dev"}[name]
    assert params == _prototype(sibling)


def test_library_exports_the_symbols():
    """the cross-compiled library has the five entry points (no GPU needed)"""
    from eigenexa_amd import _lib

    lib = _lib.load()
    for name in HGEVR_SYMBOLS:
        assert hasattr(lib, name)


def test_python_wrapper_is_exported_and_rejects_bad_windows_before_the_library(monkeypatch, capsys):
    """il < 1, iu > n, il > iu, n <= 0, a mode outside A / N, a missing z with mode A: status -2 and a warning, without
    loading the library"""
    import eigenexa_amd as ee
    from eigenexa_amd import _lib, api

    assert "KMATH_EIGEN_HGEV_RANGE" in dir(ee)
    assert "not in the reference" in ee.KMATH_EIGEN_HGEV_RANGE.__doc__

    def boom():
        raise AssertionError("the library must not be touched")

    monkeypatch.setattr(_lib, "load", boom)
    a = np.zeros((10, 10), dtype=np.complex128, order="F")
    b = np.zeros((10, 10), dtype=np.complex128, order="F")
    z = np.zeros((10, 10), dtype=np.complex128, order="F")
    w = np.zeros(10)
    for n, il, iu, zz, mode in [(10, 0, 3, z, "A"), (10, 2, 11, z, "A"), (10, 5, 4, z, "A"), (0, 1, 1, z, "A"),
                                (-1, 1, 1, z, "A"), (10, 1, 3, z, "X"), (10, 1, 3, z, "S"), (10, 1, 3, None, "A")]:
        api._state["last_status"] = 0
        ee.KMATH_EIGEN_HGEV_RANGE(n, il, iu, a, 10, b, 10, w, zz, 10, mode=mode)
        assert api.last_status() == -2
    assert "invalid window" in capsys.readouterr().err


def test_fortran_module_declares_the_subroutine():
    src = open(os.path.join(ROOT, "eigenexa_amd", "fortran", "eigen_libs_mod.F90")).read()
    assert 'bind(C, name="eigx_hgev_range")' in src
    assert re.search(r"^subroutine KMATH_EIGEN_HGEV_RANGE\(n, il, iu, a, lda, b, ldb, w, z, ldz, mode\)", src, flags=re.M)
    body = src.split("subroutine KMATH_EIGEN_HGEV_RANGE")[1]
    assert re.search(r"complex\(8\), intent\(inout\) :: a\(lda, \*\), b\(ldb, \*\), z\(ldz, \*\)", body)
    assert re.search(r"character\(\*\), intent\(in\), optional :: mode", body)
