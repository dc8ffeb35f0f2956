"""Windowed batched small complex Hermitian eigensolves (eigen_h_batch_range, an EXTENSION): eigenpairs il .. iu of every matrix
of a batch, the complex sibling of eigen_s_batch_range (tests/test_batch_range.py, which this file mirrors).  Route 1 is a window
kernel (Hermitian tridiagonalisation and phase chain, then on the real tridiagonal matrix Sturm-count multi-section, inverse
iteration, two Gram-Schmidt passes, Rayleigh-Ritz, and the complex back-transformation of m columns, all in LDS; mode 'A' for
m <= 16 and n <= 64, mode 'N' for any m and n <= 96), route 2 the kernel of eigen_h_batch into workspace with a gather of the
window, route 3 (n above the cutoff of key 22) eigx_h_range_dev matrix by matrix.  GPU tests are marked; the CPU tests at the end
check the ctypes table (_lib.HBATCH_RANGE_SIGNATURES) against the header of the entries (include/eigenexa_amd_hbatch_range.h), the
Python wrapper's argument checks and the Fortran binding.

Gates, per matrix, on the m columns against the dense A: residual ||A Z - Z W||_F / (n eps ||A||_F) against gates.residual and
orthogonality ||Z^H Z - I_m||_F / (n eps) against gates.orthogonality of tests/golden/known_answers.json, the eigenvalues against
the il .. iu slice of numpy.linalg.eigvalsh to 1e-12 max(1, max|w|), ascending, and w == 0 exactly for the zero matrix (the
matrices, the buffers and the guards of tests/test_hbatch.py)."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from c_header import prototype as _prototype
from test_hbatch import BAD_ARG, EPS, FLANG, GATE_ORTH, GATE_RES, GUARD, NONFINITE, ROOT, Batch, _dev, _families, _random_batch

ARG_NAMES = ["n", "batch", "il", "iu", "a", "lda", "stride_a", "w", "ldw", "z", "ldz", "stride_z", "mode", "info"]
SIZES = [1, 2, 3, 5, 17, 32, 33, 64, 65, 96]
MW = 16


def _eligible(n, m, mode="A"):
    """the window kernel serves mode 'N' for any m, mode 'A' for m <= MW at n <= 64 (the class of 96 has no window storage)"""
    return mode == "N" or (n <= 64 and m <= MW)


@functools.lru_cache(maxsize=None)
def _fam(n):
    """the ten families of tests/test_hbatch.py with their LAPACK eigenvalues, computed once and read-only"""
    mats = _families(n)
    ref = [np.linalg.eigvalsh(M) for M in mats]
    for M in mats + ref:
        M.setflags(write=False)
    return mats, ref


def _windows(n):
    """lowest min(n, 8), eight in the middle, top eight, (1, 1), (n, n), exactly MW wide and MW + 1 wide"""
    c = n // 2
    wins = [(1, min(n, 8)), (max(1, c - 3), min(n, max(1, c - 3) + 7)), (max(1, n - 7), n), (1, 1), (n, n), (1, min(n, MW))]
    if n >= MW + 1:
        wins.append((1, MW + 1))
    return list(dict.fromkeys(wins))


class RBatch(Batch):
    """device buffers of one windowed call: a of tests/test_hbatch.py's Batch (lda = n + 3, a padded stride, NaN in the strict
    lower triangles, the imaginary parts of the diagonal, the padding rows and the gaps); w (ldw = m + 2), z (ldz = n + 1, stride
    ldz m + 7, complex elements) and info prefilled with a guard"""

    def __init__(self, mats, il, iu):
        import torch

        super().__init__(mats)
        self.il, self.iu, self.m = il, iu, iu - il + 1
        self.ldw = self.m + 2
        self.stride_z = self.ldz * self.m + 7
        self.w = torch.full((self.ldw * self.batch,), GUARD, dtype=torch.float64, device=_dev())
        self.z = torch.full((2 * self.stride_z * self.batch,), GUARD, dtype=torch.float64, device=_dev())

    def args(self, mode=b"A", info=True, z=True):
        return (self.n, self.batch, self.il, self.iu, self.a.data_ptr(), self.lda, self.stride_a, self.w.data_ptr(), self.ldw,
                self.z.data_ptr() if z else None, self.ldz, self.stride_z, mode, self.info.data_ptr() if info else None)

    def run(self, lib, mode=b"A", info=True, z=True):
        return lib.eigx_h_batch_range_dev(*self.args(mode, info, z))

    def results(self, want_z=True):
        """w (batch, m), Z (batch, n, m) complex with Z[k][:, j] the j-th eigenvector of the window, info; asserts that the
        guards survived: nothing beyond w(1:m), z(1:n, 1:m) is written"""
        n, b, m = self.n, self.batch, self.m
        w = self.w.cpu().numpy().reshape(b, self.ldw)
        assert (w[:, m:] == GUARD).all(), "w beyond m was touched"
        zb = self.z.cpu().numpy().reshape(b, 2 * self.stride_z)
        assert (zb[:, 2 * self.ldz * m:] == GUARD).all(), "the gaps between the eigenvector blocks were touched"
        zz = zb[:, :2 * self.ldz * m].reshape(b, m, self.ldz, 2)
        assert (zz[:, :, n:] == GUARD).all(), "rows of z beyond n were touched"
        if not want_z:
            assert (zz == GUARD).all(), "z was touched"
        Z = zz[:, :, :n, 0] + 1j * zz[:, :, :n, 1]
        return w[:, :m].copy(), np.transpose(Z, (0, 2, 1)).copy(), self.info.cpu().numpy()


def _range_info(lib):
    r, m, d = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    assert lib.eigx_batch_range_info(C.byref(r), C.byref(m), C.byref(d)) == 0
    return r.value, m.value, d.value


class _Key:
    """eigx_tune(key, value) for the length of a with-block; None leaves the key alone"""

    def __init__(self, lib, key, value):
        self.lib, self.key, self.value = lib, key, value

    def __enter__(self):
        self.old = None if self.value is None else self.lib.eigx_tune(self.key, self.value)
        assert self.old != -1
        return self

    def __exit__(self, *exc):
        if self.value is not None:
            assert self.lib.eigx_tune(self.key, self.old) == self.value


def _metrics_m(A, w, Z):
    """residual and orthogonality of m columns (test_hbatch._metrics assumes n of them)"""
    n, m = Z.shape
    res = np.linalg.norm(A @ Z - Z * w[None, :]) / (n * EPS * np.linalg.norm(A))
    orth = np.linalg.norm(Z.conj().T @ Z - np.eye(m)) / (n * EPS)
    return res, orth


def _gates(A, w, Z):
    """for the zero matrix, whose residual gate leaves no room, w = 0 exactly is asked and the orthogonality gate only"""
    if not A.any():
        assert (w == 0.0).all()
        return 0.0, _metrics_m(np.eye(A.shape[0]), np.ones(len(w)), Z)[1]
    return _metrics_m(A, w, Z)


def _check_window(A, wref, il, iu, w, Z=None, tag=""):
    """eigenvalues against the il .. iu slice of numpy.linalg.eigvalsh to 1e-12 max(1, max|w|), ascending, and both gates on the
    m columns against the dense A"""
    tol = 1e-12 * max(1.0, np.abs(wref).max())
    werr = np.abs(w - wref[il - 1:iu]).max()
    assert (np.diff(w) >= 0).all(), tag
    if not A.any():
        assert (w == 0.0).all(), tag
    res = orth = 0.0
    if Z is not None:
        res, orth = _gates(A, w, Z)
    print(f"  {tag}: |w - w_lapack| = {werr:.2e} (tol {tol:.2e}), residual {res:.3e}, orthogonality {orth:.3e}")
    assert werr <= tol, tag
    assert res < GATE_RES and orth < GATE_ORTH, tag
    return res, orth


def _full_solve(lib, mats):
    """eigx_h_batch_dev on the same batch: w (batch, n), Z (batch, n, n)"""
    B = Batch(mats)
    assert B.run(lib) == 0
    w, Z, info = B.results()
    assert (info == 0).all()
    return w, Z


# ------------------------------------------------------------------------------------------------ 1. sizes, families, windows
@pytest.mark.gpu
@pytest.mark.parametrize("key", [None, 1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_families_windows(gpu_lib, n, key):
    """every window of _windows(n) on the ten families under route key `key` (None: the default); route and m from
    eigx_batch_range_info, nothing redone; with key 2 the results are bit for bit the slices of eigx_h_batch_dev; mode 'A' at
    n = 65 and 96 takes route 2 under every key"""
    mats, ref = _fam(n)
    full = _full_solve(gpu_lib, mats) if key == 2 else None
    worst = [0.0, 0.0]
    with _Key(gpu_lib, 26, key):
        for il, iu in _windows(n):
            B = RBatch(mats, il, iu)
            assert B.run(gpu_lib) == 0
            route, m, redone = _range_info(gpu_lib)
            w, Z, info = B.results()
            assert (info == 0).all() and m == iu - il + 1
            assert redone == 0, (n, il, iu)          # key 27 = 50: no family is refused
            assert route in (1, 2)
            if key is not None:
                assert route == (1 if key == 1 and _eligible(n, m) else 2), (n, il, iu, route)
            if n > 64:
                assert route == 2, (n, il, iu, route)
            for k, A in enumerate(mats):
                r, o = _check_window(A, ref[k], il, iu, w[k], Z[k], f"n={n} window {il}..{iu} matrix {k} route {route}")
                worst = [max(worst[0], r), max(worst[1], o)]
            if key == 2:
                assert (w == full[0][:, il - 1:iu]).all() and (Z == full[1][:, :, il - 1:iu]).all(), (n, il, iu)
    print(f"n={n} key 26={key}: worst residual {worst[0]:.3e}, worst orthogonality {worst[1]:.3e}")


# ------------------------------------------------------------------------------------------------ 2. redo
@pytest.mark.gpu
@pytest.mark.parametrize("n,il,iu", [(5, 2, 4), (17, 1, 8), (64, 30, 45)])
def test_redo(gpu_lib, n, il, iu):
    """key 27 = 101 refuses every matrix: all of them go to the redo, whose results are those of route 2 bit for bit"""
    mats, ref = _fam(n)
    with _Key(gpu_lib, 26, 2):
        B2 = RBatch(mats, il, iu)
        assert B2.run(gpu_lib) == 0
        assert _range_info(gpu_lib) == (2, iu - il + 1, 0)
        w2, Z2, _ = B2.results()
    with _Key(gpu_lib, 26, 1), _Key(gpu_lib, 27, 101):
        B = RBatch(mats, il, iu)
        assert B.run(gpu_lib) == 0
        assert _range_info(gpu_lib) == (1, iu - il + 1, len(mats))
    w, Z, info = B.results()
    assert (info == 0).all()
    assert (w == w2).all() and (Z == Z2).all()
    for k, A in enumerate(mats):
        _check_window(A, ref[k], il, iu, w[k], Z[k], f"redo n={n} matrix {k}")
    # only some matrices marked cannot be forced from outside; a failed matrix beside redone ones keeps its status
    bad = [M.copy() for M in mats[:4]]
    bad[2][0, n - 1] = bad[2][n - 1, 0] = np.nan
    with _Key(gpu_lib, 26, 1), _Key(gpu_lib, 27, 101):
        B = RBatch(bad, il, iu)
        assert B.run(gpu_lib) == NONFINITE
        assert _range_info(gpu_lib) == (1, iu - il + 1, 3)
    w, Z, info = B.results()
    assert info.tolist() == [0, 0, NONFINITE, 0]
    assert np.isnan(w[2]).all() and (Z[2] == GUARD + 1j * GUARD).all()
    for k in (0, 1, 3):
        assert (w[k] == w2[k]).all() and (Z[k] == Z2[k]).all()


# ------------------------------------------------------------------------------------------------ 3. bit identity
@pytest.mark.gpu
@pytest.mark.parametrize("key", [None, 1])
def test_position_independence_and_reproducibility(gpu_lib, key):
    """1500 matrices of n = 17 with window 7 .. 10: every matrix passes the gates, two runs agree bit for bit, and a matrix gives
    the same bits at position k, at position batch - 1 - k, at position 0 of a batch of three and alone"""
    n, nb, il, iu = 17, 1500, 7, 10
    fam, _ = _fam(n)
    mats = _random_batch(n, nb, 3)
    for k in range(9, nb, 10):
        mats[k] = fam[(k // 10) % len(fam)]
    with _Key(gpu_lib, 26, key):
        B = RBatch(mats, il, iu)
        assert B.run(gpu_lib) == 0
        assert _range_info(gpu_lib)[2] == 0
        w1, Z1, info = B.results()
        assert (info == 0).all()
        B.refill()
        assert B.run(gpu_lib) == 0
        w2, Z2, _ = B.results()
        assert (w1 == w2).all() and (Z1 == Z2).all()
        R = RBatch(mats[::-1], il, iu)
        assert R.run(gpu_lib) == 0
        wr, Zr, _ = R.results()
        assert (wr[::-1] == w1).all() and (Zr[::-1] == Z1).all()
        for k in (0, 9, 19, 69, 700, 1499):
            S = RBatch([mats[k]], il, iu)
            assert S.run(gpu_lib) == 0
            ws, Zs, _ = S.results()
            assert (ws[0] == w1[k]).all() and (Zs[0] == Z1[k]).all(), k
            T = RBatch([mats[k], mats[0], mats[1]], il, iu)
            assert T.run(gpu_lib) == 0
            wt, Zt, _ = T.results()
            assert (wt[0] == w1[k]).all() and (Zt[0] == Z1[k]).all(), k
    Am = np.stack(mats)
    wref = np.linalg.eigvalsh(Am)
    tol = 1e-12 * np.maximum(1.0, np.abs(wref).max(axis=1))
    assert (np.abs(w1 - wref[:, il - 1:iu]).max(axis=1) <= tol).all() and (np.diff(w1, axis=1) >= 0).all()
    anorm = np.linalg.norm(Am, axis=(1, 2))
    res = np.linalg.norm(Am @ Z1 - Z1 * w1[:, None, :], axis=(1, 2))
    orth = np.linalg.norm(np.transpose(Z1.conj(), (0, 2, 1)) @ Z1 - np.eye(iu - il + 1), axis=(1, 2)) / (n * EPS)
    zero = anorm == 0.0
    assert (res[zero] == 0.0).all() and (w1[zero] == 0.0).all()
    resg = res[~zero] / (n * EPS * anorm[~zero])
    print(f"batch {nb}, n={n}, key 26={key}: worst residual {resg.max():.3e}, worst orthogonality {orth.max():.3e}")
    assert resg.max() < GATE_RES and orth.max() < GATE_ORTH


# ------------------------------------------------------------------------------------------------ 4. mode 'N'
@pytest.mark.gpu
@pytest.mark.parametrize("key", [None, 1, 2])
@pytest.mark.parametrize("n", [5, 33, 80, 96])
def test_mode_n(gpu_lib, n, key):
    """z untouched, a NULL z accepted, every m up to n served by route 1 (n = 80 and 96 included), the eigenvalues within the
    tolerance of mode 'A''s"""
    mats, ref = _fam(n)
    with _Key(gpu_lib, 26, key):
        for il, iu in [(1, min(n, MW)), (1, n), (max(1, n - 20), n)]:
            B = RBatch(mats, il, iu)
            assert B.run(gpu_lib, mode=b"N", z=False) == 0
            route = _range_info(gpu_lib)[0]
            if key is not None:
                assert route == key
            wn, _, info = B.results(want_z=False)
            assert (info == 0).all()
            B.refill()
            assert B.run(gpu_lib, mode=b"n") == 0      # z passed but not written
            wn2, _, _ = B.results(want_z=False)
            assert (wn2 == wn).all()
            for k, A in enumerate(mats):
                _check_window(A, ref[k], il, iu, wn[k], None, f"mode N n={n} window {il}..{iu} matrix {k} route {route}")
            if iu - il + 1 <= MW:
                B.refill()
                assert B.run(gpu_lib) == 0
                wa, _, _ = B.results()
                for k in range(B.batch):
                    assert np.abs(wn[k] - wa[k]).max() <= 1e-12 * max(1.0, np.abs(wa[k]).max())


# ------------------------------------------------------------------------------------------------ 5. scale
@pytest.mark.gpu
@pytest.mark.parametrize("key", [1, 2])
@pytest.mark.parametrize("n", [20, 60])
def test_scales_in_one_batch(gpu_lib, n, key):
    """copies of one matrix scaled by 1e120, 1 and 1e-120: each is scaled by its own max|a|"""
    from eigenexa_amd import layout

    A0 = layout.random_hermitian(n, seed=4)
    wr = np.linalg.eigvalsh(A0)
    il, iu = n // 2 - 3, n // 2 + 4
    with _Key(gpu_lib, 26, key):
        B = RBatch([A0 * 1e120, A0, A0 * 1e-120], il, iu)
        assert B.run(gpu_lib) == 0
        assert _range_info(gpu_lib) == (key, 8, 0)
    w, Z, info = B.results()
    assert (info == 0).all()
    for k, f in enumerate((1e120, 1.0, 1e-120)):
        werr = np.abs(w[k] / f - wr[il - 1:iu]).max() / np.abs(wr).max()
        res, orth = _metrics_m(A0, w[k] / f, Z[k])
        print(f"  scale {f:g}: |w - w_lapack| / max|w| = {werr:.2e}, residual {res:.3e}, orthogonality {orth:.3e}")
        assert werr <= 1e-12 and res < GATE_RES and orth < GATE_ORTH


# ------------------------------------------------------------------------------------------------ 6. failures are local
@pytest.mark.gpu
@pytest.mark.parametrize("key", [1, 2])
def test_failures_are_local(gpu_lib, key):
    from eigenexa_amd import layout

    n, il, iu = 33, 10, 15
    mats = [layout.random_hermitian(n, seed=60 + k) for k in range(5)]
    ref = [np.linalg.eigvalsh(M) for M in mats]
    mats[1][4, 20] = mats[1][20, 4] = np.nan
    mats[3][0, 32] = mats[3][32, 0] = 1j * np.inf
    with _Key(gpu_lib, 26, key):
        B = RBatch(mats, il, iu)
        assert B.run(gpu_lib) == NONFINITE
        w, Z, info = B.results()
        assert info.tolist() == [0, NONFINITE, 0, NONFINITE, 0]
        for k in (1, 3):
            assert np.isnan(w[k]).all() and (Z[k] == GUARD + 1j * GUARD).all()
        for k in (0, 2, 4):
            _check_window(mats[k], ref[k], il, iu, w[k], Z[k], f"matrix {k} beside failed ones")
        err = C.c_int64(0)
        assert gpu_lib.eigx_get_errinfo(C.byref(err)) == 0 and err.value == -1
        # the status of the call is that of the first failed matrix, also with info = NULL and in mode 'N'
        B.refill()
        assert B.run(gpu_lib, mode=b"N", info=False, z=False) == NONFINITE
        wn, _, info = B.results(want_z=False)
        assert (info == 77).all() and np.isnan(wn[[1, 3]]).all() and np.isfinite(wn[[0, 2, 4]]).all()


# ------------------------------------------------------------------------------------------------ 7. above the cutoff
@pytest.mark.gpu
@pytest.mark.parametrize("n,cut", [(40, 32), (100, None)])
def test_above_the_cutoff_is_eigen_h_range(gpu_lib, n, cut):
    """key 22 = 32 at n = 40, the default at n = 100: the call is the caller's loop over eigx_h_range_dev, bit for bit"""
    from eigenexa_amd import layout

    il, iu = 5, 12
    mats = [layout.random_hermitian(n, seed=90 + k) for k in range(2)] + [_fam(n)[0][1]]
    with _Key(gpu_lib, 22, cut):
        B = RBatch(mats, il, iu)
        assert B.run(gpu_lib) == 0
        assert _range_info(gpu_lib) == (3, iu - il + 1, 0)
    w, Z, info = B.results()
    assert (info == 0).all()
    L = RBatch(mats, il, iu)
    for k in range(L.batch):
        assert gpu_lib.eigx_h_range_dev(n, il, iu, L.a.data_ptr() + 16 * k * L.stride_a, L.lda, L.w.data_ptr() + 8 * k * L.ldw,
                                        L.z.data_ptr() + 16 * k * L.stride_z, L.ldz, 48, 128, b"A") == 0
    wl, Zl, _ = L.results()
    assert (wl == w).all() and (Zl == Z).all()
    for k, A in enumerate(mats):
        _check_window(A, np.linalg.eigvalsh(A), il, iu, w[k], Z[k], f"above the cutoff n={n} matrix {k}")


# ------------------------------------------------------------------------------------------------ 8. interface
def _host_image(mats, lda):
    """a[lda, n, nb] complex128, Fortran order: the upper triangles, NaN elsewhere and in the imaginary parts of the diagonal"""
    n, nb = mats[0].shape[0], len(mats)
    up = np.tri(n, dtype=bool).T
    a = np.full((lda, n, nb), np.nan + 1j * np.nan, order="F")
    for k in range(nb):
        a[:n, :, k] = np.where(up, mats[k], np.nan + 1j * np.nan)
        a.imag[np.arange(n), np.arange(n), k] = np.nan
    return a


@pytest.mark.gpu
def test_host_and_device_forms_agree(gpu_lib):
    import eigenexa_amd as ee
    from eigenexa_amd import api

    n, nb, il, iu = 33, 5, 3, 9
    m = iu - il + 1
    mats = list(_fam(n)[0][:nb])
    B = RBatch(mats, il, iu)
    assert B.run(gpu_lib) == 0
    wd, Zd, _ = B.results()
    lda, ldz = n + 3, n + 1
    G = GUARD + 1j * GUARD
    for zcols in (m, m + 2):                        # evenly spaced blocks of z, and a padded stride
        a = _host_image(mats, lda)
        z = np.full((ldz, zcols, nb), G, order="F")
        w = np.full((m + 1, nb), GUARD, order="F")
        info = np.full(nb, 77, dtype=np.int32)
        ee.eigen_h_batch_range(n, nb, il, iu, a, lda, w, z, ldz, info=info, ldw=m + 1, stride_z=ldz * zcols)
        assert api.last_status() == 0 and (info == 0).all()
        assert api.batch_range_info().m == m
        assert (z[n:] == G).all() and (z[:, m:] == G).all() and (w[m:] == GUARD).all()
        for k in range(nb):
            assert (w[:m, k] == wd[k]).all() and (z[:n, :m, k] == Zd[k]).all()
    # the torch route of the wrapper, mode 'N'
    import torch

    B.refill()
    ee.eigen_h_batch_range(n, nb, il, iu, torch.view_as_complex(B.a.view(-1, 2)), B.lda, B.w, None, 0, mode="N",
                           stride_a=B.stride_a, ldw=B.ldw)
    assert api.last_status() == 0
    wn, _, _ = B.results(want_z=False)
    assert np.abs(wn - wd).max() <= 1e-12 * max(1.0, np.abs(wd).max())
    # a failed matrix in the host form: its z stays as it was
    a = _host_image(mats, lda)
    a[1, 2, 2] = np.inf
    z = np.full((ldz, m, nb), G, order="F")
    w = np.full((m, nb), GUARD, order="F")
    ee.eigen_h_batch_range(n, nb, il, iu, a, lda, w, z, ldz, info=info)
    assert api.last_status() == NONFINITE and info.tolist() == [0, 0, NONFINITE, 0, 0]
    assert np.isnan(w[:, 2]).all() and (z[:, :, 2] == G).all()
    for k in (0, 1, 3, 4):
        assert (w[:, k] == wd[k]).all() and (z[:n, :, k] == Zd[k]).all()


@pytest.mark.gpu
def test_host_form_with_gapped_blocks_of_z_and_a_failed_matrix(gpu_lib):
    """n = 5, il .. iu = 2 .. 4, three matrices, a NaN in the middle one, mode 'A'; z with ldz = n + 1 and stride_z = ldz m + 7 (the
    layout of RBatch), so the m columns of a matrix come back by a copy of their own.  The block of the failed matrix, the padding
    rows and the gaps keep what the caller passed; the other two blocks are those of the device form bit for bit."""
    n, nb, il, iu = 5, 3, 2, 4
    m = iu - il + 1
    mats = _random_batch(n, nb, 70)
    mats[1][0, 3] = mats[1][3, 0] = np.nan
    B = RBatch(mats, il, iu)
    assert (B.ldz, B.stride_z) == (n + 1, (n + 1) * m + 7)
    assert B.run(gpu_lib) == NONFINITE
    wd, Zd, infod = B.results()
    assert infod.tolist() == [0, NONFINITE, 0] and np.isfinite(Zd[[0, 2]]).all()
    a = B.a_host.copy()
    w, z = np.full(B.ldw * nb, GUARD), np.full(2 * B.stride_z * nb, GUARD)
    info = np.full(nb, 77, dtype=np.int32)
    rc = gpu_lib.eigx_h_batch_range(n, nb, il, iu, a.ctypes.data, B.lda, B.stride_a, w.ctypes.data, B.ldw, z.ctypes.data, B.ldz,
                                    B.stride_z, b"A", info.ctypes.data)
    assert rc == NONFINITE and info.tolist() == [0, NONFINITE, 0]
    zb = z.reshape(nb, 2 * B.stride_z)
    assert (zb[1] == GUARD).all(), "z of the failed matrix was touched"
    assert (zb[:, 2 * B.ldz * m:] == GUARD).all(), "the gaps between the eigenvector blocks were touched"
    zz = zb[:, :2 * B.ldz * m].reshape(nb, m, B.ldz, 2)
    assert (zz[:, :, n:] == GUARD).all(), "rows of z beyond n were touched"
    wh = w.reshape(nb, B.ldw)
    assert (wh[:, m:] == GUARD).all() and np.isnan(wh[1, :m]).all()
    for k in (0, 2):
        assert np.array_equal(wh[k, :m].view(np.int64), wd[k].view(np.int64)), k
        Zh = (zz[k, :, :n, 0] + 1j * zz[k, :, :n, 1]).T
        assert np.array_equal(np.ascontiguousarray(Zh).view(np.int64), np.ascontiguousarray(Zd[k]).view(np.int64)), k


@pytest.mark.gpu
def test_arguments(gpu_lib):
    n, nb, il, iu = 12, 3, 4, 8
    m = iu - il + 1
    mats = _random_batch(n, nb, 11)
    B = RBatch(mats, il, iu)
    ah = B.a_host.copy()
    wh = np.full(B.ldw * nb, GUARD)
    zh = np.full(2 * B.stride_z * nb, GUARD)
    ih = np.full(nb, 77, dtype=np.int32)
    dev = dict(zip(ARG_NAMES, B.args()))
    host = dict(dev, a=ah.ctypes.data, w=wh.ctypes.data, z=zh.ctypes.data, info=ih.ctypes.data)
    bad = [dict(n=0), dict(n=-2), dict(batch=-1), dict(il=0), dict(il=-1), dict(iu=n + 1), dict(il=9, iu=8), dict(ldw=m - 1),
           dict(ldz=n - 1), dict(stride_z=B.ldz * m - 1), dict(lda=n - 1), dict(stride_a=B.lda * n - 1), dict(a=None), dict(w=None),
           dict(z=None), dict(mode=b"X"), dict(mode=b"S"), dict(mode=b"C"), dict(mode=b"V")]
    for fn, ok in ((gpu_lib.eigx_h_batch_range_dev, dev), (gpu_lib.eigx_h_batch_range, host)):
        for change in bad:
            assert fn(*{**ok, **change}.values()) == BAD_ARG, change
        assert fn(*{**ok, "batch": 0}.values()) == 0                                  # empty batch
        assert fn(*{**ok, "batch": 0, "a": None, "w": None, "z": None, "info": None, "stride_a": 0, "stride_z": 0}.values()) == 0
    B.results()                                                                      # nothing was touched ...
    assert (B.z.cpu().numpy() == GUARD).all() and (B.w.cpu().numpy() == GUARD).all() and (B.info.cpu().numpy() == 77).all()
    assert np.array_equal(B.a.cpu().numpy(), B.a_host, equal_nan=True)
    assert np.array_equal(ah, B.a_host, equal_nan=True) and (wh == GUARD).all() and (zh == GUARD).all() and (ih == 77).all()
    # one matrix: the strides are not looked at; lower-case mode; info = NULL
    S = RBatch(mats[:1], il, iu)
    one = dict(zip(ARG_NAMES, S.args(mode=b"a", info=False)), stride_a=0, stride_z=0)
    assert gpu_lib.eigx_h_batch_range_dev(*one.values()) == 0
    w, Z, info = S.results()
    assert (info == 77).all()
    _check_window(mats[0], np.linalg.eigvalsh(mats[0]), il, iu, w[0], Z[0], "one matrix, strides 0, info NULL")
    # ldz and stride_z are ignored in mode 'N'; the timers
    assert gpu_lib.eigx_h_batch_range_dev(*{**dev, "z": None, "ldz": 0, "stride_z": 0, "mode": b"n", "info": None}.values()) == 0
    wn, _, _ = B.results(want_z=False)
    assert np.abs(wn[0] - w[0]).max() <= 1e-12 * max(1.0, np.abs(w[0]).max())
    t = (C.c_double * 16)()
    gpu_lib.eigx_get_timers(t)
    assert t[0] > 0.0 and all(t[q] == 0.0 for q in range(1, 16))


@pytest.mark.gpu
def test_hbatch_range_refuses_several_ranks():
    """two ranks on the one card: both entries return EIGX_ERR_BAD_ARG on both ranks and the processes exit cleanly"""
    import socket

    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = os.path.join(os.path.dirname(__file__), "hbatch_range_worker.py")
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


@pytest.mark.gpu
def test_fortran_hbatch_range_caller(gpu_lib, tmp_path):
    """a Fortran program calls eigen_h_batch_range of module eigen_libs_mod on four scaled phased Frank matrices of n = 30: the
    six largest eigenpairs, then the three smallest eigenvalues beside a matrix with a NaN"""
    import json

    if not os.path.exists(FLANG):
        pytest.skip("no flang")
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "known_answers.json")))
    lib = os.path.join(ROOT, "eigenexa_amd", "lib")
    mod = os.path.join(ROOT, "eigenexa_amd", "fortran", "eigen_libs_mod.F90")
    src = os.path.join(ROOT, "tests", "fortran", "hbatch_range_caller.F90")
    subprocess.check_call([FLANG, "-cpp", "-O2", "-c", mod, "-o", "eigen_libs_mod.o"], cwd=tmp_path)
    subprocess.check_call([FLANG, "-cpp", "-O2", "-c", src, "-o", "hbatch_range_caller.o"], cwd=tmp_path)
    subprocess.check_call([FLANG, "-o", "hbatch_range_caller", "hbatch_range_caller.o", "eigen_libs_mod.o", f"-L{lib}",
                           "-leigenexa_amd", f"-Wl,-rpath,{lib}"], cwd=tmp_path)
    out = subprocess.run([str(tmp_path / "hbatch_range_caller")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"max rel eigenvalue error\s*=\s*([0-9.eEdD+-]+)", out.stdout)
    assert m, out.stdout
    assert float(m.group(1).replace("D", "E").replace("d", "e")) < gold["gates"]["frank_rel_err"]
    m = re.search(r"max residual in n eps \|\|A\|\|\s*=\s*([0-9.eEdD+-]+)", out.stdout)
    assert m, out.stdout
    assert float(m.group(1).replace("D", "E").replace("d", "e")) < GATE_RES


# ------------------------------------------------------------------------------------------------ CPU
HEADER = os.path.join(ROOT, "include", "eigenexa_amd_hbatch_range.h")


@pytest.mark.parametrize("name", ["eigx_h_batch_range", "eigx_h_batch_range_dev"])
def test_header_prototypes_match_the_ctypes_table(monkeypatch, name):
    """the entries are declared in include/eigenexa_amd_hbatch_range.h and mirrored by _lib.HBATCH_RANGE_SIGNATURES: the parser of
    the other header tests, pointed at that file"""
    import c_header
    from eigenexa_amd import _lib

    monkeypatch.setattr(c_header, "HEADER", HEADER)
    params = _prototype(name)
    restype, argtypes = _lib.HBATCH_RANGE_SIGNATURES[name]
    assert restype is C.c_int and len(argtypes) == len(params) == 14
    for p, t in zip(params, argtypes):
        if p.startswith("char "):
            assert t is C.c_char
        elif "*" in p:
            assert t is C.c_void_p
        elif p.startswith("int64_t "):
            assert t is C.c_int64
        else:
            assert p.startswith("int ") and t is C.c_int
    assert [p.split()[-1].replace("_dev", "") for p in params] == ARG_NAMES


def test_the_hbatch_range_header_is_part_of_the_public_one(monkeypatch):
    """eigenexa_amd.h includes the file, the file declares exactly the two entries of the table, no name sits in another table,
    and the loaded library has them with these signatures"""
    import c_header
    from eigenexa_amd import _lib

    main = open(os.path.join(ROOT, "include", "eigenexa_amd.h")).read()
    assert re.search(r'^#include "eigenexa_amd_hbatch_range\.h"$', main, flags=re.M)
    monkeypatch.setattr(c_header, "HEADER", HEADER)
    protos = c_header.all_prototypes()
    assert set(protos) == set(_lib.HBATCH_RANGE_SIGNATURES) == {"eigx_h_batch_range", "eigx_h_batch_range_dev"}
    for other in (_lib.SIGNATURES, _lib.GBATCH_SIGNATURES, _lib.HGBATCH_SIGNATURES, _lib.VBATCH_SIGNATURES, _lib.GVBATCH_SIGNATURES,
                  _lib.BATCH_RANGE_SIGNATURES, _lib.LAB_SIGNATURES):
        assert not set(_lib.HBATCH_RANGE_SIGNATURES) & set(other)
    lib = _lib.load()
    for name, (restype, argtypes) in _lib.HBATCH_RANGE_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes


def test_python_wrapper_rejects_bad_arguments_before_the_library(monkeypatch, capsys):
    """every EIGX_ERR_BAD_ARG case of the contract: status -2 and one warning line each, without loading the library"""
    import eigenexa_amd as ee
    from eigenexa_amd import _lib, api

    def boom():
        raise AssertionError("the library must not be touched")

    monkeypatch.setattr(_lib, "load", boom)
    n, nb, il, iu = 6, 3, 2, 4
    m = iu - il + 1
    a = np.zeros((n, n, nb), dtype=np.complex128, order="F")
    z = np.zeros((n, m, nb), dtype=np.complex128, order="F")
    w = np.zeros((m, nb), order="F")
    ok = dict(n=n, batch=nb, il=il, iu=iu, a=a, lda=n, w=w, z=z, ldz=n)
    bad = [dict(n=0), dict(n=-1), dict(batch=-1), dict(il=0), dict(iu=n + 1), dict(il=5, iu=4), dict(lda=n - 1), dict(ldw=m - 1),
           dict(stride_a=n * n - 1), dict(ldz=n - 1), dict(stride_z=n * m - 1), dict(a=None), dict(w=None), dict(z=None),
           dict(mode="X"), dict(mode="C"), dict(n="x"), dict(il="x")]
    for change in bad:
        api._state["last_status"] = 0
        ee.eigen_h_batch_range(**{**ok, **change})
        assert api.last_status() == -2, change
        err = capsys.readouterr().err
        assert err.count("\n") == 1 and "eigen_h_batch_range: invalid arguments" in err
    assert "eigen_h_batch_range" in dir(ee) and "batch_range_info" in dir(ee)
    assert "eigen_h_batch_range" in api.batch_range_info.__doc__ and "eigen_s_batch_range" in api.batch_range_info.__doc__


def test_fortran_module_binds_the_hbatch_range_entry():
    src = open(os.path.join(ROOT, "eigenexa_amd", "fortran", "eigen_libs_mod.F90")).read()
    assert 'bind(C, name="eigx_h_batch_range")' in src
    assert re.search(r"public :: eigen_h_batch_range\b", src)
    body = re.search(r"subroutine eigen_h_batch_range\(n, batch, il, iu, a, lda, w, z, ldz, mode, info\)(.*?)end subroutine", src,
                     flags=re.S)
    assert body
    assert re.search(r"complex\(8\), intent\(inout\), contiguous :: a\(:, :, :\)", body.group(1))
    assert re.search(r"complex\(8\), intent\(inout\), contiguous :: z\(:, :, :\)", body.group(1))
