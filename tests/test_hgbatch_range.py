"""Windowed batched small complex generalised eigensolves (eigen_hgev_batch_range, an EXTENSION): eigenpairs il .. iu of every
Hermitian-definite pencil A x = lambda B x of a batch, the complex sibling of eigen_gev_batch_range (tests/test_gbatch_range.py,
which this file mirrors).  Route 1 is a window kernel (the complex Cholesky factor and C = U^-H A U^-1 of eigen_hgev_batch,
Hermitian tridiagonalisation of C with its phase chain, then Sturm-count multi-section, inverse iteration, two Gram-Schmidt
passes, Rayleigh-Ritz, the back-transformation of m complex columns and Z = U^-1 V, all in LDS; mode 'A' for m <= 16 at n <= 32 and
for m <= 8 at 33 <= n <= 64, mode 'N' for any m and n <= 64), route 2 eigx_hgev_batch_dev into workspace with a gather of the
window, route 3 (n above the cutoff of key 24) eigx_hgev_range_dev pencil by pencil.  On routes 1 and 2 b comes back as the U of
eigx_hgev_batch_dev, bit for bit.  GPU tests are marked; the CPU tests at the end check the ctypes table
(_lib.HGBATCH_RANGE_SIGNATURES) against the header of the entries (include/eigenexa_amd_hgbatch_range.h), the Python wrapper's
argument checks and the Fortran binding.

Gates, per pencil, those of tests/test_hgbatch.py restricted to the m columns, with w_ref the slice il .. iu of what
eigx_hgev_batch_dev returns for the pencil (itself held against scipy.linalg.eigh(A, B) by tests/test_hgbatch.py) and
scale = max(1, max|w_ref|): |w - w_ref(il:iu)| < 1e-12 scale, ||A Z - B Z W||_F < 1e-12 scale n, ||Z^H B Z - I_m||_F < 1e-12 n,
w ascending (w == 0 exactly for the zero A), and for the factor ||U^H U - B||_F < 1e-12 n ||B||_F with a real positive diagonal."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_hbatch as hb
from c_header import prototype as _prototype
from test_hbatch_range import _Key, _range_info
from test_hgbatch import (BAD_ARG, FLANG, GUARD, NONFINITE, NOT_SPD, ROOT, Pencils, _cgram, _mixed, _overlaps, _random_pencils,
                          _reference)

ARG_NAMES = ["n", "batch", "il", "iu", "a", "lda", "stride_a", "b", "ldb", "stride_b", "w", "ldw", "z", "ldz", "stride_z", "mode",
             "info"]
SIZES = [1, 2, 3, 5, 17, 32, 33, 64]      # routes 1 and 2; 65 (above the default cutoff of key 24) takes route 3
ENTRIES = ["eigx_hgev_batch_range", "eigx_hgev_batch_range_dev"]


def _width(n):
    """the widest window the class of n serves in mode 'A': 16 in the class of 32, 8 in the class of 64"""
    return 16 if n <= 32 else 8


def _eligible(n, m, mode="A"):
    return n <= 64 and (mode == "N" or m <= _width(n))


def _windows(n):
    """(1, 1), (n, n), the lowest and the highest width(n), width(n) in the middle, and one window of width(n) + 1 (the first on
    which mode 'A' is not eligible: m = 17 in the class of 32, m = 9 in the class of 64)"""
    W = min(n, _width(n))
    c = max(1, n // 2 - W // 2 + 1)
    wins = [(1, 1), (n, n), (1, W), (n - W + 1, n), (c, min(n, c + W - 1))]
    if n >= _width(n) + 1:
        wins.append((2, _width(n) + 2) if n >= _width(n) + 2 else (1, _width(n) + 1))
    return list(dict.fromkeys(wins))


class RPencils(Pencils):
    """device buffers of one windowed call: a and b of tests/test_hgbatch.py's Pencils (lda = n + 3, ldb = n + 2, padded strides,
    NaN in the strict lower triangles, the imaginary parts of the diagonals, the padding rows and the gaps; complex elements); w
    (ldw = m + 2), z (ldz = n + 1, stride ldz m + 7) and info prefilled with a guard"""

    def __init__(self, As, Bs, il, iu, **ld):
        n = As[0].shape[0]
        self.il, self.iu, self.m = il, iu, iu - il + 1
        ldz = ld.pop("ldz", None) or n + 1
        stride_z = ld.pop("stride_z", None) or ldz * self.m + 7
        super().__init__(As, Bs, ldw=self.m + 2, ldz=ldz, stride_z=stride_z, **ld)

    def args(self, mode=b"A", info=True, z=True):
        return (self.n, self.batch, self.il, self.iu, self.a.data_ptr(), self.lda, self.stride_a, self.b.data_ptr(), self.ldb,
                self.stride_b, self.w.data_ptr(), self.ldw, self.z.data_ptr() if z else None, self.ldz, self.stride_z, mode,
                self.info.data_ptr() if info else None)

    def run(self, lib, mode=b"A", info=True, z=True):
        return lib.eigx_hgev_batch_range_dev(*self.args(mode, info, z))

    def results(self, want_z=True):
        """w (batch, m), Z (batch, n, m) complex with Z[k][:, j] the j-th eigenvector of the window, U (batch, n, n) complex upper
        triangular, info, and the raw image of b; asserts that the guards survived: nothing beyond w(1:m), z(1:n, 1:m) is written,
        and the strict lower triangles, the padding rows and the gaps of b still hold their NaN"""
        n, nb, m = self.n, self.batch, self.m
        w = self.w.cpu().numpy().reshape(nb, self.ldw)
        assert (w[:, m:] == GUARD).all(), "w beyond m was touched"
        zb = self.z.cpu().numpy().reshape(nb, 2 * self.stride_z)
        assert (zb[:, 2 * self.ldz * m:] == GUARD).all(), "the gaps between the eigenvector blocks were touched"
        zz = zb[:, :2 * self.ldz * m].reshape(nb, m, self.ldz, 2)
        assert (zz[:, :, n:] == GUARD).all(), "rows of z beyond n were touched"
        if not want_z:
            assert (zz == GUARD).all(), "z was touched"
        braw = self.b.cpu().numpy()
        bb = braw.reshape(nb, 2 * self.stride_b)
        assert np.isnan(bb[:, 2 * self.ldb * n:]).all(), "the gaps between the matrices b were touched"
        bm = bb[:, :2 * self.ldb * n].reshape(nb, n, self.ldb, 2)   # bm[k, j, i] = b(i, j) of pencil k
        assert np.isnan(bm[:, :, n:]).all(), "rows of b beyond n were touched"
        lower = ~np.tri(n, dtype=bool)                         # [j, i]: i > j
        assert np.isnan(bm[:, :, :n][:, lower]).all(), "the strict lower triangle of b was written"
        Z = np.transpose(zz[:, :, :n, 0] + 1j * zz[:, :, :n, 1], (0, 2, 1)).copy()
        Ut = np.nan_to_num(bm[:, :, :n, 0], nan=0.0) + 1j * np.nan_to_num(bm[:, :, :n, 1], nan=0.0)
        U = np.triu(np.transpose(Ut, (0, 2, 1)))
        return w[:, :m].copy(), Z, U, self.info.cpu().numpy(), braw

    def b_as_passed(self, k):
        """the image of pencil k's b is what the caller passed"""
        s = 2 * self.stride_b
        return np.array_equal(self.b.cpu().numpy()[k * s:(k + 1) * s], self.b_host[k * s:(k + 1) * s], equal_nan=True)

    def z_untouched(self, k):
        s = 2 * self.stride_z
        return (self.z.cpu().numpy()[k * s:(k + 1) * s] == GUARD).all()


def _gates_m(A, B, il, iu, w, Z, U, what, wref=None):
    """test_hgbatch._gates on the m columns of the window; wref: the n eigenvalues to compare with (default: scipy's)"""
    n, m = A.shape[0], iu - il + 1
    wref = _reference(A, B) if wref is None else wref
    scale = max(1.0, np.abs(wref).max())
    werr = np.abs(w - wref[il - 1:iu]).max()
    line = f"  {what}: |w - w_ref| = {werr:.2e} (gate {1e-12 * scale:.2e})"
    assert (np.diff(w) >= 0).all(), what
    if not A.any():
        assert (w == 0.0).all(), what
    if Z is not None:
        res = np.linalg.norm(A @ Z - B @ Z * w)
        orth = np.linalg.norm(Z.conj().T @ B @ Z - np.eye(m))
        line += f", ||AZ - BZW|| = {res:.2e} (gate {1e-12 * scale * n:.2e}), ||Z^H B Z - I|| = {orth:.2e} (gate {1e-12 * n:.2e})"
    fac = np.linalg.norm(U.conj().T @ U - B)
    print(line + f", ||U^H U - B|| = {fac:.2e} (gate {1e-12 * n * np.linalg.norm(B):.2e})")
    assert werr < 1e-12 * scale, what
    if Z is not None:
        assert res < 1e-12 * scale * n, what
        assert orth < 1e-12 * n, what
    assert fac < 1e-12 * n * np.linalg.norm(B), what
    assert (np.diag(U).real > 0).all() and (np.diag(U).imag == 0).all(), what


_FULL = {}


def _full_solve(lib, As, Bs, tag):
    """eigx_hgev_batch_dev on the same pencils: w (batch, n), Z (batch, n, n), U (batch, n, n); once per tag"""
    if tag not in _FULL:
        P = Pencils(list(As), list(Bs))
        assert P.run(lib) == 0
        w, Z, U, info, _ = P.results()
        assert (info == 0).all()
        _FULL[tag] = (w, Z, U)
    return _FULL[tag]


# ------------------------------------------------------------------------------------------------ 1. sizes, pencils, windows
@pytest.mark.gpu
@pytest.mark.parametrize("key", [None, 1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_pencils_windows(gpu_lib, n, key):
    """every window of _windows(n) on the ten mixed pencils under route key `key` (None: the default); route and m from
    eigx_batch_range_info, nothing redone; with key 2 w and z are bit for bit the slices of eigx_hgev_batch_dev; a window of
    width(n) + 1 takes route 2 under every key; under every key U is bit for bit that of eigx_hgev_batch_dev; then (1, n) in mode
    'N', on route 1 under key 1"""
    As, Bs = _mixed(n)
    wf, Zf, Uf = _full_solve(gpu_lib, As, Bs, ("mixed", n))
    with _Key(gpu_lib, 26, key):
        for il, iu in _windows(n):
            P = RPencils(As, Bs, il, iu)
            assert P.run(gpu_lib) == 0
            route, m, redone = _range_info(gpu_lib)
            w, Z, U, info, _ = P.results()
            assert (info == 0).all() and m == iu - il + 1
            assert redone == 0, (n, il, iu)          # key 27 = 50: no pencil is refused
            assert route in (1, 2)
            if key is not None:
                assert route == (1 if key == 1 and _eligible(n, m) else 2), (n, il, iu, route)
            if m > _width(n):
                assert route == 2, (n, il, iu, route)
            assert (U == Uf).all(), (n, il, iu, route)
            for k in range(P.batch):
                _gates_m(As[k], Bs[k], il, iu, w[k], Z[k], U[k], f"n={n} window {il}..{iu} pencil {k} route {route}", wref=wf[k])
            if key == 2:
                assert (w == wf[:, il - 1:iu]).all() and (Z == Zf[:, :, il - 1:iu]).all(), (n, il, iu)
        P = RPencils(As, Bs, 1, n)
        assert P.run(gpu_lib, mode=b"N", z=False) == 0
        route, m, redone = _range_info(gpu_lib)
        assert (m, redone) == (n, 0) and (key is None or route == key)
        w, _, U, info, _ = P.results(want_z=False)
        assert (info == 0).all() and (U == Uf).all()
        for k in range(P.batch):
            _gates_m(As[k], Bs[k], 1, n, w[k], None, U[k], f"mode N n={n} pencil {k} route {route}", wref=wf[k])
        if key == 2:
            assert (w == wf).all()


def test_windows_show_the_eligibility_edge():
    """the case table holds m = 16 and 17 in the class of 32 and m = 8 and 9 in the class of 64"""
    for n, W in ((32, 16), (17, 16), (33, 8), (64, 8)):
        ms = {iu - il + 1 for il, iu in _windows(n)}
        assert W in ms and W + 1 in ms and max(ms) == W + 1 and 1 in ms
        assert _eligible(n, W) and not _eligible(n, W + 1) and _eligible(n, n, "N")


# ------------------------------------------------------------------------------------------------ 2. redo
@pytest.mark.gpu
@pytest.mark.parametrize("n,il,iu", [(5, 2, 4), (17, 1, 8), (64, 30, 37)])
def test_redo(gpu_lib, n, il, iu):
    """key 27 = 101 refuses every pencil: all of them go to the redo, whose w, z and U are those of route 2 bit for bit -- U is
    factored once, from B: route 1 leaves the b of a refused pencil alone"""
    As, Bs = _mixed(n)
    nb, m = len(As), iu - il + 1
    wf, _, Uf = _full_solve(gpu_lib, As, Bs, ("mixed", n))
    with _Key(gpu_lib, 26, 2):
        P2 = RPencils(As, Bs, il, iu)
        assert P2.run(gpu_lib) == 0
        assert _range_info(gpu_lib) == (2, m, 0)
        w2, Z2, U2, _, _ = P2.results()
    assert (U2 == Uf).all()
    with _Key(gpu_lib, 26, 1), _Key(gpu_lib, 27, 101):
        P = RPencils(As, Bs, il, iu)
        assert P.run(gpu_lib) == 0
        assert _range_info(gpu_lib) == (1, m, nb)
    w, Z, U, info, _ = P.results()
    assert (info == 0).all()
    assert (w == w2).all() and (Z == Z2).all() and (U == U2).all()
    for k in range(nb):
        _gates_m(As[k], Bs[k], il, iu, w[k], Z[k], U[k], f"redo n={n} pencil {k}", wref=wf[k])
    # only some pencils marked cannot be forced from outside; a failed pencil beside redone ones keeps its status, its b and z
    Ab = [M.copy() for M in As[:4]]
    Ab[2][0, n - 1] = Ab[2][n - 1, 0] = np.nan
    with _Key(gpu_lib, 26, 1), _Key(gpu_lib, 27, 101):
        P = RPencils(Ab, list(Bs[:4]), il, iu)
        assert P.run(gpu_lib) == NONFINITE
        assert _range_info(gpu_lib) == (1, m, 3)
    w, Z, U, info, _ = P.results()
    assert info.tolist() == [0, 0, NONFINITE, 0]
    assert np.isnan(w[2]).all() and P.z_untouched(2) and P.b_as_passed(2)
    for k in (0, 1, 3):
        assert (w[k] == w2[k]).all() and (Z[k] == Z2[k]).all() and (U[k] == U2[k]).all()


# ------------------------------------------------------------------------------------------------ 3. bit identity
@pytest.mark.gpu
@pytest.mark.parametrize("n,nb,il,iu", [(17, 600, 7, 10), (40, 300, 3, 10)])
def test_position_independence_and_reproducibility(gpu_lib, n, nb, il, iu):
    """key 26 = 1, more pencils than the card has compute units, one size per n-class: every pencil passes the gates, two runs
    agree bit for bit, and a pencil gives the same bits of w, z and U at position k, at position batch - 1 - k, at position 0 of
    a batch of three and alone"""
    import scipy.linalg

    m = iu - il + 1
    As, Bs = _random_pencils(n, nb, 3)
    fa, fb = _mixed(n)
    for k in range(9, nb, 10):
        As[k], Bs[k] = fa[(k // 10) % len(fa)], fb[(k // 10) % len(fb)]
    with _Key(gpu_lib, 26, 1):
        P = RPencils(As, Bs, il, iu)
        assert P.run(gpu_lib) == 0
        assert _range_info(gpu_lib) == (1, m, 0)
        w1, Z1, U1, info, _ = P.results()
        assert (info == 0).all()
        P.refill()
        assert P.run(gpu_lib) == 0
        w2, Z2, U2, _, _ = P.results()
        assert (w1 == w2).all() and (Z1 == Z2).all() and (U1 == U2).all()
        R = RPencils(As[::-1], Bs[::-1], il, iu)
        assert R.run(gpu_lib) == 0
        wr, Zr, Ur, _, _ = R.results()
        assert (wr[::-1] == w1).all() and (Zr[::-1] == Z1).all() and (Ur[::-1] == U1).all()
        for k in (0, 9, 19, 69, nb // 2, nb - 1):
            S = RPencils([As[k]], [Bs[k]], il, iu)
            assert S.run(gpu_lib) == 0
            ws, Zs, Us, _, _ = S.results()
            assert (ws[0] == w1[k]).all() and (Zs[0] == Z1[k]).all() and (Us[0] == U1[k]).all(), k
            T = RPencils([As[k], As[0], As[1]], [Bs[k], Bs[0], Bs[1]], il, iu)
            assert T.run(gpu_lib) == 0
            wt, Zt, Ut, _, _ = T.results()
            assert (wt[0] == w1[k]).all() and (Zt[0] == Z1[k]).all() and (Ut[0] == U1[k]).all(), k
    Am, Bm = np.stack(As), np.stack(Bs)
    wref = np.stack([scipy.linalg.eigh(As[k], Bs[k], eigvals_only=True, subset_by_index=(il - 1, iu - 1)) for k in range(nb)])
    wall = np.stack([scipy.linalg.eigvalsh(As[k], Bs[k], subset_by_index=(n - 1, n - 1)) for k in range(nb)])[:, 0]
    scale = np.maximum(1.0, np.maximum(np.abs(wall), np.abs(wref).max(axis=1)))
    werr = np.abs(w1 - wref).max(axis=1) / scale
    res = np.linalg.norm(Am @ Z1 - Bm @ Z1 * w1[:, None, :], axis=(1, 2)) / (scale * n)
    orth = np.linalg.norm(np.transpose(Z1.conj(), (0, 2, 1)) @ Bm @ Z1 - np.eye(m), axis=(1, 2)) / n
    fac = np.linalg.norm(np.transpose(U1.conj(), (0, 2, 1)) @ U1 - Bm, axis=(1, 2)) / (n * np.linalg.norm(Bm, axis=(1, 2)))
    print(f"batch {nb}, n={n}, key 26=1, in units of 1e-12: |w - w_ref| {werr.max() * 1e12:.3f}, residual {res.max() * 1e12:.3f}, "
          f"B-orthogonality {orth.max() * 1e12:.3f}, factor {fac.max() * 1e12:.3f}")
    assert (np.diff(w1, axis=1) >= 0).all()
    assert werr.max() < 1e-12 and res.max() < 1e-12 and orth.max() < 1e-12 and fac.max() < 1e-12


# ------------------------------------------------------------------------------------------------ 4. B = I and the zero A
@pytest.mark.gpu
@pytest.mark.parametrize("key", [1, 2])
@pytest.mark.parametrize("n", [5, 33, 64])
def test_identity_overlap_and_zero_matrix(gpu_lib, n, key):
    """B = I: U comes back as the identity exactly and the gates pass.  A = 0 with an overlap of condition 1e4: w == 0 exactly
    and Z^H B Z = I (the vectors are columns of U^-1)"""
    il, iu = max(1, n // 2 - 3), min(n, n // 2 + 4)
    m = iu - il + 1
    fam = hb._families(n)
    ill = _overlaps(n)[1]
    As = fam + [np.zeros((n, n), dtype=np.complex128)]
    Bs = [np.eye(n, dtype=np.complex128)] * len(fam) + [ill]
    with _Key(gpu_lib, 26, key):
        P = RPencils(As, Bs, il, iu)
        assert P.run(gpu_lib) == 0
        assert _range_info(gpu_lib) == (key, m, 0)
    w, Z, U, info, _ = P.results()
    assert (info == 0).all()
    assert (U[:len(fam)] == np.eye(n)).all()
    for k in range(len(fam)):
        _gates_m(As[k], Bs[k], il, iu, w[k], Z[k], U[k], f"B = I n={n} pencil {k}", wref=np.linalg.eigvalsh(As[k]))
    assert (w[-1] == 0.0).all()
    orth = np.linalg.norm(Z[-1].conj().T @ ill @ Z[-1] - np.eye(m))
    print(f"  zero A, cond(B) = 1e4, n={n}: ||Z^H B Z - I|| = {orth:.2e} (gate {1e-12 * n:.2e})")
    assert orth < 1e-12 * n
    assert np.linalg.norm(U[-1].conj().T @ U[-1] - ill) < 1e-12 * n * np.linalg.norm(ill)


# ------------------------------------------------------------------------------------------------ 5. scales
@pytest.mark.gpu
@pytest.mark.parametrize("key", [1, 2])
@pytest.mark.parametrize("n", [20, 60])
def test_scales_in_one_batch(gpu_lib, n, key):
    """one pencil with A and B scaled by 2^600, 1 and 2^-600 in one batch: each is scaled by its own maxima; the gates on the
    pencil brought back to scale 1 (w fb / fa, z sqrt(fb), U / sqrt(fb), all powers of two: exact)"""
    from eigenexa_amd import layout

    A0, B0 = hb._herm(layout.random_hermitian(n, seed=4)), _cgram(n, 9)
    il, iu = n // 2 - 3, n // 2 + 4
    big, small = 2.0 ** 600, 2.0 ** -600
    scales = [(big, 1.0), (1.0, 1.0), (small, 1.0), (1.0, big), (1.0, small), (big, big), (small, small)]
    wref = _reference(A0, B0)
    with _Key(gpu_lib, 26, key):
        P = RPencils([A0 * fa for fa, _ in scales], [B0 * fb for _, fb in scales], il, iu)
        assert P.run(gpu_lib) == 0
        assert _range_info(gpu_lib) == (key, 8, 0)
    w, Z, U, info, _ = P.results()
    assert (info == 0).all()
    for k, (fa, fb) in enumerate(scales):
        assert np.isfinite(w[k]).all() and np.isfinite(Z[k]).all() and np.isfinite(U[k]).all()
        rt = np.sqrt(fb)
        _gates_m(A0, B0, il, iu, w[k] * (fb / fa), Z[k] * rt, U[k] / rt, f"n={n} scales ({fa:g}, {fb:g})", wref=wref)


# ------------------------------------------------------------------------------------------------ 6. failures are local
@pytest.mark.gpu
@pytest.mark.parametrize("key", [1, 2])
def test_failures_are_local(gpu_lib, key):
    """a NaN in A, a NaN in B and a B that is not positive definite among good pencils: the failed ones keep b, get w = NaN and
    leave z untouched, the others are correct; the call returns the code of the lowest failed index"""
    n, il, iu = 33, 10, 15
    As, Bs = _random_pencils(n, 6, 60)
    As[1][4, 20], As[1][20, 4] = complex(np.nan, 1.0), complex(np.nan, -1.0)       # NaN in Re of A
    Bs[3][0, 32], Bs[3][32, 0] = complex(0.5, np.nan), complex(0.5, np.nan)        # NaN in Im of B
    Bs[4] = np.eye(n, dtype=np.complex128)
    Bs[4][n // 2, n // 2] = -1.0
    want = [0, NONFINITE, 0, NONFINITE, NOT_SPD, 0]
    bad, good = [1, 3, 4], [0, 2, 5]
    with _Key(gpu_lib, 26, key):
        P = RPencils(As, Bs, il, iu)
        assert P.run(gpu_lib) == NONFINITE
        assert _range_info(gpu_lib)[0] == key
        w, Z, U, info, _ = P.results()
        assert info.tolist() == want
        for k in bad:
            assert np.isnan(w[k]).all() and P.z_untouched(k) and P.b_as_passed(k), k
        for k in good:
            _gates_m(As[k], Bs[k], il, iu, w[k], Z[k], U[k], f"pencil {k} beside failed ones")
        err = C.c_int64(0)
        assert gpu_lib.eigx_get_errinfo(C.byref(err)) == 0 and err.value == -1
        # the status of the call is that of the first failed pencil, also with info = NULL and in mode 'N'
        P.refill()
        assert P.run(gpu_lib, mode=b"N", info=False, z=False) == NONFINITE
        wn, _, Un, info, _ = P.results(want_z=False)
        assert (info == 77).all() and np.isnan(wn[bad]).all() and np.isfinite(wn[good]).all()
        assert all(P.b_as_passed(k) for k in bad) and (Un[good] == U[good]).all()
        Q = RPencils(As[4:] + As[:4], Bs[4:] + Bs[:4], il, iu)
        assert Q.run(gpu_lib, info=False) == NOT_SPD


# ------------------------------------------------------------------------------------------------ 7. above the cutoff
@pytest.mark.gpu
@pytest.mark.parametrize("n,cut", [(40, 32), (65, None)])
@pytest.mark.parametrize("odd", [False, True])
def test_above_the_cutoff_is_hgev_range(gpu_lib, n, cut, odd):
    """key 24 = 32 at n = 40, the default at n = 65: the call is the caller's loop over eigx_hgev_range_dev(n, il, iu, ...) on the
    same arrays, bit for bit, with odd and with even leading dimensions; route 3; one bad pencil keeps its status"""
    il, iu = 5, 12
    m = iu - il + 1
    nb = 3
    As, Bs = _random_pencils(n, nb, 90 + n)
    ld0 = n + 2 + ((n + 2 + int(odd)) & 1)                  # even, or odd
    ld = dict(lda=ld0, ldb=ld0 + 2, ldz=ld0 + 4)
    assert all((v & 1) == int(odd) for v in ld.values())
    with _Key(gpu_lib, 24, cut):
        P = RPencils(As, Bs, il, iu, **ld)
        assert P.run(gpu_lib) == 0
        assert _range_info(gpu_lib) == (3, m, 0)
        w, Z, U, info, _ = P.results()
        assert (info == 0).all()
        Ab = [M.copy() for M in As]
        Ab[1][2, 3] = Ab[1][3, 2] = np.nan
        Q = RPencils(Ab, Bs, il, iu, **ld)
        assert Q.run(gpu_lib) == NONFINITE
        assert _range_info(gpu_lib) == (3, m, 0)
        wq, Zq, Uq, iq, _ = Q.results()
        err = C.c_int64(0)
        assert gpu_lib.eigx_get_errinfo(C.byref(err)) == 0 and err.value == -1
    assert iq.tolist() == [0, NONFINITE, 0]
    assert np.isnan(wq[1]).all() and Q.z_untouched(1) and Q.b_as_passed(1)
    L = RPencils(As, Bs, il, iu, **ld)
    for k in range(nb):
        rc = gpu_lib.eigx_hgev_range_dev(n, il, iu, L.a.data_ptr() + 16 * k * L.stride_a, L.lda, L.b.data_ptr() + 16 * k * L.stride_b,
                                         L.ldb, L.w.data_ptr() + 8 * k * L.ldw, L.z.data_ptr() + 16 * k * L.stride_z, L.ldz, b"A")
        assert rc == 0
    assert np.array_equal(L.w.cpu().numpy(), P.w.cpu().numpy())
    assert np.array_equal(L.z.cpu().numpy(), P.z.cpu().numpy())
    assert np.array_equal(L.b.cpu().numpy(), P.b.cpu().numpy(), equal_nan=True)
    for k in (0, 2):
        assert (wq[k] == w[k]).all() and (Zq[k] == Z[k]).all() and (Uq[k] == U[k]).all()
    for k in range(nb):
        _gates_m(As[k], Bs[k], il, iu, w[k], Z[k], U[k], f"above the cutoff n={n} odd={odd} pencil {k}")


# ------------------------------------------------------------------------------------------------ 8. host against device form
def _host_images(As, Bs, lda, ldb):
    """a[lda, n, nb], b[ldb, n, nb], complex128, Fortran order: the upper triangles with the real parts of the diagonals, NaN
    elsewhere"""
    n, nb = As[0].shape[0], len(As)
    up = np.tri(n, dtype=bool).T
    cnan = complex(np.nan, np.nan)
    a = np.full((lda, n, nb), cnan, order="F")
    b = np.full((ldb, n, nb), cnan, order="F")
    for k in range(nb):
        a[:n, :, k] = np.where(up, As[k], cnan)
        b[:n, :, k] = np.where(up, Bs[k], cnan)
        a.imag[np.arange(n), np.arange(n), k] = np.nan
        b.imag[np.arange(n), np.arange(n), k] = np.nan
    return a, b


@pytest.mark.gpu
def test_host_and_device_forms_agree(gpu_lib):
    import torch

    import eigenexa_amd as ee
    from eigenexa_amd import api

    n, nb, il, iu = 33, 5, 3, 9
    m = iu - il + 1
    As, Bs = _mixed(n)
    As, Bs = list(As[:nb]), list(Bs[:nb])
    P = RPencils(As, Bs, il, iu)
    assert P.run(gpu_lib) == 0
    wd, Zd, Ud, _, _ = P.results()
    lda, ldb, ldz = n + 3, n + 2, n + 1
    up = np.tri(n, dtype=bool).T
    cg = complex(GUARD, GUARD)
    info = np.full(nb, 77, dtype=np.int32)
    for zcols in (m, m + 2):                        # evenly spaced blocks of z, and a padded stride
        a, b = _host_images(As, Bs, lda, ldb)
        z = np.full((ldz, zcols, nb), cg, order="F")
        w = np.full((m + 1, nb), GUARD, order="F")
        info[:] = 77
        ee.eigen_hgev_batch_range(n, nb, il, iu, a, lda, b, ldb, w, z, ldz, info=info, ldw=m + 1, stride_z=ldz * zcols)
        assert api.last_status() == 0 and (info == 0).all()
        assert api.batch_range_info().m == m
        assert (z[n:] == cg).all() and (z[:, m:] == cg).all() and (w[m:] == GUARD).all() and np.isnan(b[n:]).all()
        for k in range(nb):
            assert (w[:m, k] == wd[k]).all() and (z[:n, :m, k] == Zd[k]).all() and (np.triu(b[:n, :, k]) == Ud[k]).all()
            assert np.isnan(b[:n, :, k][~up]).all()
    # the torch route of the wrapper, mode 'N': complex128 views of the device buffers
    P.refill()
    ee.eigen_hgev_batch_range(n, nb, il, iu, torch.view_as_complex(P.a.view(-1, 2)), P.lda, torch.view_as_complex(P.b.view(-1, 2)),
                              P.ldb, P.w, None, 0, mode="N", stride_a=P.stride_a, stride_b=P.stride_b, ldw=P.ldw)
    assert api.last_status() == 0
    wn, _, Un, _, _ = P.results(want_z=False)
    assert np.abs(wn - wd).max() <= 1e-12 * max(1.0, np.abs(wd).max()) and (Un == Ud).all()
    # failed pencils in the host form: z and b stay as they were
    a, b = _host_images(As, Bs, lda, ldb)
    a[1, 2, 2] = complex(0.0, np.inf)
    b[:n, :, 3] = np.where(up, -np.eye(n), complex(np.nan, np.nan))
    b2, b3 = b[:, :, 2].copy(), b[:, :, 3].copy()
    z = np.full((ldz, m, nb), cg, order="F")
    w = np.full((m, nb), GUARD, order="F")
    ee.eigen_hgev_batch_range(n, nb, il, iu, a, lda, b, ldb, w, z, ldz, info=info)
    assert api.last_status() == NONFINITE and info.tolist() == [0, 0, NONFINITE, NOT_SPD, 0]
    assert np.isnan(w[:, 2:4]).all() and (z[:, :, 2:4] == cg).all()
    assert np.array_equal(b[:, :, 2], b2, equal_nan=True) and np.array_equal(b[:, :, 3], b3, equal_nan=True)
    for k in (0, 1, 4):
        assert (w[:, k] == wd[k]).all() and (z[:n, :, k] == Zd[k]).all() and (np.triu(b[:n, :, k]) == Ud[k]).all()


@pytest.mark.gpu
def test_host_form_with_gapped_blocks_of_z_and_a_failed_pencil(gpu_lib):
    """n = 5, il .. iu = 2 .. 4, three pencils, a NaN in the middle one, mode 'A'; the layout of RPencils (odd and even leading
    dimensions, gapped strides) on host arrays.  The blocks of the failed pencil (z and b), the padding rows and the gaps keep what
    the caller passed; the other two are those of the device form bit for bit."""
    n, nb, il, iu = 5, 3, 2, 4
    m = iu - il + 1
    As, Bs = _random_pencils(n, nb, 70)
    As[1][0, 3] = As[1][3, 0] = np.nan
    P = RPencils(As, Bs, il, iu)
    assert (P.ldz, P.stride_z) == (n + 1, (n + 1) * m + 7)
    assert P.run(gpu_lib) == NONFINITE
    wd, Zd, Ud, infod, brawd = P.results()
    assert infod.tolist() == [0, NONFINITE, 0] and np.isfinite(Zd[[0, 2]]).all()
    a, b = P.a_host.copy(), P.b_host.copy()
    w, z = np.full(P.ldw * nb, GUARD), np.full(2 * P.stride_z * nb, GUARD)
    info = np.full(nb, 77, dtype=np.int32)
    rc = gpu_lib.eigx_hgev_batch_range(n, nb, il, iu, a.ctypes.data, P.lda, P.stride_a, b.ctypes.data, P.ldb, P.stride_b, w.ctypes.data,
                                       P.ldw, z.ctypes.data, P.ldz, P.stride_z, b"A", info.ctypes.data)
    assert rc == NONFINITE and info.tolist() == [0, NONFINITE, 0]
    assert np.array_equal(w, P.w.cpu().numpy(), equal_nan=True), "w of the host form is not that of the device form"
    zd = P.z.cpu().numpy()
    assert np.array_equal(z, zd), "z of the host form is not that of the device form"
    assert (z.reshape(nb, -1)[1] == GUARD).all(), "z of the failed pencil was touched"
    assert np.array_equal(b, brawd, equal_nan=True), "b of the host form is not that of the device form"
    assert np.array_equal(b.reshape(nb, -1)[1], P.b_host.reshape(nb, -1)[1], equal_nan=True), "b of the failed pencil was touched"


# ------------------------------------------------------------------------------------------------ 9. arguments
@pytest.mark.gpu
def test_arguments(gpu_lib):
    n, nb, il, iu = 12, 3, 4, 8
    m = iu - il + 1
    As, Bs = _random_pencils(n, nb, 11)
    P = RPencils(As, Bs, il, iu)
    ah, bh = P.a_host.copy(), P.b_host.copy()
    wh = np.full(P.ldw * nb, GUARD)
    zh = np.full(2 * P.stride_z * nb, GUARD)
    ih = np.full(nb, 77, dtype=np.int32)
    dev = dict(zip(ARG_NAMES, P.args()))
    host = dict(dev, a=ah.ctypes.data, b=bh.ctypes.data, w=wh.ctypes.data, z=zh.ctypes.data, info=ih.ctypes.data)
    bad = [dict(n=0), dict(n=-2), dict(batch=-1), dict(il=0), dict(il=-1), dict(iu=n + 1), dict(il=9, iu=8), dict(ldw=m - 1),
           dict(ldz=n - 1), dict(stride_z=P.ldz * m - 1), dict(lda=n - 1), dict(stride_a=P.lda * n - 1), dict(ldb=n - 1),
           dict(stride_b=P.ldb * n - 1), dict(a=None), dict(b=None), dict(w=None), dict(z=None), dict(mode=b"X"), dict(mode=b"S"),
           dict(mode=b"C"), dict(mode=b"V")]
    for fn, ok in ((gpu_lib.eigx_hgev_batch_range_dev, dev), (gpu_lib.eigx_hgev_batch_range, host)):
        for change in bad:
            assert fn(*{**ok, **change}.values()) == BAD_ARG, change
        assert fn(*{**ok, "batch": 0}.values()) == 0                                  # empty batch
        assert fn(*{**ok, "batch": 0, "a": None, "b": None, "w": None, "z": None, "info": None, "stride_a": 0, "stride_b": 0,
                    "stride_z": 0}.values()) == 0
    P.results(want_z=False)                                                          # nothing was touched ...
    assert (P.z.cpu().numpy() == GUARD).all() and (P.w.cpu().numpy() == GUARD).all() and (P.info.cpu().numpy() == 77).all()
    assert np.array_equal(P.a.cpu().numpy(), P.a_host, equal_nan=True) and np.array_equal(P.b.cpu().numpy(), P.b_host, equal_nan=True)
    assert np.array_equal(ah, P.a_host, equal_nan=True) and np.array_equal(bh, P.b_host, equal_nan=True)
    assert (wh == GUARD).all() and (zh == GUARD).all() and (ih == 77).all()
    # one pencil: the strides are not looked at; lower-case mode; info = NULL
    S = RPencils(As[:1], Bs[:1], il, iu)
    one = dict(zip(ARG_NAMES, S.args(mode=b"a", info=False)), stride_a=0, stride_b=0, stride_z=0)
    assert gpu_lib.eigx_hgev_batch_range_dev(*one.values()) == 0
    w, Z, U, info, _ = S.results()
    assert (info == 77).all()
    _gates_m(As[0], Bs[0], il, iu, w[0], Z[0], U[0], "one pencil, strides 0, info NULL")
    # ldz and stride_z are ignored in mode 'N'; the timers
    assert gpu_lib.eigx_hgev_batch_range_dev(*{**dev, "z": None, "ldz": 0, "stride_z": 0, "mode": b"n", "info": None}.values()) == 0
    wn, _, Un, _, _ = P.results(want_z=False)
    assert np.abs(wn[0] - w[0]).max() <= 1e-12 * max(1.0, np.abs(w[0]).max()) and (Un[0] == U[0]).all()
    t = (C.c_double * 16)()
    gpu_lib.eigx_get_timers(t)
    assert t[0] > 0.0 and all(t[q] == 0.0 for q in range(1, 16))


# ------------------------------------------------------------------------------------------------ 10. several ranks, Fortran
@pytest.mark.gpu
def test_hgbatch_range_refuses_several_ranks():
    """two ranks on the one card: both entries return EIGX_ERR_BAD_ARG on both ranks and the processes exit cleanly"""
    import socket

    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = os.path.join(os.path.dirname(__file__), "hgbatch_range_worker.py")
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
def test_fortran_hgbatch_range_caller(gpu_lib, tmp_path):
    """a Fortran program calls eigen_hgev_batch_range of module eigen_libs_mod on four complex Frank / Gram pencils of n = 30: the
    six largest eigenpairs, then the three smallest eigenvalues beside a pencil with a NaN; it prints its worst figure in units of
    each gate"""
    if not os.path.exists(FLANG):
        pytest.skip("no flang")
    lib = os.path.join(ROOT, "eigenexa_amd", "lib")
    mod = os.path.join(ROOT, "eigenexa_amd", "fortran", "eigen_libs_mod.F90")
    src = os.path.join(ROOT, "tests", "fortran", "hgbatch_range_caller.F90")
    subprocess.check_call([FLANG, "-cpp", "-O2", "-c", mod, "-o", "eigen_libs_mod.o"], cwd=tmp_path)
    subprocess.check_call([FLANG, "-cpp", "-O2", "-c", src, "-o", "hgbatch_range_caller.o"], cwd=tmp_path)
    subprocess.check_call([FLANG, "-o", "hgbatch_range_caller", "hgbatch_range_caller.o", "eigen_libs_mod.o", f"-L{lib}",
                           "-leigenexa_amd", f"-Wl,-rpath,{lib}"], cwd=tmp_path)
    out = subprocess.run([str(tmp_path / "hgbatch_range_caller")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    for what in ("residual", "B-orthogonality", "factor"):
        m = re.search(what + r" in units of its gate\s*=\s*([0-9.eEdD+-]+)", out.stdout)
        assert m, out.stdout
        assert float(m.group(1).replace("D", "E").replace("d", "e")) < 1.0, out.stdout


# ------------------------------------------------------------------------------------------------ CPU
HEADER = os.path.join(ROOT, "include", "eigenexa_amd_hgbatch_range.h")


@pytest.mark.parametrize("name", ENTRIES)
def test_header_prototypes_match_the_ctypes_table(monkeypatch, name):
    """the entries are declared in include/eigenexa_amd_hgbatch_range.h and mirrored by _lib.HGBATCH_RANGE_SIGNATURES: the parser
    of the other header tests, pointed at that file"""
    import c_header
    from eigenexa_amd import _lib

    monkeypatch.setattr(c_header, "HEADER", HEADER)
    params = _prototype(name)
    restype, argtypes = _lib.HGBATCH_RANGE_SIGNATURES[name]
    assert restype is C.c_int and len(argtypes) == len(params) == 17
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


def test_the_hgbatch_range_header_is_part_of_the_public_one(monkeypatch):
    """eigenexa_amd.h includes the file, the file declares exactly the two entries of the table, no name sits in another table,
    and the loaded library has them with these signatures"""
    import c_header
    from eigenexa_amd import _lib

    main = open(os.path.join(ROOT, "include", "eigenexa_amd.h")).read()
    assert re.search(r'^#include "eigenexa_amd_hgbatch_range\.h"$', main, flags=re.M)
    monkeypatch.setattr(c_header, "HEADER", HEADER)
    protos = c_header.all_prototypes()
    assert set(protos) == set(_lib.HGBATCH_RANGE_SIGNATURES) == set(ENTRIES)
    for other in (_lib.SIGNATURES, _lib.GBATCH_SIGNATURES, _lib.HGBATCH_SIGNATURES, _lib.VBATCH_SIGNATURES, _lib.GVBATCH_SIGNATURES,
                  _lib.BATCH_RANGE_SIGNATURES, _lib.HBATCH_RANGE_SIGNATURES, _lib.GBATCH_RANGE_SIGNATURES, _lib.LAB_SIGNATURES):
        assert not set(_lib.HGBATCH_RANGE_SIGNATURES) & set(other)
    lib = _lib.load()
    for name, (restype, argtypes) in _lib.HGBATCH_RANGE_SIGNATURES.items():
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
    b = np.zeros((n, n, nb), dtype=np.complex128, order="F")
    z = np.zeros((n, m, nb), dtype=np.complex128, order="F")
    w = np.zeros((m, nb), order="F")
    ok = dict(n=n, batch=nb, il=il, iu=iu, a=a, lda=n, b=b, ldb=n, w=w, z=z, ldz=n)
    bad = [dict(n=0), dict(n=-1), dict(batch=-1), dict(il=0), dict(iu=n + 1), dict(il=5, iu=4), dict(lda=n - 1), dict(ldb=n - 1),
           dict(ldw=m - 1), dict(stride_a=n * n - 1), dict(stride_b=n * n - 1), dict(ldz=n - 1), dict(stride_z=n * m - 1),
           dict(a=None), dict(b=None), dict(w=None), dict(z=None), dict(mode="X"), dict(mode="C"), dict(n="x"), dict(il="x")]
    for change in bad:
        api._state["last_status"] = 0
        ee.eigen_hgev_batch_range(**{**ok, **change})
        assert api.last_status() == -2, change
        err = capsys.readouterr().err
        assert err.count("\n") == 1 and "eigen_hgev_batch_range: invalid arguments" in err
    assert "eigen_hgev_batch_range" in dir(ee) and "batch_range_info" in dir(ee)
    assert "eigen_hgev_batch_range" in api.batch_range_info.__doc__


def test_fortran_module_binds_the_hgbatch_range_entry():
    src = open(os.path.join(ROOT, "eigenexa_amd", "fortran", "eigen_libs_mod.F90")).read()
    assert 'bind(C, name="eigx_hgev_batch_range")' in src
    assert re.search(r"public :: eigen_hgev_batch_range\b", src)
    body = re.search(r"subroutine eigen_hgev_batch_range\(n, batch, il, iu, a, lda, b, ldb, w, z, ldz, mode, info\)(.*?)end subroutine",
                     src, flags=re.S)
    assert body
    assert re.search(r"complex\(8\), intent\(inout\), contiguous :: a\(:, :, :\), b\(:, :, :\)", body.group(1))
    assert re.search(r"real\(8\), intent\(inout\), contiguous :: w\(:, :\)", body.group(1))
    assert re.search(r"complex\(8\), intent\(inout\), contiguous :: z\(:, :, :\)", body.group(1))
