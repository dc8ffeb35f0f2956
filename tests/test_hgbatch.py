"""Batched small complex generalised eigensolves (eigen_hgev_batch, an EXTENSION: the reference has no complex generalised
solver): one kernel launch, one workgroup per Hermitian-definite pencil A x = lambda B x with both matrices as split planes in
LDS (Cholesky B = U^H U, C = U^-H A U^-1 by two substitutions, the reduction, phase chain and QL of eigen_h_batch, Z = U^-1 Y),
n <= 64; larger n falls back to eigx_hgev_range_dev pencil by pencil.  GPU tests are marked; the CPU tests at the end check the
ctypes table (_lib.HGBATCH_SIGNATURES) against the header of the entries (include/eigenexa_amd_hgbatch.h), the Python wrapper's
argument checks, the Fortran binding and tune key 24.

Gates, per pencil, against scipy.linalg.eigh(A, B) with scale = max(1, max|w_ref|) (those of tests/test_hgev_range.py and the
factor gate of tests/test_gbatch.py): |w - w_ref| < 1e-12 scale, ||A Z - B Z W||_F < 1e-12 scale n, ||Z^H B Z - I||_F < 1e-12 n,
w ascending, ||U^H U - B||_F < 1e-12 n ||B||_F, Re diag(U) > 0 and Im diag(U) exactly 0.  A numpy complex128 model of the
route stayed at or below 0.004 (eigenvalues), 0.005 (residual), 0.16 (B-orthogonality) and 0.0003 (factor) of these gates on
random Hermitian and phased Frank A against B of cond 1e4, Gram and identity at n = 1 .. 64."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_hbatch as hb
from c_header import prototype as _prototype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLANG = os.environ.get("FC", "/opt/rocm/lib/llvm/bin/flang")
GUARD = -7.25
BAD_ARG, NONFINITE, INTERNAL, NOT_SPD = -2, -5, -6, -7
ARG_NAMES = ["n", "batch", "a", "lda", "stride_a", "b", "ldb", "stride_b", "w", "ldw", "z", "ldz", "stride_z", "mode", "info"]
ENTRIES = ["eigx_hgev_batch", "eigx_hgev_batch_dev"]


def _dev():
    import torch

    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ pencils
def _cgram(n, seed):
    rng = np.random.default_rng(700 + seed)
    G = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    return hb._herm(G @ G.conj().T / n + 0.1 * np.eye(n))


def _overlaps(n):
    """D M D^H with M the Helmert-built matrix of tests/test_gbatch.py (cond about 1.2) and D unit phases, Q diag(logspace(0,
    -4, n)) Q^H with Q complex unitary (cond 1e4), identity, a real diagonal, a seeded complex Gram matrix"""
    from eigenexa_amd import layout

    rng = np.random.default_rng(31 + n)
    ph = np.exp(1j * rng.uniform(0.0, 2.0 * np.pi, n))
    helm = layout.helmert_spectrum_matrix(n, 10)[0] if n > 1 else np.array([[10.0]])
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    ill = (Q * np.logspace(0, -4, n)) @ Q.conj().T
    mats = (ph[:, None] * helm * ph.conj()[None, :], ill, np.eye(n), np.diag(np.linspace(0.5, 3.0, n)), _cgram(n, n))
    return [hb._herm(np.asarray(M, dtype=np.complex128)) for M in mats]


@functools.lru_cache(maxsize=None)
def _mixed(n):
    """ten pencils: family k of A (those of tests/test_hbatch.py) with overlap k mod 5 -- every family and every overlap, the
    zero matrix included"""
    As, ov = hb._families(n), _overlaps(n)
    Bs = [ov[k % len(ov)] for k in range(len(As))]
    for M in As + Bs:
        M.setflags(write=False)
    return As, Bs


def _random_pencils(n, nb, seed):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((nb, n, n)) + 1j * rng.standard_normal((nb, n, n))
    Bs = G @ np.transpose(G.conj(), (0, 2, 1)) / n + 0.1 * np.eye(n)
    return hb._random_batch(n, nb, seed + 1), [hb._herm(B) for B in Bs]


def _image(mats, ld, stride):
    """the memory image of a strided batch of interleaved complex matrices (ld, stride in complex elements): upper triangles;
    NaN in the strict lower triangles, the imaginary parts of the diagonals, the padding rows and the gaps"""
    n = mats[0].shape[0]
    buf = np.full(2 * stride * len(mats), np.nan)
    upper = np.tri(n, dtype=bool)                              # [j, i]: i <= j
    for k, M in enumerate(mats):
        v = buf[2 * k * stride:2 * (k * stride + ld * n)].reshape(n, ld, 2)   # v[j, i] = m(i, j)
        v[:, :n, 0] = np.where(upper, M.T.real, np.nan)
        v[:, :n, 1] = np.where(upper, M.T.imag, np.nan)
        v[np.arange(n), np.arange(n), 1] = np.nan
    return buf


class Pencils:
    """device buffers of one call (float64 tensors holding interleaved complex; leading dimensions and strides in complex
    elements): a and b with NaN wherever the entry must not read; w, z and info prefilled with a guard"""

    def __init__(self, As, Bs, lda=None, ldb=None, ldz=None, ldw=None, stride_a=None, stride_b=None, stride_z=None):
        import torch

        self.As, self.Bs = As, Bs
        self.n = n = As[0].shape[0]
        self.batch = nb = len(As)
        self.lda = n + 3 if lda is None else lda
        self.ldb = n + 2 if ldb is None else ldb
        self.ldz = n + 1 if ldz is None else ldz
        self.ldw = n + 2 if ldw is None else ldw
        self.stride_a = self.lda * n + 5 if stride_a is None else stride_a
        self.stride_b = self.ldb * n + 3 if stride_b is None else stride_b
        self.stride_z = self.ldz * n + 7 if stride_z is None else stride_z
        self.a_host = _image(As, self.lda, self.stride_a)
        self.b_host = _image(Bs, self.ldb, self.stride_b)
        self.a = torch.from_numpy(self.a_host).to(_dev())
        self.b = torch.from_numpy(self.b_host).to(_dev())
        self.w = torch.full((self.ldw * nb,), GUARD, dtype=torch.float64, device=_dev())
        self.z = torch.full((2 * self.stride_z * nb,), GUARD, dtype=torch.float64, device=_dev())
        self.info = torch.full((nb,), 77, dtype=torch.int32, device=_dev())

    def refill(self):
        import torch

        self.a.copy_(torch.from_numpy(self.a_host))
        self.b.copy_(torch.from_numpy(self.b_host))
        self.w.fill_(GUARD)
        self.z.fill_(GUARD)
        self.info.fill_(77)

    def args(self, mode=b"A", info=True, z=True):
        return (self.n, self.batch, self.a.data_ptr(), self.lda, self.stride_a, self.b.data_ptr(), self.ldb, self.stride_b,
                self.w.data_ptr(), self.ldw, self.z.data_ptr() if z else None, self.ldz, self.stride_z, mode,
                self.info.data_ptr() if info else None)

    def run(self, lib, mode=b"A", info=True, z=True):
        return lib.eigx_hgev_batch_dev(*self.args(mode, info, z))

    def results(self, want_z=True):
        """w (batch, n), Z (batch, n, n) complex with Z[k][:, j] the j-th eigenvector, U (batch, n, n) complex upper triangular,
        info, and the raw image of b; asserts that the guards of w and z survived, and in b the NaN of the strict lower
        triangles, the padding rows and the gaps"""
        n, nb = self.n, self.batch
        w = self.w.cpu().numpy().reshape(nb, self.ldw)
        assert (w[:, n:] == GUARD).all(), "w beyond n was touched"
        zb = self.z.cpu().numpy().reshape(nb, 2 * self.stride_z)
        assert (zb[:, 2 * self.ldz * n:] == GUARD).all(), "the gaps between the eigenvector matrices were touched"
        zz = zb[:, :2 * self.ldz * n].reshape(nb, n, self.ldz, 2)
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
        return w[:, :n].copy(), Z, U, self.info.cpu().numpy(), braw

    def diag_im(self):
        """the imaginary parts of the diagonals of b as they stand in memory, (batch, n)"""
        n, nb = self.n, self.batch
        bm = self.b.cpu().numpy().reshape(nb, 2 * self.stride_b)[:, :2 * self.ldb * n].reshape(nb, n, self.ldb, 2)
        return bm[:, np.arange(n), np.arange(n), 1]


_REF = {}


def _reference(A, B):
    """scipy.linalg.eigh(A, B), eigenvalues only; computed once per pencil (by the identity of the read-only arrays)"""
    import scipy.linalg

    key = (id(A), id(B))
    if key not in _REF:
        _REF[key] = (A, B, scipy.linalg.eigh(A, B, eigvals_only=True))
    return _REF[key][2]


def _gates(A, B, w, Z, U, what, wref=None):
    n = A.shape[0]
    wref = _reference(A, B) if wref is None else wref
    scale = max(1.0, np.abs(wref).max())
    werr = np.abs(w - wref).max()
    line = f"  {what}: |w - w_ref| = {werr:.2e} (gate {1e-12 * scale:.2e})"
    assert (np.diff(w) >= 0).all(), what
    if Z is not None:
        res = np.linalg.norm(A @ Z - B @ Z * w)
        orth = np.linalg.norm(Z.conj().T @ B @ Z - np.eye(n))
        line += f", ||AZ - BZW|| = {res:.2e} (gate {1e-12 * scale * n:.2e}), ||Z^H B Z - I|| = {orth:.2e} (gate {1e-12 * n:.2e})"
    fac = np.linalg.norm(U.conj().T @ U - B)
    print(line + f", ||U^H U - B|| = {fac:.2e} (gate {1e-12 * n * np.linalg.norm(B):.2e})")
    assert werr < 1e-12 * scale, what
    if Z is not None:
        assert res < 1e-12 * scale * n, what
        assert orth < 1e-12 * n, what
    assert fac < 1e-12 * n * np.linalg.norm(B), what
    assert (np.diag(U).real > 0).all() and (np.diag(U).imag == 0).all(), what


# ------------------------------------------------------------------------------------------------ 1. sizes, families, overlaps
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 5, 17, 32, 33, 63, 64])
def test_mixed_batch(gpu_lib, n):
    As, Bs = _mixed(n)
    P = Pencils(As, Bs)
    assert P.run(gpu_lib) == 0
    w, Z, U, info, _ = P.results()
    assert (info == 0).all()
    assert (P.diag_im() == 0.0).all(), "Im of the diagonal of U is written as exactly 0"
    for k in range(P.batch):
        _gates(As[k], Bs[k], w[k], Z[k], U[k], f"n={n} pencil {k}")


# ------------------------------------------------------------------------------------------------ 2. larger batches and modes
@pytest.mark.gpu
def test_more_workgroups_than_the_card_holds_and_mode_n(gpu_lib):
    """batch = 1500 at n = 17: every pencil is checked; mode 'N' gives the same w and U bit for bit and leaves z alone"""
    import scipy.linalg

    n, nb = 17, 1500
    As, Bs = _random_pencils(n, nb, 3)
    fa, fb = _mixed(n)
    for k in range(9, nb, 10):
        As[k], Bs[k] = fa[(k // 10) % len(fa)], fb[(k // 10) % len(fb)]
    P = Pencils(As, Bs)
    assert P.run(gpu_lib) == 0
    w, Z, U, info, _ = P.results()
    assert (info == 0).all()
    Am, Bm = np.stack(As), np.stack(Bs)
    wr = np.stack([scipy.linalg.eigh(As[k], Bs[k], eigvals_only=True) for k in range(nb)])
    scale = np.maximum(1.0, np.abs(wr).max(axis=1))
    werr = np.abs(w - wr).max(axis=1) / scale
    res = np.linalg.norm(Am @ Z - Bm @ Z * w[:, None, :], axis=(1, 2)) / (scale * n)
    orth = np.linalg.norm(np.transpose(Z.conj(), (0, 2, 1)) @ Bm @ Z - np.eye(n), axis=(1, 2)) / n
    fac = np.linalg.norm(np.transpose(U.conj(), (0, 2, 1)) @ U - Bm, axis=(1, 2)) / (n * np.linalg.norm(Bm, axis=(1, 2)))
    print(f"batch {nb}, n={n}, in units of 1e-12: |w - w_ref| {werr.max() * 1e12:.3f}, residual {res.max() * 1e12:.3f}, "
          f"B-orthogonality {orth.max() * 1e12:.3f}, factor {fac.max() * 1e12:.3f}")
    assert (np.diff(w, axis=1) >= 0).all()
    assert werr.max() < 1e-12 and res.max() < 1e-12 and orth.max() < 1e-12 and fac.max() < 1e-12
    dU = np.diagonal(U, axis1=1, axis2=2)
    assert (dU.real > 0).all() and (P.diag_im() == 0.0).all()
    P.refill()
    assert P.run(gpu_lib, mode=b"N", z=False) == 0
    wn, _, Un, info, _ = P.results(want_z=False)
    assert (info == 0).all()
    assert (wn == w).all() and (Un == U).all() and (P.diag_im() == 0.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 33, 64])
def test_mode_n_matches_mode_a(gpu_lib, n):
    As, Bs = _mixed(n)
    P = Pencils(As, Bs)
    assert P.run(gpu_lib) == 0
    wa, _, Ua, _, _ = P.results()
    P.refill()
    assert P.run(gpu_lib, mode=b"n", z=False) == 0
    wn, _, Un, info, _ = P.results(want_z=False)
    assert (info == 0).all()
    assert (wn == wa).all() and (Un == Ua).all()
    for k in range(P.batch):
        _gates(As[k], Bs[k], wn[k], None, Un[k], f"mode N n={n} pencil {k}")


# ------------------------------------------------------------------------------------------------ 3. B = I is eigx_h_batch
@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 33, 64])
def test_identity_overlap_is_eigen_h_batch(gpu_lib, n):
    """with B = I every substitution is exact and the reduction and QL have the arithmetic of eigx_h_batch: w and both planes
    of z bit for bit those of eigx_h_batch_dev on the same A (one of them scaled: max|a| = 1e100), and U = I exactly"""
    import torch

    As = hb._families(n) + [hb._families(n)[0] * 1e100]
    nb = len(As)
    P = Pencils(As, [np.eye(n, dtype=np.complex128)] * nb)
    assert P.run(gpu_lib) == 0
    w, Z, U, info, _ = P.results()
    assert (info == 0).all()
    assert (U == np.eye(n)).all()
    a = torch.from_numpy(P.a_host).to(_dev())
    ws = torch.full((P.ldw * nb,), GUARD, dtype=torch.float64, device=_dev())
    zs = torch.full((2 * P.stride_z * nb,), GUARD, dtype=torch.float64, device=_dev())
    assert gpu_lib.eigx_h_batch_dev(n, nb, a.data_ptr(), P.lda, P.stride_a, ws.data_ptr(), P.ldw, zs.data_ptr(), P.ldz, P.stride_z,
                                    b"A", None) == 0
    assert np.array_equal(ws.cpu().numpy(), P.w.cpu().numpy())
    assert np.array_equal(zs.cpu().numpy().view(np.int64), P.z.cpu().numpy().view(np.int64))   # both planes, signs of zeros too
    for k in (0, 1, nb - 1):
        _gates(As[k], np.eye(n), w[k], Z[k], U[k], f"B = I n={n} pencil {k}", wref=np.linalg.eigvalsh(As[k]))


# ------------------------------------------------------------------------------------------------ 4. real data
@pytest.mark.gpu
@pytest.mark.parametrize("n", [20, 48])
def test_real_data_against_eigen_gev_batch(gpu_lib, n):
    """pencils with Im = 0 everywhere: the eigenvalues agree with those of eigx_gev_batch_dev on the real arrays to the
    eigenvalue gate (bit identity is not expected: the reflectors differ), and every gate holds"""
    import torch

    import test_gbatch as gb

    Ar, Br = gb._mixed(n)
    As = [np.asarray(M, dtype=np.complex128) for M in Ar]
    Bs = [np.asarray(M, dtype=np.complex128) for M in Br]
    P = Pencils(As, Bs)
    assert P.run(gpu_lib) == 0
    w, Z, U, info, _ = P.results()
    assert (info == 0).all()
    R = gb.Pencils(list(Ar), list(Br))
    assert R.run(gpu_lib) == 0
    wr, _, _, infor, _ = R.results()
    assert (infor == 0).all()
    for k in range(P.batch):
        wref = gb._reference(Ar[k], Br[k])
        scale = max(1.0, np.abs(wref).max())
        print(f"  n={n} pencil {k}: |w - w_real| = {np.abs(w[k] - wr[k]).max():.2e} (gate {1e-12 * scale:.2e})")
        assert np.abs(w[k] - wr[k]).max() < 1e-12 * scale, k
        _gates(As[k], Bs[k], w[k], Z[k], U[k], f"real data n={n} pencil {k}", wref=wref)


# ------------------------------------------------------------------------------------------------ 5. bit identity
@pytest.mark.gpu
def test_position_independence_and_reproducibility(gpu_lib):
    n, nb = 40, 24
    fa, fb = _mixed(n)
    Ar, Br = _random_pencils(n, nb - len(fa), 8)
    As, Bs = list(fa) + Ar, list(fb) + Br
    P = Pencils(As, Bs)
    assert P.run(gpu_lib) == 0
    w1, Z1, U1, _, _ = P.results()
    P.refill()
    assert P.run(gpu_lib) == 0
    w2, Z2, U2, _, _ = P.results()
    assert (w1 == w2).all() and (Z1 == Z2).all() and (U1 == U2).all()
    order = list(range(nb))[::-1]                           # every pencil at another position
    Q = Pencils([As[k] for k in order], [Bs[k] for k in order])
    assert Q.run(gpu_lib) == 0
    wq, Zq, Uq, _, _ = Q.results()
    for p, k in enumerate(order):
        assert (wq[p] == w1[k]).all() and (Zq[p] == Z1[k]).all() and (Uq[p] == U1[k]).all(), k
    for k in (0, 3, 11, nb - 1):                             # ... and alone
        S = Pencils([As[k]], [Bs[k]])
        assert S.run(gpu_lib) == 0
        ws, Zs, Us, _, _ = S.results()
        assert (ws[0] == w1[k]).all() and (Zs[0] == Z1[k]).all() and (Us[0] == U1[k]).all(), k


# ------------------------------------------------------------------------------------------------ 6. scales
@pytest.mark.gpu
@pytest.mark.parametrize("n", [20, 50])
def test_scales_in_one_batch(gpu_lib, n):
    """A and B each of magnitude 1e120, 1e60, 1, 1e-60, 1e-120, all 25 combinations in one batch: each pencil is scaled by its
    own maxima; the gates on the pencil brought back to scale 1 (w fb / fa, z sqrt(fb), U / sqrt(fb))"""
    from eigenexa_amd import layout

    A0, B0 = hb._herm(layout.random_hermitian(n, seed=4)), _cgram(n, 9)
    A0.setflags(write=False)
    B0.setflags(write=False)
    mags = [1e120, 1e60, 1.0, 1e-60, 1e-120]
    scales = [(fa, fb) for fa in mags for fb in mags]
    P = Pencils([A0 * fa for fa, _ in scales], [B0 * fb for _, fb in scales])
    assert P.run(gpu_lib) == 0
    w, Z, U, info, _ = P.results()
    assert (info == 0).all()
    for k, (fa, fb) in enumerate(scales):
        assert np.isfinite(w[k]).all() and np.isfinite(Z[k]).all() and np.isfinite(U[k]).all()
        rt = np.sqrt(fb)
        _gates(A0, B0, w[k] * (fb / fa), Z[k] * rt, U[k] / rt, f"n={n} scales ({fa:g}, {fb:g})")


# ------------------------------------------------------------------------------------------------ 7. failures are local
@pytest.mark.gpu
def test_failures_are_local(gpu_lib):
    n = 33
    As, Bs = _random_pencils(n, 9, 60)
    As[1][4, 20], As[1][20, 4] = complex(np.nan, 1.0), complex(np.nan, -1.0)       # NaN in Re of A
    Bs[3][0, 32], Bs[3][32, 0] = complex(0.5, np.inf), complex(0.5, -np.inf)       # Inf in Im of B
    for k, pos in ((4, 0), (5, n // 2), (6, n - 1)):
        Bs[k] = np.eye(n, dtype=np.complex128)
        Bs[k][pos, pos] = -1.0
    Bs[7] = np.zeros((n, n), dtype=np.complex128)
    want = [0, NONFINITE, 0, NONFINITE, NOT_SPD, NOT_SPD, NOT_SPD, NOT_SPD, 0]
    failed = [k for k in range(9) if want[k]]
    P = Pencils(As, Bs)
    assert P.run(gpu_lib) == NONFINITE
    w, Z, U, info, braw = P.results()
    assert info.tolist() == want
    # b of every failed pencil is as it was passed, its z untouched
    assert np.array_equal(braw.reshape(9, -1)[failed], P.b_host.reshape(9, -1)[failed], equal_nan=True)
    zraw = P.z.cpu().numpy().reshape(9, -1)
    for k in range(9):
        if want[k]:
            assert np.isnan(w[k]).all() and (zraw[k] == GUARD).all(), k
        else:
            _gates(As[k], Bs[k], w[k], Z[k], U[k], f"pencil {k} beside failed ones")
    # the return value is the code of the lowest failed index, also with info = NULL
    P.refill()
    assert P.run(gpu_lib, info=False) == NONFINITE
    assert (P.info.cpu().numpy() == 77).all()
    wi, Zi, Ui, _, _ = P.results()
    good = [k for k in range(9) if not want[k]]
    assert (wi[good] == w[good]).all() and (Zi[good] == Z[good]).all() and (Ui[good] == U[good]).all()
    Q = Pencils(As[4:] + As[:4], Bs[4:] + Bs[:4])
    assert Q.run(gpu_lib, info=False) == NOT_SPD
    Q.refill()
    assert Q.run(gpu_lib, mode=b"N", z=False) == NOT_SPD
    wq, _, _, iq, bq = Q.results(want_z=False)
    assert iq.tolist() == want[4:] + want[:4]
    assert (wq[4] == w[8]).all() and (wq[5] == w[0]).all() and np.isnan(wq[0]).all()
    fq = [k for k in range(9) if iq[k]]
    assert np.array_equal(bq.reshape(9, -1)[fq], Q.b_host.reshape(9, -1)[fq], equal_nan=True)


# ------------------------------------------------------------------------------------------------ 8. fallback
@pytest.mark.gpu
@pytest.mark.parametrize("n,key", [(40, 32), (65, None)])
@pytest.mark.parametrize("odd", [False, True])
def test_fallback_is_hgev_range(gpu_lib, n, key, odd):
    """above the cutoff (key 24 = 32 at n = 40; the default at n = 65) the call is the caller's loop over
    eigx_hgev_range_dev(n, 1, n, ...) on the same arrays, bit for bit, with odd and with even leading dimensions"""
    nb = 3
    As, Bs = _random_pencils(n, nb, 90 + n)
    ld0 = n + 2 + ((n + 2 + int(odd)) & 1)                  # even, or odd
    ld = dict(lda=ld0, ldb=ld0 + 2, ldz=ld0 + 4)
    assert all((v & 1) == int(odd) for v in ld.values())
    P = Pencils(As, Bs, **ld)
    old = gpu_lib.eigx_tune(24, key) if key is not None else None
    try:
        assert old in (None, 64)
        assert P.run(gpu_lib) == 0
    finally:
        if key is not None:
            assert gpu_lib.eigx_tune(24, old) == key
    w, Z, U, info, _ = P.results()
    assert (info == 0).all()
    L = Pencils(As, Bs, **ld)
    for k in range(nb):
        rc = gpu_lib.eigx_hgev_range_dev(n, 1, n, L.a.data_ptr() + 16 * k * L.stride_a, L.lda, L.b.data_ptr() + 16 * k * L.stride_b,
                                         L.ldb, L.w.data_ptr() + 8 * k * L.ldw, L.z.data_ptr() + 16 * k * L.stride_z, L.ldz, b"A")
        assert rc == 0
    assert np.array_equal(L.w.cpu().numpy(), P.w.cpu().numpy())
    assert np.array_equal(L.z.cpu().numpy(), P.z.cpu().numpy())
    assert np.array_equal(L.b.cpu().numpy(), P.b.cpu().numpy(), equal_nan=True)
    for k in range(nb):
        _gates(As[k], Bs[k], w[k], Z[k], U[k], f"fallback n={n} odd={odd} pencil {k}")


@pytest.mark.gpu
def test_fallback_reports_per_pencil(gpu_lib):
    """key 24 = 0: every n takes the loop; a NaN and an indefinite B among good pencils, mode 'N': the statuses and w are those
    of the caller's loop"""
    n = 12
    As, Bs = _random_pencils(n, 4, 33)
    As[1][2, 3] = np.nan
    As[1][3, 2] = np.nan
    Bs[2] = -np.eye(n, dtype=np.complex128)
    P = Pencils(As, Bs)
    old = gpu_lib.eigx_tune(24, 0)
    try:
        assert P.run(gpu_lib, mode=b"N", z=False) == NONFINITE
    finally:
        assert gpu_lib.eigx_tune(24, old) == 0
    w, _, U, info, braw = P.results(want_z=False)
    L = Pencils(As, Bs)
    rcs = [gpu_lib.eigx_hgev_range_dev(n, 1, n, L.a.data_ptr() + 16 * k * L.stride_a, L.lda, L.b.data_ptr() + 16 * k * L.stride_b,
                                       L.ldb, L.w.data_ptr() + 8 * k * L.ldw, None, L.ldz, b"N") for k in range(4)]
    assert info.tolist() == rcs == [0, NONFINITE, NOT_SPD, 0]
    assert np.isnan(w[1]).all()
    assert np.array_equal(braw.reshape(4, -1)[1], P.b_host.reshape(4, -1)[1], equal_nan=True)
    wl = L.w.cpu().numpy().reshape(4, L.ldw)[:, :n]
    assert np.array_equal(wl[[0, 1, 3]], w[[0, 1, 3]], equal_nan=True)
    assert np.array_equal(L.b.cpu().numpy(), braw, equal_nan=True)
    for k in (0, 3):
        _gates(As[k], Bs[k], w[k], None, U[k], f"fallback mode N pencil {k}")


# ------------------------------------------------------------------------------------------------ 9. host and device forms
@pytest.mark.gpu
def test_host_and_device_forms_agree(gpu_lib):
    import eigenexa_amd as ee
    from eigenexa_amd import api

    n, nb = 33, 5
    As, Bs = _mixed(n)
    As, Bs = list(As[:nb]), list(Bs[:nb])
    P = Pencils(As, Bs)
    assert P.run(gpu_lib) == 0
    wd, Zd, Ud, _, _ = P.results()
    lda, ldb, ldz = n + 3, n + 2, n + 1
    up = np.tri(n, dtype=bool).T
    cnan = complex(np.nan, np.nan)

    def fill():
        a = np.full((lda, n, nb), cnan, order="F")
        b = np.full((ldb, n, nb), cnan, order="F")
        for k in range(nb):
            a[:n, :, k] = np.where(up, As[k], cnan)
            b[:n, :, k] = np.where(up, Bs[k], cnan)
            a.imag[np.arange(n), np.arange(n), k] = np.nan   # (of the diagonals the real parts only)
            b.imag[np.arange(n), np.arange(n), k] = np.nan
        return a, b

    a, b = fill()
    z = np.full((ldz, n, nb), complex(GUARD, GUARD), order="F")
    w = np.full((n, nb), GUARD, order="F")
    info = np.full(nb, 77, dtype=np.int32)
    ee.eigen_hgev_batch(n, nb, a, lda, b, ldb, w, z, ldz, info=info)
    assert api.last_status() == 0 and (info == 0).all()
    assert (z[n:] == complex(GUARD, GUARD)).all() and np.isnan(b[n:]).all()
    for k in range(nb):
        assert (w[:, k] == wd[k]).all() and (z[:n, :, k] == Zd[k]).all() and (np.triu(b[:n, :, k]) == Ud[k]).all()
        assert np.isnan(b[:n, :, k][~up]).all()
    # the torch route of the wrapper, mode 'N': complex128 views of the device buffers
    import torch

    P.refill()
    ee.eigen_hgev_batch(n, nb, torch.view_as_complex(P.a.view(-1, 2)), P.lda, torch.view_as_complex(P.b.view(-1, 2)), P.ldb, P.w, None,
                        0, mode="N", stride_a=P.stride_a, stride_b=P.stride_b, ldw=P.ldw)
    assert api.last_status() == 0
    wn, _, Un, _, _ = P.results(want_z=False)
    assert (wn == wd).all() and (Un == Ud).all()
    # failed pencils in the host form: z and b stay as they were
    a, b = fill()
    a[1, 2, 2] = complex(0.0, np.inf)
    b[:n, :, 3] = np.where(up, -np.eye(n), cnan)
    b3 = b[:, :, 3].copy()
    b2 = b[:, :, 2].copy()
    z[:] = complex(GUARD, GUARD)
    ee.eigen_hgev_batch(n, nb, a, lda, b, ldb, w, z, ldz, info=info)
    assert api.last_status() == NONFINITE and info.tolist() == [0, 0, NONFINITE, NOT_SPD, 0]
    assert np.isnan(w[:, 2]).all() and np.isnan(w[:, 3]).all() and (z[:, :, 2:4] == complex(GUARD, GUARD)).all()
    assert np.array_equal(b[:, :, 2], b2, equal_nan=True) and np.array_equal(b[:, :, 3], b3, equal_nan=True)
    for k in (0, 1, 4):
        assert (w[:, k] == wd[k]).all() and (z[:n, :, k] == Zd[k]).all() and (np.triu(b[:n, :, k]) == Ud[k]).all()


# ------------------------------------------------------------------------------------------------ 10. arguments
@pytest.mark.gpu
def test_arguments(gpu_lib):
    n, nb = 12, 3
    As, Bs = _random_pencils(n, nb, 1)
    P = Pencils(As, Bs)
    ah, bh = P.a_host.copy(), P.b_host.copy()
    wh = np.full(P.ldw * nb, GUARD)
    zh = np.full(2 * P.stride_z * nb, GUARD)
    ih = np.full(nb, 77, dtype=np.int32)
    dev = dict(zip(ARG_NAMES, P.args()))
    host = dict(dev, a=ah.ctypes.data, b=bh.ctypes.data, w=wh.ctypes.data, z=zh.ctypes.data, info=ih.ctypes.data)
    bad = [dict(n=0), dict(n=-2), dict(batch=-1), dict(lda=n - 1), dict(ldb=n - 1), dict(ldw=n - 1), dict(ldz=n - 1),
           dict(stride_a=P.lda * n - 1), dict(stride_b=P.ldb * n - 1), dict(stride_z=P.ldz * n - 1), dict(a=None), dict(b=None),
           dict(w=None), dict(z=None), dict(mode=b"X"), dict(mode=b"S"), dict(mode=b"C"), dict(mode=b"V")]
    for fn, ok in ((gpu_lib.eigx_hgev_batch_dev, dev), (gpu_lib.eigx_hgev_batch, host)):
        for change in bad:
            assert fn(*{**ok, **change}.values()) == BAD_ARG, change
        assert fn(*{**ok, "batch": 0}.values()) == 0                                  # empty batch
        assert fn(*{**ok, "batch": 0, "a": None, "b": None, "w": None, "z": None, "info": None, "stride_a": 0, "stride_b": 0,
                    "stride_z": 0}.values()) == 0
    # nothing was touched ...
    assert (P.z.cpu().numpy() == GUARD).all() and (P.w.cpu().numpy() == GUARD).all() and (P.info.cpu().numpy() == 77).all()
    assert np.array_equal(P.a.cpu().numpy(), P.a_host, equal_nan=True) and np.array_equal(P.b.cpu().numpy(), P.b_host, equal_nan=True)
    assert np.array_equal(ah, P.a_host, equal_nan=True) and np.array_equal(bh, P.b_host, equal_nan=True)
    assert (wh == GUARD).all() and (zh == GUARD).all() and (ih == 77).all()
    # one pencil: the strides are not looked at; lower-case mode; info = NULL
    S = Pencils(As[:1], Bs[:1])
    one = dict(zip(ARG_NAMES, S.args(mode=b"a", info=False)), stride_a=0, stride_b=0, stride_z=0)
    assert gpu_lib.eigx_hgev_batch_dev(*one.values()) == 0
    w, Z, U, info, _ = S.results()
    assert (info == 77).all()
    _gates(As[0], Bs[0], w[0], Z[0], U[0], "one pencil, strides 0, info NULL")
    # ldz and stride_z are ignored in mode 'N'; the timers
    assert gpu_lib.eigx_hgev_batch_dev(*{**dev, "z": None, "ldz": 0, "stride_z": 0, "mode": b"n", "info": None}.values()) == 0
    wn, _, Un, _, _ = P.results(want_z=False)
    assert (wn[0] == w[0]).all() and (Un[0] == U[0]).all()
    t = (C.c_double * 16)()
    gpu_lib.eigx_get_timers(t)
    assert t[0] > 0.0 and all(t[q] == 0.0 for q in range(1, 16))


# ------------------------------------------------------------------------------------------------ 11. two ranks
@pytest.mark.gpu
def test_hgbatch_refuses_several_ranks():
    """two ranks on the one card: both entries return EIGX_ERR_BAD_ARG on both ranks and the processes exit cleanly"""
    import socket

    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = os.path.join(os.path.dirname(__file__), "hgbatch_worker.py")
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


# ------------------------------------------------------------------------------------------------ 12. Fortran
@pytest.mark.gpu
def test_fortran_hgbatch_caller(gpu_lib, tmp_path):
    """a Fortran program calls eigen_hgev_batch of module eigen_libs_mod on four phased-Frank / Gram pencils of n = 30 and
    prints its worst figure in units of each gate"""
    if not os.path.exists(FLANG):
        pytest.skip("no flang")
    lib = os.path.join(ROOT, "eigenexa_amd", "lib")
    mod = os.path.join(ROOT, "eigenexa_amd", "fortran", "eigen_libs_mod.F90")
    src = os.path.join(ROOT, "tests", "fortran", "hgbatch_caller.F90")
    subprocess.check_call([FLANG, "-cpp", "-O2", "-c", mod, "-o", "eigen_libs_mod.o"], cwd=tmp_path)
    subprocess.check_call([FLANG, "-cpp", "-O2", "-c", src, "-o", "hgbatch_caller.o"], cwd=tmp_path)
    subprocess.check_call([FLANG, "-o", "hgbatch_caller", "hgbatch_caller.o", "eigen_libs_mod.o", f"-L{lib}", "-leigenexa_amd",
                           f"-Wl,-rpath,{lib}"], cwd=tmp_path)
    out = subprocess.run([str(tmp_path / "hgbatch_caller")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    for what in ("residual", "B-orthogonality", "factor"):
        m = re.search(what + r" in units of its gate\s*=\s*([0-9.eEdD+-]+)", out.stdout)
        assert m, out.stdout
        assert float(m.group(1).replace("D", "E").replace("d", "e")) < 1.0, out.stdout


# ------------------------------------------------------------------------------------------------ CPU
HGBATCH_HEADER = os.path.join(ROOT, "include", "eigenexa_amd_hgbatch.h")


@pytest.mark.parametrize("name", ENTRIES)
def test_header_prototypes_match_the_ctypes_table(monkeypatch, name):
    """the entries are declared in include/eigenexa_amd_hgbatch.h and mirrored by _lib.HGBATCH_SIGNATURES: the parser of the
    other header tests, pointed at that file"""
    import c_header
    from eigenexa_amd import _lib

    monkeypatch.setattr(c_header, "HEADER", HGBATCH_HEADER)
    params = _prototype(name)
    restype, argtypes = _lib.HGBATCH_SIGNATURES[name]
    assert restype is C.c_int and len(argtypes) == len(params) == 15
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
    assert re.search(r"#define\s+EIGX_HGBATCH_NMAX\s+64\b", open(HGBATCH_HEADER).read())


def test_the_hgbatch_header_is_part_of_the_public_one(monkeypatch):
    """eigenexa_amd.h includes the file, the file declares exactly the entries of the table, no name sits in two tables, and
    the loaded library has them with these signatures"""
    import c_header
    from eigenexa_amd import _lib

    main = open(os.path.join(ROOT, "include", "eigenexa_amd.h")).read()
    assert re.search(r'^#include "eigenexa_amd_hgbatch\.h"$', main, flags=re.M)
    monkeypatch.setattr(c_header, "HEADER", HGBATCH_HEADER)
    protos = c_header.all_prototypes()
    assert set(protos) == set(_lib.HGBATCH_SIGNATURES) == set(ENTRIES)
    assert not set(_lib.HGBATCH_SIGNATURES) & set(_lib.SIGNATURES)
    assert not set(_lib.HGBATCH_SIGNATURES) & set(_lib.GBATCH_SIGNATURES)
    assert not set(_lib.GBATCH_SIGNATURES) & set(_lib.SIGNATURES)
    lib = _lib.load()
    for name, (restype, argtypes) in _lib.HGBATCH_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes


def test_python_wrapper_rejects_bad_arguments_before_the_library(monkeypatch, capsys):
    """every EIGX_ERR_BAD_ARG case of the contract: status -2 and one warning line each, without loading the library"""
    import eigenexa_amd as ee
    from eigenexa_amd import _lib, api

    def boom():
        raise AssertionError("the library must not be touched")

    monkeypatch.setattr(_lib, "load", boom)
    n, nb = 6, 3
    a = np.zeros((n, n, nb), dtype=np.complex128, order="F")
    b = np.zeros((n, n, nb), dtype=np.complex128, order="F")
    z = np.zeros((n, n, nb), dtype=np.complex128, order="F")
    w = np.zeros((n, nb), order="F")
    ok = dict(n=n, batch=nb, a=a, lda=n, b=b, ldb=n, w=w, z=z, ldz=n)
    bad = [dict(n=0), dict(n=-1), dict(batch=-1), dict(lda=n - 1), dict(ldb=n - 1), dict(ldw=n - 1), dict(stride_a=n * n - 1),
           dict(stride_b=n * n - 1), dict(ldz=n - 1), dict(stride_z=n * n - 1), dict(a=None), dict(b=None), dict(w=None),
           dict(z=None), dict(mode="X"), dict(mode="C"), dict(n="x")]
    for change in bad:
        api._state["last_status"] = 0
        ee.eigen_hgev_batch(**{**ok, **change})
        assert api.last_status() == -2, change
        err = capsys.readouterr().err
        assert err.count("\n") == 1 and "eigen_hgev_batch: invalid arguments" in err
    assert "eigen_hgev_batch" in dir(ee)


def test_fortran_module_binds_the_hgbatch_entry():
    src = open(os.path.join(ROOT, "eigenexa_amd", "fortran", "eigen_libs_mod.F90")).read()
    assert 'bind(C, name="eigx_hgev_batch")' in src
    assert re.search(r"public :: eigen_hgev_batch\b", src)
    m = re.search(r"subroutine eigen_hgev_batch\(n, batch, a, lda, b, ldb, w, z, ldz, mode, info\)(.*?)end subroutine eigen_hgev_batch",
                  src, flags=re.S)
    assert m
    assert re.search(r"complex\(8\), intent\(inout\), contiguous :: a\(:, :, :\), b\(:, :, :\)", m.group(1))
    assert re.search(r"real\(8\), intent\(inout\), contiguous :: w\(:, :\)", m.group(1))


def test_tune_key_24_refuses_values_outside_its_range():
    """key 24 (no GPU needed): default 64, takes 0 .. 64; anything else is refused with -1 and changes nothing"""
    from eigenexa_amd import _lib

    lib = _lib.load()
    assert lib.eigx_tune(24, 32) == 64
    assert lib.eigx_tune(24, 65) == -1 and lib.eigx_tune(24, -1) == -1 and lib.eigx_tune(24, 1 << 20) == -1
    assert lib.eigx_tune(24, 0) == 32             # the refused values changed nothing
    assert lib.eigx_tune(24, 64) == 0
    assert lib.eigx_tune(24, 64) == 64
