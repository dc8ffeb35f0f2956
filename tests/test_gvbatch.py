"""Ragged batched generalised eigensolves (eigen_gev_vbatch, an EXTENSION: the reference solves one pencil per call): pencils
A x = lambda B x of differing orders in one call, sorted by n-class on the host (eigx_vbatch_plan), one launch per class, one
workgroup per pencil with both matrices in LDS -- the arithmetic of eigen_gev_batch, bit for bit; blocks above the cutoff
(eigx_tune key 23) go through eigx_gev_range_dev one by one.  GPU tests are marked; the CPU tests at the end check the ctypes
table (_lib.GVBATCH_SIGNATURES) against the header of the entries (include/eigenexa_amd_gvbatch.h), the Python wrappers'
argument checks and the Fortran bindings.

This file also holds what tests/test_hgvbatch.py (eigen_hgev_vbatch) shares with it: the two families (G, HG), the buffers of a
ragged call (RaggedPencils) and the bodies of the GPU tests (check_*), which take the family.  The pencils and the gates are those
of tests/test_gbatch.py / tests/test_hgbatch.py (_mixed, _overlaps, _random_pencils, _gates: eigenvalues against
scipy.linalg.eigh(A, B), residual, B-orthogonality, U^T U - B, positive diagonal of U), imported and unchanged."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_gbatch as tg
import test_hgbatch as thg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLANG = tg.FLANG
GUARD = tg.GUARD
BAD_ARG, NONFINITE, INTERNAL, NOT_SPD = -2, -5, -6, -7
GVBATCH_HEADER = os.path.join(ROOT, "include", "eigenexa_amd_gvbatch.h")
ENTRIES = ["eigx_gev_vbatch", "eigx_gev_vbatch_dev", "eigx_hgev_vbatch", "eigx_hgev_vbatch_dev"]
ARG_NAMES = ["batch", "n", "a", "off_a", "lda", "b", "off_b", "ldb", "w", "off_w", "z", "off_z", "ldz", "mode", "info"]


class Family:
    """what differs between eigen_gev_vbatch and eigen_hgev_vbatch: cs = doubles per element of a, b and z; top = the largest n
    the kernels serve; key = the tune key of the cutoff; sizes = every class edge and the remainders of the substitutions'
    chains; big = the first order above the largest class"""

    def __init__(self, name, cs, top, key, sizes, big, mod):
        self.name, self.cs, self.top, self.key, self.sizes, self.big, self.mod = name, cs, top, key, sizes, big, mod

    def mixed(self, n):
        return self.mod._mixed(n)

    def random(self, n, nb, seed):
        """nb random pencils of order n: (As, Bs), writable"""
        As, Bs = self.mod._random_pencils(n, nb, seed)
        return [np.array(A) for A in As], [np.array(B) for B in Bs]

    def gates(self, A, B, w, Z, U, what, wref=None):
        return self.mod._gates(A, B, w, Z, U, what, wref)

    def vbatch(self, lib, host=False):
        return getattr(lib, f"eigx_{self.name}_vbatch" + ("" if host else "_dev"))

    def uniform(self, lib):
        return getattr(lib, f"eigx_{self.name}_batch_dev")

    def range_dev(self, lib):
        return getattr(lib, f"eigx_{self.name}_range_dev")


G = Family("gev", 1, 96, 23, [1, 2, 3, 5, 17, 32, 33, 64, 65, 95, 96], 97, tg)
HG = Family("hgev", 2, 64, 24, [1, 2, 3, 5, 17, 32, 33, 63, 64], 65, thg)


def _dev():
    import torch

    return torch.device("cuda:0")


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


class RaggedPencils:
    """buffers of one ragged call, on the host (numpy, float64; complex interleaved) and on the device: lda = n + 3,
    ldb = n + 2, ldz = n + 1 (ld: {k: (lda, ldb, ldz)} for other values), offsets with gaps in front of every block; a and b
    hold NaN in the strict lower triangles, the padding rows, the gaps and (HG) the imaginary parts of the diagonals; w, z and
    info are prefilled with guards.  An empty block (0 x 0 matrices) gets offsets inside the gaps.  Offsets and leading
    dimensions count elements."""

    def __init__(self, fam, As, Bs, device=True, ld=None):
        self.fam, self.As, self.Bs = fam, As, Bs
        cs = fam.cs
        self.batch = nb = len(As)
        self.n = np.array([M.shape[0] for M in As], dtype=np.int32).reshape(nb)
        self.lda = (self.n + 3).astype(np.int32)
        self.ldb = (self.n + 2).astype(np.int32)
        self.ldz = (self.n + 1).astype(np.int32)
        for k, v in (ld or {}).items():
            self.lda[k], self.ldb[k], self.ldz[k] = v
        self.off_a, self.off_b, self.off_w, self.off_z = (np.zeros(nb, dtype=np.int64) for _ in range(4))
        ta = tb = tw = tz = 0
        for k in range(nb):
            n = int(self.n[k])
            self.off_a[k], ta = ta + 5, ta + 5 + int(self.lda[k]) * n
            self.off_b[k], tb = tb + 3, tb + 3 + int(self.ldb[k]) * n
            self.off_w[k], tw = tw + 2, tw + 2 + n
            self.off_z[k], tz = tz + 7, tz + 7 + int(self.ldz[k]) * n
        self.len_a, self.len_b, self.len_w, self.len_z = ta + 5, tb + 3, tw + 2, tz + 7
        self.a_host = np.full(cs * self.len_a, np.nan)
        self.b_host = np.full(cs * self.len_b, np.nan)
        self.wmask = np.zeros(self.len_w, dtype=bool)            # what the call may write
        self.zmask = np.zeros((self.len_z, cs), dtype=bool)
        self.bmask = np.zeros((self.len_b, cs), dtype=bool)      # the upper triangles of b
        for k in range(nb):
            n = int(self.n[k])
            if n == 0:
                continue
            upper = np.tri(n, dtype=bool)                         # [j, i]: i <= j
            for buf, off, ldv, M in ((self.a_host, self.off_a, self.lda, As[k]), (self.b_host, self.off_b, self.ldb, Bs[k])):
                v = buf[cs * off[k]:cs * (off[k] + ldv[k] * n)].reshape(n, ldv[k], cs)   # v[j, i] = m(i, j)
                v[:, :n, 0] = np.where(upper, M.T.real, np.nan)
                if cs == 2:
                    v[:, :n, 1] = np.where(upper, M.T.imag, np.nan)
                    v[np.arange(n), np.arange(n), 1] = np.nan
            self.wmask[self.off_w[k]:self.off_w[k] + n] = True
            self.zmask[self.off_z[k]:self.off_z[k] + self.ldz[k] * n].reshape(n, self.ldz[k], cs)[:, :n] = True
            self.bmask[self.off_b[k]:self.off_b[k] + self.ldb[k] * n].reshape(n, self.ldb[k], cs)[:, :n][upper] = True
        self.zmask = self.zmask.reshape(-1)
        self.bmask = self.bmask.reshape(-1)
        self.a_work = self.a_host.copy()                          # a and b of a host call (destroyed / factor)
        self.b_work = self.b_host.copy()
        self.w_host = np.full(self.len_w, GUARD)
        self.z_host = np.full(cs * self.len_z, GUARD)
        self.info_host = np.full(nb, 77, dtype=np.int32)
        if device:
            import torch

            self.a = torch.from_numpy(self.a_host).to(_dev())
            self.b = torch.from_numpy(self.b_host).to(_dev())
            self.w = torch.full((self.len_w,), GUARD, dtype=torch.float64, device=_dev())
            self.z = torch.full((cs * self.len_z,), GUARD, dtype=torch.float64, device=_dev())
            self.info = torch.full((nb,), 77, dtype=torch.int32, device=_dev())

    def refill(self):
        import torch

        self.a.copy_(torch.from_numpy(self.a_host))
        self.b.copy_(torch.from_numpy(self.b_host))
        self.w.fill_(GUARD)
        self.z.fill_(GUARD)
        self.info.fill_(77)

    def args(self, mode=b"A", info=True, z=True, host=False, **change):
        """the argument list of a call; change: name -> value of the arguments to replace"""
        if host:
            self.a_work = self.a_host.copy()
            self.b_work = self.b_host.copy()
            arrays = dict(a=self.a_work.ctypes.data, b=self.b_work.ctypes.data, w=self.w_host.ctypes.data, z=self.z_host.ctypes.data,
                          info=self.info_host.ctypes.data)
        else:
            arrays = dict(a=self.a.data_ptr(), b=self.b.data_ptr(), w=self.w.data_ptr(), z=self.z.data_ptr(), info=self.info.data_ptr())
        g = dict(batch=self.batch, n=self.n, off_a=self.off_a, lda=self.lda, off_b=self.off_b, ldb=self.ldb, off_w=self.off_w,
                 off_z=self.off_z, ldz=self.ldz, mode=mode, **arrays)
        if not z:
            g["z"] = g["off_z"] = g["ldz"] = None
        if not info:
            g["info"] = None
        g.update(change)
        self.keep = [np.ascontiguousarray(v) for v in g.values() if isinstance(v, np.ndarray)]   # alive during the call
        return [g[name].ctypes.data if isinstance(g[name], np.ndarray) else g[name] for name in ARG_NAMES]

    def run(self, lib, mode=b"A", info=True, z=True, host=False, **change):
        return self.fam.vbatch(lib, host)(*self.args(mode, info, z, host, **change))

    def images(self, host=False):
        """(w, z, b, info) as numpy arrays, whole buffers"""
        if host:
            return self.w_host, self.z_host, self.b_work, self.info_host
        return self.w.cpu().numpy(), self.z.cpu().numpy(), self.b.cpu().numpy(), self.info.cpu().numpy()

    def block_ptrs(self, k):
        """addresses of block k of the device a, b, w and z"""
        cs = self.fam.cs
        return (self.a.data_ptr() + 8 * cs * int(self.off_a[k]), self.b.data_ptr() + 8 * cs * int(self.off_b[k]),
                self.w.data_ptr() + 8 * int(self.off_w[k]), self.z.data_ptr() + 8 * cs * int(self.off_z[k]))

    def b_as_passed(self, k, host=False):
        """is the block of b (its padding rows included) as it was passed?"""
        cs, n = self.fam.cs, int(self.n[k])
        sl = slice(cs * self.off_b[k], cs * (self.off_b[k] + self.ldb[k] * n))
        return np.array_equal(_bits(self.images(host)[2][sl]), _bits(self.b_host[sl]))

    def results(self, want_z=True, host=False, untouched=(), by_range=()):
        """per block: w (n), Z (n, n) with Z[:, j] the j-th eigenvector, U (n, n) upper triangular; info; asserts that every
        guard outside w(1:n_k) and z(1:n_k, 1:n_k) survived, that b outside the upper triangles is as it was passed (NaN), and
        (want_z false, or k in untouched) the guards of z inside too.  by_range: the real blocks that went through
        eigx_gev_range_dev, which owns the strict lower triangle of its b (tests/test_gbatch.py holds it to the padding rows and
        the gaps only)"""
        cs = self.fam.cs
        wb, zb, bb, info = self.images(host)
        assert (wb[~self.wmask] == GUARD).all(), "w outside the blocks was touched"
        assert (zb[~self.zmask] == GUARD).all(), "z outside the blocks (padding rows, gaps) was touched"
        held = ~self.bmask
        if cs == 1:
            for k in by_range:
                n = int(self.n[k])
                held[self.off_b[k]:self.off_b[k] + self.ldb[k] * n].reshape(n, self.ldb[k])[:, :n] = False
        assert np.isnan(bb[held]).all(), "b outside the upper triangles (lower triangles, padding rows, gaps) was touched"
        if not want_z:
            assert (zb == GUARD).all(), "z was touched"
        ws, Zs, Us = [], [], []
        for k in range(self.batch):
            n = int(self.n[k])
            ws.append(wb[self.off_w[k]:self.off_w[k] + n].copy())
            zz = zb[cs * self.off_z[k]:cs * (self.off_z[k] + self.ldz[k] * n)].reshape(n, self.ldz[k], cs)[:, :n]
            if k in untouched:
                assert (zz == GUARD).all(), f"z of block {k} was touched"
            Zs.append((zz[:, :, 0] + (1j * zz[:, :, 1] if cs == 2 else 0.0)).T.copy())
            uu = np.nan_to_num(bb[cs * self.off_b[k]:cs * (self.off_b[k] + self.ldb[k] * n)].reshape(n, self.ldb[k], cs)[:, :n], nan=0.0)
            Us.append(np.triu((uu[:, :, 0] + (1j * uu[:, :, 1] if cs == 2 else 0.0)).T))
        return ws, Zs, Us, info.copy()


def solve_blocks_alone(lib, R):
    """every block of R solved on its own, in place in R's device buffers, by eigx_*_batch_dev(n_k, 1, ...)"""
    fam = R.fam
    for k in range(R.batch):
        n = int(R.n[k])
        if n == 0:
            continue
        pa, pb, pw, pz = R.block_ptrs(k)
        assert fam.uniform(lib)(n, 1, pa, int(R.lda[k]), 0, pb, int(R.ldb[k]), 0, pw, n, pz, int(R.ldz[k]), 0, b"A", None) == 0, k


def same_bits(R1, R2):
    """w, z and b of two calls on the same layout agree bit for bit, whole buffers (the guards and the NaN included)"""
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(R1.images()[:3], R2.images()[:3]))


def same_block(r1, k1, r2, k2):
    """w, Z and U of block k1 of the results r1 and of block k2 of r2 agree exactly"""
    return all(np.array_equal(r1[q][k1], r2[q][k2]) for q in range(3))


_MIXED = {}


def mixed_pencils(fam):
    """three pencils of fam.mixed(n) per size of fam.sizes -- number 3 i + j of size number i, so every family of A and every
    overlap occurs -- in a shuffled order; computed once and left unchanged"""
    if fam.name not in _MIXED:
        As, Bs = [], []
        for i, n in enumerate(fam.sizes):
            fa, fb = fam.mixed(n)
            for j in range(3):
                As.append(fa[(3 * i + j) % len(fa)])
                Bs.append(fb[(3 * i + j) % len(fa)])
        order = np.random.default_rng(11).permutation(len(As))
        _MIXED[fam.name] = ([As[q] for q in order], [Bs[q] for q in order])
    return _MIXED[fam.name]


def diag_im_is_zero(R, host=False):
    """HG: the imaginary parts of the diagonals of U are written as exactly 0"""
    bb = R.images(host)[2]
    for k in range(R.batch):
        n = int(R.n[k])
        v = bb[2 * R.off_b[k]:2 * (R.off_b[k] + R.ldb[k] * n)].reshape(n, R.ldb[k], 2)
        if not (v[np.arange(n), np.arange(n), 1] == 0.0).all():
            return False
    return True


# ------------------------------------------------------------------------------------------------ 1. ragged mixed call
def check_mixed(lib, fam):
    As, Bs = mixed_pencils(fam)
    R = RaggedPencils(fam, As, Bs)
    assert R.run(lib) == 0
    ws, Zs, Us, info = R.results()
    assert (info == 0).all()
    if fam.cs == 2:
        assert diag_im_is_zero(R)
    for k in range(R.batch):
        fam.gates(As[k], Bs[k], ws[k], Zs[k], Us[k], f"{fam.name}: block {k} n={As[k].shape[0]}")


@pytest.mark.gpu
def test_ragged_mixed_call(gpu_lib):
    check_mixed(gpu_lib, G)


# ------------------------------------------------------------------------------------------------ 2. bit identity
def check_bits(lib, fam):
    """every block of the mixed call against eigx_*_batch_dev(n_k, 1, ...) on a copy: the whole w, z and b buffers; the same
    call twice; the same call with the blocks in reversed order"""
    As, Bs = mixed_pencils(fam)
    R = RaggedPencils(fam, As, Bs)
    assert R.run(lib) == 0
    alone = RaggedPencils(fam, As, Bs)
    solve_blocks_alone(lib, alone)
    assert same_bits(R, alone), "a block differs from the uniform entry's solve of it"
    again = RaggedPencils(fam, As, Bs)
    assert again.run(lib) == 0
    assert same_bits(R, again), "two runs differ"
    res = R.results()
    rev = RaggedPencils(fam, As[::-1], Bs[::-1])
    assert rev.run(lib) == 0
    rres = rev.results()
    nb = len(As)
    for k in range(nb):
        assert same_block(res, k, rres, nb - 1 - k), f"block {k} depends on the order"


@pytest.mark.gpu
def test_bit_identity_with_the_uniform_entry(gpu_lib):
    check_bits(gpu_lib, G)


# ------------------------------------------------------------------------------------------------ 2b. two entries, one result
def _solo(lib, X, k, code):
    """block k of X by eigx_*_batch_dev(n_k, 1, ...) with its own status word: the call returns `code`"""
    n = int(X.n[k])
    pa, pb, pw, pz = X.block_ptrs(k)
    rc = X.fam.uniform(lib)(n, 1, pa, int(X.lda[k]), 0, pb, int(X.ldb[k]), 0, pw, n, pz, int(X.ldz[k]), 0, b"A", X.info.data_ptr() + 4 * k)
    assert rc == code, (k, rc)


def _check_good_and_failed(X, As, Bs, codes):
    """the gates on the good blocks of X; w = NaN, the status and an untouched z for the failed ones"""
    import scipy.linalg

    failed = [k for k, c in enumerate(codes) if c]
    ws, Zs, Us, info = X.results(untouched=failed)
    assert info.tolist() == codes
    for k, c in enumerate(codes):
        if c:
            assert np.isnan(ws[k]).all(), k
        else:
            X.fam.gates(As[k], Bs[k], ws[k], Zs[k], Us[k], f"{X.fam.name}: block {k} n={As[k].shape[0]}",
                        wref=scipy.linalg.eigh(As[k], Bs[k], eigvals_only=True))


def check_edges_with_failed_blocks(lib, fam):
    """The uniform and the ragged entry promise the same bits, failures included (eigen_hgev: they are one kernel, csrc/hgbatch.hip).
    One pencil at n = 1, 2 and on both sides of every n-class edge the
    kernels reach, a block with a NaN in A and a block whose B is not positive definite, each between two good ones: w, z, b
    and info of the ragged call against eigx_*_batch_dev(n_k, 1, ...) with info, bit for bit, whole buffers"""
    sizes = [n for n in (1, 2, 32, 33, 64, 65, 96) if n <= fam.top]
    pairs = [fam.random(n, 1, 200 + n) for n in sizes]
    As, Bs = [p[0][0] for p in pairs], [p[1][0] for p in pairs]
    nanA, goodB = (x[0] for x in fam.random(40, 1, 7))
    nanA[3, 30] = nanA[30, 3] = np.nan
    goodA, indefB = (x[0] for x in fam.random(20, 1, 8))
    indefB[10, 10] = -1.0
    As[3:3], Bs[3:3] = [nanA], [goodB]                              # between the blocks of n = 32 and n = 33
    As[5:5], Bs[5:5] = [goodA], [indefB]                            # between the blocks of n = 33 and n = 64
    codes = [0] * len(As)
    codes[3], codes[5] = NONFINITE, NOT_SPD
    R = RaggedPencils(fam, As, Bs)
    assert R.run(lib) == NONFINITE                                  # the failed block with the lowest caller index
    alone = RaggedPencils(fam, As, Bs)
    for k in range(len(As)):
        _solo(lib, alone, k, codes[k])
    assert same_bits(R, alone), "a block differs from the uniform entry's solve of it"
    for X in (R, alone):
        _check_good_and_failed(X, As, Bs, codes)


@pytest.mark.gpu
def test_ragged_equals_uniform_at_the_class_edges_with_failed_blocks(gpu_lib):
    check_edges_with_failed_blocks(gpu_lib, G)


def check_uniform_failed_middle(lib, fam):
    """The uniform entry, one n per class and both kinds of failure (a NaN in A, a B that is not positive definite): a batch of
    three whose middle pencil fails leaves w, z, b and info of its neighbours as their solo calls (batch = 1) leave them, bit for
    bit, and the failed pencil as its solo call leaves it.  (Three blocks of one order in the buffers of a ragged call are evenly
    spaced: a uniform batch with those strides.)"""
    for n in [n for n in (5, 33, 65) if n <= fam.top]:
        for code in (NONFINITE, NOT_SPD):
            As, Bs = fam.random(n, 3, 300 + n)
            if code == NONFINITE:
                As[1][0, n - 1] = As[1][n - 1, 0] = np.nan
            else:
                Bs[1][n // 2, n // 2] = -1.0
            codes = [0, code, 0]
            T, solo = RaggedPencils(fam, As, Bs), RaggedPencils(fam, As, Bs)
            offs = (T.off_a, T.off_b, T.off_w, T.off_z)
            steps = [int(v[1] - v[0]) for v in offs]
            assert all(int(v[2] - v[1]) == s for v, s in zip(offs, steps))
            pa, pb, pw, pz = T.block_ptrs(0)
            rc = fam.uniform(lib)(n, 3, pa, int(T.lda[0]), steps[0], pb, int(T.ldb[0]), steps[1], pw, steps[2], pz, int(T.ldz[0]), steps[3],
                                  b"A", T.info.data_ptr())
            assert rc == code
            for k in range(3):
                _solo(lib, solo, k, codes[k])
            assert same_bits(T, solo), f"n={n}, code {code}: a pencil beside a failed one differs from its solo result"
            _check_good_and_failed(T, As, Bs, codes)
            assert np.array_equal(T.images()[3], solo.images()[3])


@pytest.mark.gpu
def test_uniform_failed_pencil_leaves_its_neighbours(gpu_lib):
    check_uniform_failed_middle(gpu_lib, G)


# ------------------------------------------------------------------------------------------------ 3. many workgroups
def check_many(lib, fam):
    """1500 pencils with n drawn from 1 .. 24 and three of n = 40 (two classes, more workgroups than the card holds): info all
    zero, the gates on a sample of 200 (the three of n = 40 among them)"""
    import scipy.linalg

    rng = np.random.default_rng(5)
    sizes = rng.integers(1, 25, 1500)
    sizes[[3, 700, 1499]] = 40
    As, Bs = [None] * 1500, [None] * 1500
    for n in np.unique(sizes):
        where = np.flatnonzero(sizes == n)
        pa, pb = fam.mod._random_pencils(int(n), len(where), 300 + int(n))
        for q, k in enumerate(where):
            As[k], Bs[k] = pa[q], pb[q]
    R = RaggedPencils(fam, As, Bs)
    assert R.run(lib) == 0
    ws, Zs, Us, info = R.results()
    assert (info == 0).all()
    sample = sorted(set(rng.choice(1500, 197, replace=False).tolist()) | {3, 700, 1499})
    for k in sample:
        fam.gates(As[k], Bs[k], ws[k], Zs[k], Us[k], f"{fam.name}: block {k} n={sizes[k]}",
                  wref=scipy.linalg.eigh(As[k], Bs[k], eigvals_only=True))


@pytest.mark.gpu
def test_more_workgroups_than_the_card_holds(gpu_lib):
    check_many(gpu_lib, G)


# ------------------------------------------------------------------------------------------------ 4. mode 'N'
def check_mode_n(lib, fam):
    As, Bs = mixed_pencils(fam)
    R = RaggedPencils(fam, As, Bs)
    assert R.run(lib) == 0
    wa, _, ba, _ = R.images()
    for z in (True, False):                                        # z, off_z, ldz passed, then all three NULL
        R.refill()
        assert R.run(lib, mode=b"N", z=z) == 0
        wn, _, bn, info = R.images()
        R.results(want_z=False)
        assert (info == 0).all()
        assert np.array_equal(_bits(wn), _bits(wa)), "w of mode 'N' differs from mode 'A'"
        assert np.array_equal(_bits(bn), _bits(ba)), "U of mode 'N' differs from mode 'A'"


@pytest.mark.gpu
def test_mode_n(gpu_lib):
    check_mode_n(gpu_lib, G)


# ------------------------------------------------------------------------------------------------ 5. failures are local
def failing_pencils(fam, reverse=False):
    """good pencils of several classes, and the same with a NaN in A at the first, an Inf in B at a middle and B = -I at the last
    position (HG: the NaN in a real part, the Inf in an imaginary part); reverse: the whole list the other way round, so that the
    indefinite B comes first.  (good As, good Bs, As, Bs, codes)"""
    sizes = [12, 70, 90, 33, 5, 40] if fam.cs == 1 else [12, 40, 60, 33, 5, 20]
    good = [fam.random(n, 1, 60 + k) for k, n in enumerate(sizes)]
    gA, gB = [p[0][0] for p in good], [p[1][0] for p in good]
    As, Bs = [A.copy() for A in gA], [B.copy() for B in gB]
    As[0][4, 9] = As[0][9, 4] = np.nan
    m = sizes[2]
    if fam.cs == 1:
        Bs[2][0, m - 1] = Bs[2][m - 1, 0] = np.inf
    else:
        Bs[2][0, m - 1] = complex(1.0, np.inf)
        Bs[2][m - 1, 0] = complex(1.0, -np.inf)
    Bs[5] = -np.eye(sizes[5], dtype=Bs[5].dtype)
    codes = [NONFINITE, 0, NONFINITE, 0, 0, NOT_SPD]
    if reverse:
        gA, gB, As, Bs, codes = gA[::-1], gB[::-1], As[::-1], Bs[::-1], codes[::-1]
    return gA, gB, As, Bs, codes


def check_failures(lib, fam):
    for reverse in (False, True):
        gA, gB, As, Bs, codes = failing_pencils(fam, reverse)
        failed = [k for k, c in enumerate(codes) if c]
        clean = RaggedPencils(fam, gA, gB)
        assert clean.run(lib) == 0
        cres = clean.results()
        R = RaggedPencils(fam, As, Bs)
        for with_info in (True, False):
            R.refill()
            assert R.run(lib, info=with_info) == codes[failed[0]]      # the failed block with the lowest caller index
            res = R.results(untouched=failed)
            assert res[3].tolist() == (codes if with_info else [77] * len(codes))
            for k, c in enumerate(codes):
                if c:
                    assert np.isnan(res[0][k]).all(), k
                    if c == NONFINITE or fam.cs == 2:
                        assert R.b_as_passed(k), f"b of the failed block {k} was written"
                else:
                    assert same_block(res, k, cres, k), f"block {k} beside failed ones differs from the clean run"


@pytest.mark.gpu
def test_failures_are_local(gpu_lib):
    check_failures(gpu_lib, G)


# ------------------------------------------------------------------------------------------------ 6. above the cutoff
def _even(x):
    return x + (x & 1)


def range_reference(lib, fam, A, B, lds):
    """eigx_*_range_dev(n, 1, n, ...) on the pencil alone with the leading dimensions lds (real: an odd one rounded up to even,
    what the caller's loop of tests/test_gbatch.py does): its (w, Z, U) and status"""
    if fam.cs == 1:
        lds = tuple(_even(int(v)) for v in lds)
    L = RaggedPencils(fam, [A], [B], ld={0: lds})
    pa, pb, pw, pz = L.block_ptrs(0)
    n = A.shape[0]
    rc = fam.range_dev(lib)(n, 1, n, pa, int(L.lda[0]), pb, int(L.ldb[0]), pw, pz, int(L.ldz[0]), b"A")
    ws, Zs, Us, _ = L.results(by_range=[0])
    return rc, (ws, Zs, Us)


def check_above_cutoff(lib, fam):
    # default cutoff: one block of the first order above the largest class among small ones, with odd and with even lds
    sizes = [5, 33, fam.big, 17]
    pairs = [fam.random(n, 1, 90 + k) for k, n in enumerate(sizes)]
    As, Bs = [p[0][0] for p in pairs], [p[1][0] for p in pairs]
    small = RaggedPencils(fam, As[:2] + As[3:], Bs[:2] + Bs[3:])
    assert small.run(lib) == 0
    sres = small.results()
    m = fam.big
    for lds in ((m + 3, m + 5, m + 1), (m + 2, m + 4, m + 6)):
        assert len({v & 1 for v in lds}) == 1
        R = RaggedPencils(fam, As, Bs, ld={2: lds})
        assert R.run(lib) == 0
        res = R.results(by_range=[2])
        assert (res[3] == 0).all()
        rc, ref = range_reference(lib, fam, As[2], Bs[2], lds)
        assert rc == 0 and same_block(res, 2, ref, 0), f"lds {lds}: the block above the cutoff is not the range entry's"
        for k, ks in ((0, 0), (1, 1), (3, 2)):
            assert same_block(res, k, sres, ks), f"lds {lds}: block {k} differs from the run without the large one"
        for k in range(4):
            fam.gates(As[k], Bs[k], res[0][k], res[1][k], res[2][k], f"{fam.name}: default cutoff, lds {lds}, block {k}")
    # key = 32: the block of n = 40 goes through the range entry, the others through the kernel as before; then the same with an
    # indefinite B in that block: its own status, the others untouched by it
    sizes = [5, 40, 20, 32]
    pairs = [fam.random(n, 1, 95 + k) for k, n in enumerate(sizes)]
    As, Bs = [p[0][0] for p in pairs], [p[1][0] for p in pairs]
    small = RaggedPencils(fam, As, Bs)
    assert small.run(lib) == 0                                      # (default cutoff: every block by the kernel)
    sres = small.results()
    R = RaggedPencils(fam, As, Bs)
    Bbad = list(Bs)
    Bbad[1] = -np.eye(40, dtype=Bs[1].dtype)
    F = RaggedPencils(fam, As, Bbad)
    old = lib.eigx_tune(fam.key, 32)
    try:
        assert old == fam.top
        assert R.run(lib) == 0
        rc, ref = range_reference(lib, fam, As[1], Bs[1], (43, 42, 41))
        rcf = F.run(lib)
    finally:
        assert lib.eigx_tune(fam.key, old) == 32
    res = R.results(by_range=[1])
    assert (res[3] == 0).all()
    assert rc == 0 and same_block(res, 1, ref, 0), "key = 32: the block of n = 40 is not the range entry's"
    fres = F.results(by_range=[1])                                  # (w, z and b of that block: as the range entry leaves them)
    assert rcf == NOT_SPD and fres[3].tolist() == [0, NOT_SPD, 0, 0]
    for k in (0, 2, 3):
        assert same_block(res, k, sres, k) and same_block(fres, k, sres, k), k
    for k in range(4):
        fam.gates(As[k], Bs[k], res[0][k], res[1][k], res[2][k], f"{fam.name}: key {fam.key} = 32, block {k}")


@pytest.mark.gpu
def test_above_the_cutoff(gpu_lib):
    check_above_cutoff(gpu_lib, G)


# ------------------------------------------------------------------------------------------------ 7. empty blocks
def check_empty(lib, fam):
    dt = np.float64 if fam.cs == 1 else np.complex128
    none = np.zeros((0, 0), dtype=dt)
    (A5,), (B5,) = fam.random(5, 1, 1)
    (A33,), (B33,) = fam.random(33, 1, 2)
    As, Bs = [none, A5, none, A33, none], [none, B5, none, B33, none]
    R = RaggedPencils(fam, As, Bs)
    assert R.run(lib) == 0
    ws, Zs, Us, info = R.results()
    assert (info == 0).all()
    for k in (1, 3):
        fam.gates(As[k], Bs[k], ws[k], Zs[k], Us[k], f"{fam.name}: block {k} between empty ones")
    E = RaggedPencils(fam, [none, none], [none, none])              # nothing but empty blocks
    assert E.run(lib) == 0
    assert (E.results(want_z=False)[3] == 0).all()
    R.refill()                                                      # batch = 0: nothing is touched
    assert R.run(lib, batch=0) == 0
    assert fam.vbatch(lib)(0, *([None] * 12), b"A", None) == 0
    assert fam.vbatch(lib, host=True)(0, *([None] * 12), b"A", None) == 0
    info = R.results(want_z=False)[3]
    assert (R.w.cpu().numpy() == GUARD).all() and (info == 77).all()
    assert np.array_equal(_bits(R.b.cpu().numpy()), _bits(R.b_host))


@pytest.mark.gpu
def test_empty_blocks(gpu_lib):
    check_empty(gpu_lib, G)


# ------------------------------------------------------------------------------------------------ 8. forms and refusals
def check_host_form(lib, fam):
    """w, z, b and info of the host form are those of the device form, bit for bit, every guard, every NaN of b and the z and
    b of the failed blocks included"""
    _, _, As, Bs, codes = failing_pencils(fam)
    failed = [k for k, c in enumerate(codes) if c]
    R = RaggedPencils(fam, As, Bs)
    assert R.run(lib) == NONFINITE
    wd, zd, bd, idv = R.images()
    assert R.run(lib, host=True) == NONFINITE
    wh, zh, bh, ih = R.images(host=True)
    R.results(host=True, untouched=failed)
    assert np.array_equal(_bits(wh), _bits(wd)) and np.array_equal(_bits(zh), _bits(zd)) and np.array_equal(_bits(bh), _bits(bd))
    assert np.array_equal(ih, idv)
    for k in failed:
        assert R.b_as_passed(k, host=True), f"b of the failed block {k} did not return as passed"
    # mode 'N' with z, off_z, ldz = NULL and info = NULL
    R.w_host[:] = GUARD
    R.z_host[:] = GUARD
    R.info_host[:] = 77
    assert R.run(lib, mode=b"N", z=False, info=False, host=True) == NONFINITE
    assert np.array_equal(_bits(R.w_host), _bits(wd)) and np.array_equal(_bits(R.b_work), _bits(bd))
    assert (R.z_host == GUARD).all() and (R.info_host == 77).all()


@pytest.mark.gpu
def test_host_and_device_forms_agree(gpu_lib):
    check_host_form(gpu_lib, G)


def check_arguments(lib, fam):
    pairs = [fam.random(n, 1, n) for n in (12, 7, 30)]
    As, Bs = [p[0][0] for p in pairs], [p[1][0] for p in pairs]
    R = RaggedPencils(fam, As, Bs)

    def at(v, k, x):
        v = v.copy()
        v[k] = x
        return v

    bad = [dict(batch=-1), dict(n=None), dict(a=None), dict(off_a=None), dict(lda=None), dict(b=None), dict(off_b=None),
           dict(ldb=None), dict(w=None), dict(off_w=None), dict(z=None), dict(off_z=None), dict(ldz=None), dict(mode=b"X"),
           dict(mode=b"S"), dict(mode=b"C"), dict(mode=b"V"), dict(n=at(R.n, 1, -1)), dict(lda=at(R.lda, 2, 29)),
           dict(ldb=at(R.ldb, 2, 29)), dict(off_a=at(R.off_a, 0, -1)), dict(off_b=at(R.off_b, 1, -1)), dict(off_w=at(R.off_w, 1, -1)),
           dict(off_z=at(R.off_z, 2, -1)), dict(ldz=at(R.ldz, 0, 11)),
           dict(mode=b"N", b=None), dict(mode=b"N", off_b=None), dict(mode=b"N", ldb=None), dict(mode=b"N", ldb=at(R.ldb, 0, 11))]
    for host in (False, True):
        for change in bad:
            assert R.run(lib, host=host, **change) == BAD_ARG, (host, list(change))
        assert np.array_equal(_bits(R.a_work), _bits(R.a_host)) and np.array_equal(_bits(R.b_work), _bits(R.b_host))
    for host in (False, True):                                      # nothing was touched
        wb, zb, _, info = R.images(host)
        assert (wb == GUARD).all() and (zb == GUARD).all() and (info == 77).all()
    assert np.array_equal(_bits(R.a.cpu().numpy()), _bits(R.a_host)) and np.array_equal(_bits(R.b.cpu().numpy()), _bits(R.b_host))
    # mode 'N' does not look at ldz and off_z; lower-case mode
    assert R.run(lib, mode=b"n", ldz=at(R.ldz, 0, 0), off_z=at(R.off_z, 0, -5)) == 0
    ws, _, Us, info = R.results(want_z=False)
    assert (info == 0).all()
    for k in range(3):
        fam.gates(As[k], Bs[k], ws[k], None, Us[k], f"{fam.name}: mode n, block {k}")
    t = (C.c_double * 16)()
    lib.eigx_get_timers(t)
    assert t[0] > 0.0 and all(t[q] == 0.0 for q in range(1, 16))
    R.refill()
    assert R.run(lib, mode=b"a", info=False) == 0
    ws, Zs, Us, info = R.results()
    assert (info == 77).all()
    for k in range(3):
        fam.gates(As[k], Bs[k], ws[k], Zs[k], Us[k], f"{fam.name}: mode a, info NULL, block {k}")


@pytest.mark.gpu
def test_arguments_and_timers(gpu_lib):
    check_arguments(gpu_lib, G)


@pytest.mark.gpu
def test_gvbatch_refuses_several_ranks():
    """two ranks on the one card: the entries of both families return EIGX_ERR_BAD_ARG on both ranks and the processes exit
    cleanly"""
    import socket

    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = os.path.join(os.path.dirname(__file__), "gvbatch_worker.py")
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


# ------------------------------------------------------------------------------------------------ 9. Fortran
def run_fortran_caller(tmp_path, name):
    """build tests/fortran/<name>.F90 against the module and run it: its worst figures in units of each gate stay below 1"""
    lib = os.path.join(ROOT, "eigenexa_amd", "lib")
    mod = os.path.join(ROOT, "eigenexa_amd", "fortran", "eigen_libs_mod.F90")
    src = os.path.join(ROOT, "tests", "fortran", name + ".F90")
    subprocess.check_call([FLANG, "-cpp", "-O2", "-c", mod, "-o", "eigen_libs_mod.o"], cwd=tmp_path)
    subprocess.check_call([FLANG, "-cpp", "-O2", "-c", src, "-o", name + ".o"], cwd=tmp_path)
    subprocess.check_call([FLANG, "-o", name, name + ".o", "eigen_libs_mod.o", f"-L{lib}", "-leigenexa_amd", f"-Wl,-rpath,{lib}"],
                          cwd=tmp_path)
    out = subprocess.run([str(tmp_path / name)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    for what in ("residual", "B-orthogonality", "factor"):
        m = re.search(what + r" in units of its gate\s*=\s*([0-9.eEdD+-]+)", out.stdout)
        assert m, out.stdout
        assert float(m.group(1).replace("D", "E").replace("d", "e")) < 1.0, out.stdout


@pytest.mark.gpu
def test_fortran_gvbatch_caller(gpu_lib, tmp_path):
    """a Fortran program calls eigen_gev_vbatch of module eigen_libs_mod on Frank / diagonally dominant pencils of the orders 7,
    30, 70 and 12 held in flat arrays with 1-based start indices"""
    if not os.path.exists(FLANG):
        pytest.skip("no flang")
    run_fortran_caller(tmp_path, "gvbatch_caller")


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", ENTRIES)
def test_header_prototypes_match_the_ctypes_table(monkeypatch, name):
    """the entries are declared in include/eigenexa_amd_gvbatch.h and mirrored by _lib.GVBATCH_SIGNATURES: the parser of the
    other header tests, pointed at that file"""
    import c_header
    from eigenexa_amd import _lib

    monkeypatch.setattr(c_header, "HEADER", GVBATCH_HEADER)
    params = c_header.prototype(name)
    restype, argtypes = _lib.GVBATCH_SIGNATURES[name]
    assert restype is C.c_int and len(argtypes) == len(params) == 15
    for p, t in zip(params, argtypes):
        if p.startswith("char "):
            assert t is C.c_char
        elif "*" in p:
            assert t is C.c_void_p
        else:
            assert p.startswith("int ") and t is C.c_int
    assert [p.split()[-1].replace("_dev", "") for p in params] == ARG_NAMES
    for p in params:                                                # the descriptors: const int* / const int64_t*
        if p.split()[-1] in ("n", "lda", "ldb", "ldz"):
            assert p.startswith("const int*")
        if p.split()[-1].startswith("off_"):
            assert p.startswith("const int64_t*")


def test_the_gvbatch_header_is_part_of_the_public_one(monkeypatch):
    """eigenexa_amd.h includes the file, the file declares exactly the entries of the table, no name sits in two tables, and
    the loaded library has them with these signatures"""
    import c_header
    from eigenexa_amd import _lib

    main = open(os.path.join(ROOT, "include", "eigenexa_amd.h")).read()
    assert re.search(r'^#include "eigenexa_amd_gvbatch\.h"$', main, flags=re.M)
    monkeypatch.setattr(c_header, "HEADER", GVBATCH_HEADER)
    protos = c_header.all_prototypes()
    assert set(protos) == set(_lib.GVBATCH_SIGNATURES) == set(ENTRIES)
    tables = [_lib.SIGNATURES, _lib.GBATCH_SIGNATURES, _lib.HGBATCH_SIGNATURES, _lib.VBATCH_SIGNATURES, _lib.GVBATCH_SIGNATURES,
              _lib.LAB_SIGNATURES]
    for i, t1 in enumerate(tables):
        for t2 in tables[i + 1:]:
            assert not set(t1) & set(t2)
    lib = _lib.load()
    for name, (restype, argtypes) in _lib.GVBATCH_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes


def wrapper_refusals(name, dtype, monkeypatch, capsys):
    """every EIGX_ERR_BAD_ARG case of the contract: status -2 and one warning line each, without loading the library"""
    import eigenexa_amd as ee
    from eigenexa_amd import _lib, api, layout

    def boom():
        raise AssertionError("the library must not be touched")

    monkeypatch.setattr(_lib, "load", boom)
    n = [4, 0, 6]
    off_a, la = layout.ragged_offsets(n)
    off_w, lw = layout.ragged_offsets(n, ld=1)
    ok = dict(batch=3, n=n, a=np.zeros(la, dtype=dtype), off_a=off_a, lda=n, b=np.zeros(la, dtype=dtype), off_b=off_a, ldb=n,
              w=np.zeros(lw), off_w=off_w, z=np.zeros(la, dtype=dtype), off_z=off_a, ldz=n)
    bad = [dict(batch=-1), dict(batch="x"), dict(n=None), dict(a=None), dict(off_a=None), dict(lda=None), dict(b=None),
           dict(off_b=None), dict(ldb=None), dict(w=None), dict(off_w=None), dict(z=None), dict(off_z=None), dict(ldz=None),
           dict(mode="X"), dict(mode="C"), dict(n=[4, -1, 6]), dict(lda=[3, 0, 6]), dict(ldb=[4, 0, 5]), dict(off_a=[0, -1, 16]),
           dict(off_b=[0, 16, -16]), dict(off_w=[-1, 4, 4]), dict(off_z=[0, 16, -16]), dict(ldz=[4, 0, 5]), dict(n=[4, 0]),
           dict(ldb=[4, 0, 6, 6]), dict(n=[4.5, 0.0, 6.0]), dict(off_b="abc"),
           dict(mode="N", b=None), dict(mode="N", off_b=None), dict(mode="N", ldb=None), dict(mode="N", ldb=[3, 0, 6])]
    fn = getattr(ee, name)
    for change in bad:
        api._state["last_status"] = 0
        fn(**{**ok, **change})
        assert api.last_status() == -2, change
        err = capsys.readouterr().err
        assert err.count("\n") == 1 and f"{name}: invalid arguments" in err, change
    assert name in dir(ee)
    assert "layout.ragged_offsets" in fn.__doc__


def test_python_wrapper_rejects_bad_arguments_before_the_library(monkeypatch, capsys):
    wrapper_refusals("eigen_gev_vbatch", np.float64, monkeypatch, capsys)


def test_fortran_module_binds_the_gvbatch_entries():
    src = open(os.path.join(ROOT, "eigenexa_amd", "fortran", "eigen_libs_mod.F90")).read()
    for which, kind in (("gev", r"real\(8\)"), ("hgev", r"complex\(8\)")):
        assert f'bind(C, name="eigx_{which}_vbatch")' in src
        assert re.search(rf"public :: eigen_{which}_vbatch\b", src)
        m = re.search(rf"subroutine eigen_{which}_vbatch\(batch, n, a, ia, lda, b, ib, ldb, w, iw, z, iz, ldz, mode, info\)(.*?)"
                      rf"end subroutine eigen_{which}_vbatch", src, flags=re.S)
        assert m
        body = m.group(1)
        assert re.search(kind + r", intent\(inout\), contiguous :: a\(:\), b\(:\)", body)
        assert re.search(r"integer\(8\), intent\(in\) :: ia\(\*\), ib\(\*\), iw\(\*\), iz\(\*\)", body)
        assert re.search(r"character\(\*\), intent\(in\), optional :: mode", body)
        assert re.search(r"integer, intent\(out\), optional :: info\(\*\)", body)
        # the 1-based start indices become 0-based offsets
        for i, o in (("ia", "off_a"), ("ib", "off_b"), ("iw", "off_w"), ("iz", "off_z")):
            assert re.search(rf"{o} = {i}\(1:nb\) - 1", body)
        assert re.search(rf"eigx_{which}_vbatch\(batch, n, a, off_a, lda, b, off_b, ldb, w, off_w, z, off_z, ldz, md, info\)", body)
