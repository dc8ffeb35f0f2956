"""Ragged batched symmetric eigensolves (eigen_s_vbatch, an EXTENSION: the reference solves one matrix per call): blocks of
differing orders in one call, sorted by n-class on the host (eigx_vbatch_plan), one launch per class, one workgroup per block
with the block in LDS -- the arithmetic of eigen_s_batch, bit for bit; blocks above the cutoff (eigx_tune key 21) go through
eigen_s one by one.  GPU tests are marked; the CPU tests at the end check the ctypes table (_lib.VBATCH_SIGNATURES) against the
header of the entries (include/eigenexa_amd_vbatch.h), the schedule against a numpy restatement, the Python wrappers' argument
checks, layout.ragged_offsets and the Fortran bindings.

This file also holds what tests/test_hvbatch.py (eigen_h_vbatch) shares with it: the two families (S, H), the buffers of a
ragged call (Ragged) and the bodies of the GPU tests (check_*), which take the family.  The matrix families and the gates are
those of tests/test_batch.py / tests/test_hbatch.py: eigenvalues against numpy.linalg.eigvalsh to 1e-12 max(1, max|w|),
ascending order, and the residual and orthogonality gates of tests/golden/known_answers.json."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_batch as tb
import test_hbatch as thb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLANG = tb.FLANG
GUARD = tb.GUARD
BAD_ARG, NONFINITE = -2, -5
VBATCH_HEADER = os.path.join(ROOT, "include", "eigenexa_amd_vbatch.h")
SOLVERS = ["eigx_s_vbatch", "eigx_s_vbatch_dev", "eigx_h_vbatch", "eigx_h_vbatch_dev"]
ENTRIES = SOLVERS + ["eigx_vbatch_plan"]
ARG_NAMES = ["batch", "n", "a", "off_a", "lda", "w", "off_w", "z", "off_z", "ldz", "mode", "info"]


class Family:
    """what differs between eigen_s_vbatch and eigen_h_vbatch: cs = doubles per element of a and z"""

    def __init__(self, name, cs, top, key, sizes, big, mod):
        self.name, self.cs, self.top, self.key, self.sizes, self.big, self.mod = name, cs, top, key, sizes, big, mod

    def families(self, n):
        return self.mod._families(n)

    def check_matrix(self, A, w, Z=None, tag=""):
        return self.mod._check_matrix(A, w, Z, tag)

    def random(self, n, seed):
        from eigenexa_amd import layout

        return layout.random_symmetric(n, seed=seed) if self.cs == 1 else thb._herm(layout.random_hermitian(n, seed=seed))

    def vbatch(self, lib, host=False):
        return getattr(lib, f"eigx_{self.name}_vbatch" + ("" if host else "_dev"))

    def uniform(self, lib):
        return getattr(lib, f"eigx_{self.name}_batch_dev")

    def full(self, lib):
        return getattr(lib, f"eigx_{self.name}_dev")


# sizes: the class boundaries (32, 64, 96 and for S 128) from both sides; big: the first order above the largest class
S = Family("s", 1, 128, 21, [1, 2, 3, 5, 17, 32, 33, 64, 65, 96, 97, 127, 128], 129, tb)
H = Family("h", 2, 96, 22, [1, 2, 3, 5, 17, 32, 33, 64, 65, 95, 96], 97, thb)


def _dev():
    import torch

    return torch.device("cuda:0")


class Ragged:
    """buffers of one ragged call, on the host (numpy, float64; complex interleaved) and on the device: lda = n + 3,
    ldz = n + 1, offsets with gaps in front of every block; a holds NaN in the strict lower triangles, the padding rows, the gaps
    and (H) the imaginary parts of the diagonals; w, z and info are prefilled with guards.  An empty block (a 0 x 0 matrix) gets
    offsets inside the gaps.  Offsets and leading dimensions count elements."""

    def __init__(self, fam, mats, device=True):
        self.fam, self.mats = fam, mats
        cs = fam.cs
        self.batch = nb = len(mats)
        self.n = np.array([M.shape[0] for M in mats], dtype=np.int32).reshape(nb)
        self.lda = (self.n + 3).astype(np.int32)
        self.ldz = (self.n + 1).astype(np.int32)
        n64 = self.n.astype(np.int64)
        self.off_a = np.zeros(nb, dtype=np.int64)
        self.off_w = np.zeros(nb, dtype=np.int64)
        self.off_z = np.zeros(nb, dtype=np.int64)
        ta = tw = tz = 0
        for k in range(nb):
            self.off_a[k], ta = ta + 5, ta + 5 + int(self.lda[k]) * int(n64[k])
            self.off_w[k], tw = tw + 2, tw + 2 + int(n64[k])
            self.off_z[k], tz = tz + 7, tz + 7 + int(self.ldz[k]) * int(n64[k])
        self.len_a, self.len_w, self.len_z = ta + 5, tw + 2, tz + 7
        self.a_host = np.full(cs * self.len_a, np.nan)
        self.wmask = np.zeros(self.len_w, dtype=bool)            # what the call may write
        self.zmask = np.zeros((self.len_z, cs), dtype=bool)
        for k, M in enumerate(mats):
            n = int(self.n[k])
            if n == 0:
                continue
            v = self.a_host[cs * self.off_a[k]:cs * (self.off_a[k] + self.lda[k] * n)].reshape(n, self.lda[k], cs)   # v[j, i] = a(i, j)
            upper = np.tri(n, dtype=bool)                         # [j, i]: i <= j
            v[:, :n, 0] = np.where(upper, M.T.real, np.nan)
            if cs == 2:
                v[:, :n, 1] = np.where(upper, M.T.imag, np.nan)
                v[np.arange(n), np.arange(n), 1] = np.nan
            self.wmask[self.off_w[k]:self.off_w[k] + n] = True
            self.zmask[self.off_z[k]:self.off_z[k] + self.ldz[k] * n].reshape(n, self.ldz[k], cs)[:, :n] = True
        self.zmask = self.zmask.reshape(-1)
        self.a_work = self.a_host.copy()                          # the a of a host call (destroyed)
        self.w_host = np.full(self.len_w, GUARD)
        self.z_host = np.full(cs * self.len_z, GUARD)
        self.info_host = np.full(nb, 77, dtype=np.int32)
        if device:
            import torch

            self.a = torch.from_numpy(self.a_host).to(_dev())
            self.w = torch.full((self.len_w,), GUARD, dtype=torch.float64, device=_dev())
            self.z = torch.full((cs * self.len_z,), GUARD, dtype=torch.float64, device=_dev())
            self.info = torch.full((nb,), 77, dtype=torch.int32, device=_dev())

    def refill(self):
        import torch

        self.a.copy_(torch.from_numpy(self.a_host))
        self.w.fill_(GUARD)
        self.z.fill_(GUARD)
        self.info.fill_(77)

    def args(self, mode=b"A", info=True, z=True, host=False, **change):
        """the argument list of a call; change: name -> value of the arguments to replace"""
        if host:
            self.a_work = self.a_host.copy()
            arrays = dict(a=self.a_work.ctypes.data, w=self.w_host.ctypes.data, z=self.z_host.ctypes.data, info=self.info_host.ctypes.data)
        else:
            arrays = dict(a=self.a.data_ptr(), w=self.w.data_ptr(), z=self.z.data_ptr(), info=self.info.data_ptr())
        g = dict(batch=self.batch, n=self.n, off_a=self.off_a, lda=self.lda, off_w=self.off_w, off_z=self.off_z, ldz=self.ldz,
                 mode=mode, **arrays)
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
        """(w, z, info) as numpy arrays, whole buffers"""
        if host:
            return self.w_host, self.z_host, self.info_host
        return self.w.cpu().numpy(), self.z.cpu().numpy(), self.info.cpu().numpy()

    def block_a(self, k):
        """address of block k of the device a, and of its w and z"""
        cs = self.fam.cs
        return (self.a.data_ptr() + 8 * cs * int(self.off_a[k]), self.w.data_ptr() + 8 * int(self.off_w[k]),
                self.z.data_ptr() + 8 * cs * int(self.off_z[k]))

    def results(self, want_z=True, host=False, untouched=()):
        """per block: w (n), Z (n, n) with Z[:, j] the j-th eigenvector; info; asserts that every guard outside w(1:n_k) and
        z(1:n_k, 1:n_k) survived, and (want_z false, or k in untouched) those of z inside too"""
        cs = self.fam.cs
        wb, zb, info = self.images(host)
        assert (wb[~self.wmask] == GUARD).all(), "w outside the blocks was touched"
        assert (zb[~self.zmask] == GUARD).all(), "z outside the blocks (padding rows, gaps) was touched"
        if not want_z:
            assert (zb == GUARD).all(), "z was touched"
        ws, Zs = [], []
        for k in range(self.batch):
            n = int(self.n[k])
            ws.append(wb[self.off_w[k]:self.off_w[k] + n].copy())
            zz = zb[cs * self.off_z[k]:cs * (self.off_z[k] + self.ldz[k] * n)].reshape(n, self.ldz[k], cs)[:, :n]
            if k in untouched:
                assert (zz == GUARD).all(), f"z of block {k} was touched"
            Zs.append((zz[:, :, 0] + (1j * zz[:, :, 1] if cs == 2 else 0.0)).T.copy())
        return ws, Zs, info.copy()


def solve_blocks_alone(lib, R, cutoff=None):
    """every block of R solved on its own, in place in R's device buffers: eigx_*_batch_dev(n_k, 1, ...) at or below the cutoff,
    eigx_*_dev(n_k, n_k, ..., 48, 128, 'A') above it (what eigx_*_batch does there)"""
    fam = R.fam
    cutoff = fam.top if cutoff is None else cutoff
    for k in range(R.batch):
        n = int(R.n[k])
        if n == 0:
            continue
        pa, pw, pz = R.block_a(k)
        if n <= cutoff:
            assert fam.uniform(lib)(n, 1, pa, int(R.lda[k]), 0, pw, n, pz, int(R.ldz[k]), 0, b"A", None) == 0, k
        else:
            assert fam.full(lib)(n, n, pa, int(R.lda[k]), pw, pz, int(R.ldz[k]), 48, 128, b"A") == 0, k


def same_bits(R1, R2):
    """w and z of two calls on the same layout agree bit for bit, whole buffers (the guards included)"""
    w1, z1, _ = R1.images()
    w2, z2, _ = R2.images()
    return np.array_equal(w1.view(np.int64), w2.view(np.int64)) and np.array_equal(z1.view(np.int64), z2.view(np.int64))


_MIXED = {}


def mixed_mats(fam):
    """three members of the families per size of fam.sizes -- member 3 i + j of size number i, so every family occurs -- in a
    shuffled order; computed once and left unchanged"""
    if fam.name not in _MIXED:
        mats = []
        for i, n in enumerate(fam.sizes):
            F = fam.families(n)
            mats += [F[(3 * i + j) % len(F)] for j in range(3)]
        order = np.random.default_rng(11).permutation(len(mats))
        mats = [mats[q] for q in order]
        for M in mats:
            M.setflags(write=False)
        _MIXED[fam.name] = mats
    return _MIXED[fam.name]


# ------------------------------------------------------------------------------------------------ 1. ragged mixed call
def check_mixed(lib, fam):
    mats = mixed_mats(fam)
    R = Ragged(fam, mats)
    assert R.run(lib) == 0
    ws, Zs, info = R.results()
    assert (info == 0).all()
    worst = [0.0, 0.0]
    for k, A in enumerate(mats):
        r, o = fam.check_matrix(A, ws[k], Zs[k], f"block {k} n={A.shape[0]}")
        worst = [max(worst[0], r), max(worst[1], o)]
    print(f"{fam.name}: {len(mats)} blocks, worst residual {worst[0]:.3e}, worst orthogonality {worst[1]:.3e}")


@pytest.mark.gpu
def test_ragged_mixed_call(gpu_lib):
    check_mixed(gpu_lib, S)


# ------------------------------------------------------------------------------------------------ 2. many workgroups
def check_many(lib, fam):
    """1500 blocks with n drawn from 1 .. 24 and a few of n = 40 (two classes, more workgroups than the card holds): every block
    is checked"""
    rng = np.random.default_rng(5)
    sizes = rng.integers(1, 25, 1500)
    sizes[[3, 700, 1499]] = 40
    mats = []
    for n in sizes:
        G = rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if fam.cs == 2 else 0.0)
        mats.append(thb._herm(G + G.conj().T) if fam.cs == 2 else G + G.T)
    R = Ragged(fam, mats)
    assert R.run(lib) == 0
    ws, Zs, info = R.results()
    assert (info == 0).all()
    eps = np.finfo(np.float64).eps
    worst = [0.0, 0.0, 0.0]
    for k, A in enumerate(mats):
        n = A.shape[0]
        wr = np.linalg.eigvalsh(A)
        werr = np.abs(ws[k] - wr).max() / (1e-12 * max(1.0, np.abs(wr).max()))
        res = np.linalg.norm(A @ Zs[k] - Zs[k] * ws[k][None, :]) / (n * eps * np.linalg.norm(A))
        orth = np.linalg.norm(Zs[k].conj().T @ Zs[k] - np.eye(n)) / (n * eps)
        assert (np.diff(ws[k]) >= 0).all(), k
        worst = [max(worst[0], werr), max(worst[1], res), max(worst[2], orth)]
    print(f"{fam.name}: 1500 blocks: worst eigenvalue error {worst[0]:.3e} of its gate, residual {worst[1]:.3e}, "
          f"orthogonality {worst[2]:.3e}")
    assert worst[0] <= 1.0 and worst[1] < tb.GATE_RES and worst[2] < tb.GATE_ORTH


@pytest.mark.gpu
def test_more_workgroups_than_the_card_holds(gpu_lib):
    check_many(gpu_lib, S)


# ------------------------------------------------------------------------------------------------ 3. bit identity
def check_bits(lib, fam):
    """every block of the mixed call against eigx_*_batch_dev(n_k, 1, ...) on a copy; the same call with the blocks in reversed
    order; the same call twice"""
    mats = mixed_mats(fam)
    R = Ragged(fam, mats)
    assert R.run(lib) == 0
    alone = Ragged(fam, mats)
    solve_blocks_alone(lib, alone)
    assert same_bits(R, alone), "a block differs from the uniform entry's solve of it"
    again = Ragged(fam, mats)
    assert again.run(lib) == 0
    assert same_bits(R, again), "two runs differ"
    ws, Zs, _ = R.results()
    rev = Ragged(fam, mats[::-1])
    assert rev.run(lib) == 0
    wr, Zr, _ = rev.results()
    nb = len(mats)
    for k in range(nb):
        assert np.array_equal(ws[k], wr[nb - 1 - k]) and np.array_equal(Zs[k], Zr[nb - 1 - k]), f"block {k} depends on the order"


@pytest.mark.gpu
def test_bit_identity_with_the_uniform_entry(gpu_lib):
    check_bits(gpu_lib, S)


# ------------------------------------------------------------------------------------------------ 3b. two entries, one result
def check_edges_with_a_failed_block(lib, fam):
    """The uniform and the ragged entry promise the same bits, failures included.  One block at n = 1, 2 and on both sides of every n-class edge the
    kernels reach, and a NaN block between two good ones: w, z and info of the ragged call against eigx_*_batch_dev(n_k, 1, ...)
    with info, bit for bit, whole buffers; the failed block has w = NaN, its status, and z untouched in both"""
    sizes = [n for n in (1, 2, 32, 33, 64, 65, 96, 97, 128) if n <= fam.top]
    mats = [fam.random(n, seed=200 + n) for n in sizes]
    bad = fam.random(40, seed=7).copy()
    bad[3, 30] = bad[30, 3] = np.nan
    mats.insert(3, bad)                                             # between the blocks of n = 32 and n = 33
    codes = [NONFINITE if k == 3 else 0 for k in range(len(mats))]
    R = Ragged(fam, mats)
    assert R.run(lib) == NONFINITE
    alone = Ragged(fam, mats)
    for k, M in enumerate(mats):
        n = M.shape[0]
        pa, pw, pz = alone.block_a(k)
        rc = fam.uniform(lib)(n, 1, pa, int(alone.lda[k]), 0, pw, n, pz, int(alone.ldz[k]), 0, b"A", alone.info.data_ptr() + 4 * k)
        assert rc == codes[k], k
    assert same_bits(R, alone), "a block differs from the uniform entry's solve of it"
    for X in (R, alone):
        ws, Zs, info = X.results(untouched=[3])
        assert info.tolist() == codes
        assert np.isnan(ws[3]).all()
        for k, M in enumerate(mats):
            if k != 3:
                fam.check_matrix(M, ws[k], Zs[k], f"block {k} n={M.shape[0]}")


@pytest.mark.gpu
def test_ragged_equals_uniform_at_the_class_edges_with_a_failed_block(gpu_lib):
    check_edges_with_a_failed_block(gpu_lib, S)


def check_uniform_failed_middle(lib, fam):
    """The uniform entry, one n per class: a batch of three whose middle matrix holds a NaN leaves w, z and info of its
    neighbours as their solo calls (batch = 1) leave them, bit for bit, and the failed matrix as its solo call leaves it.  (Three
    blocks of one order in the buffers of a ragged call are evenly spaced: a uniform batch with those strides.)"""
    for n in [n for n in (5, 33, 65, 97) if n <= fam.top]:
        mats = [fam.random(n, seed=300 + n + k).copy() for k in range(3)]
        mats[1][0, n - 1] = mats[1][n - 1, 0] = np.nan
        T, solo = Ragged(fam, mats), Ragged(fam, mats)
        lda, ldz = int(T.lda[0]), int(T.ldz[0])
        steps = [int(v[1] - v[0]) for v in (T.off_a, T.off_w, T.off_z)]
        assert all(int(v[2] - v[1]) == s for v, s in zip((T.off_a, T.off_w, T.off_z), steps))
        pa, pw, pz = T.block_a(0)
        assert fam.uniform(lib)(n, 3, pa, lda, steps[0], pw, steps[1], pz, ldz, steps[2], b"A", T.info.data_ptr()) == NONFINITE
        for k in range(3):
            pa, pw, pz = solo.block_a(k)
            rc = fam.uniform(lib)(n, 1, pa, lda, 0, pw, n, pz, ldz, 0, b"A", solo.info.data_ptr() + 4 * k)
            assert rc == (NONFINITE if k == 1 else 0)
        assert same_bits(T, solo), f"n={n}: a matrix beside a failed one differs from its solo result"
        ws, Zs, info = T.results(untouched=[1])
        assert info.tolist() == [0, NONFINITE, 0] and np.array_equal(info, solo.results(untouched=[1])[2])
        assert np.isnan(ws[1]).all()
        for k in (0, 2):
            fam.check_matrix(mats[k], ws[k], Zs[k], f"n={n}, matrix {k} beside the failed one")


@pytest.mark.gpu
def test_uniform_failed_matrix_leaves_its_neighbours(gpu_lib):
    check_uniform_failed_middle(gpu_lib, S)


# ------------------------------------------------------------------------------------------------ 4. mode 'N'
def check_mode_n(lib, fam):
    mats = mixed_mats(fam)
    R = Ragged(fam, mats)
    assert R.run(lib) == 0
    wa = R.images()[0]
    for z in (True, False):                                        # z, off_z, ldz passed, then all three NULL
        R.refill()
        assert R.run(lib, mode=b"N", z=z) == 0
        wn, _, info = R.images()
        R.results(want_z=False)
        assert (info == 0).all()
        assert np.array_equal(wn.view(np.int64), wa.view(np.int64)), "w of mode 'N' differs from mode 'A'"


@pytest.mark.gpu
def test_mode_n(gpu_lib):
    check_mode_n(gpu_lib, S)


# ------------------------------------------------------------------------------------------------ 5. failures are local
def failing_mats(fam):
    """good blocks of several classes with a NaN block at the first, an Inf block at a middle and a NaN block at the last
    position (H: the NaN in real parts, the Inf in an imaginary part); the first failed block lies in the smallest class, which
    is launched last"""
    big = 100 if fam.cs == 1 else 90
    sizes = [12, 70, big, 33, 5, 40]
    mats = [fam.random(n, seed=60 + k).copy() for k, n in enumerate(sizes)]
    mats[0][4, 9] = mats[0][9, 4] = np.nan
    if fam.cs == 1:
        mats[2][0, big - 1] = mats[2][big - 1, 0] = np.inf
    else:
        mats[2][0, big - 1] = complex(1.0, np.inf)
        mats[2][big - 1, 0] = complex(1.0, -np.inf)
    mats[5][7, 7] = np.nan
    return mats, [0, 2, 5]


def check_failures(lib, fam):
    mats, failed = failing_mats(fam)
    R = Ragged(fam, mats)
    for with_info in (True, False):
        R.refill()
        assert R.run(lib, info=with_info) == NONFINITE
        ws, Zs, info = R.results(untouched=failed)
        assert info.tolist() == ([NONFINITE if k in failed else 0 for k in range(len(mats))] if with_info else [77] * len(mats))
        for k, A in enumerate(mats):
            if k in failed:
                assert np.isnan(ws[k]).all(), k
            else:
                fam.check_matrix(A, ws[k], Zs[k], f"block {k} beside failed ones")


@pytest.mark.gpu
def test_failures_are_local(gpu_lib):
    check_failures(gpu_lib, S)


# ------------------------------------------------------------------------------------------------ 6. above the cutoff
def check_above_cutoff(lib, fam):
    # default cutoff: one block of the first order above the largest class among small ones
    mats = [fam.random(n, seed=90 + k) for k, n in enumerate([5, 33, fam.big, 17])]
    R = Ragged(fam, mats)
    assert R.run(lib) == 0
    alone = Ragged(fam, mats)
    solve_blocks_alone(lib, alone)
    assert same_bits(R, alone)
    # (the statistics the full-size solver leaves in a(1, 1): the same flop count)
    q = fam.cs * int(R.off_a[2])
    assert R.a[q].item() == alone.a[q].item()
    ws, Zs, info = R.results()
    assert (info == 0).all()
    for k, A in enumerate(mats):
        fam.check_matrix(A, ws[k], Zs[k], f"default cutoff, block {k} n={A.shape[0]}")
    # key = 32: the block of n = 40 goes through the full-size solver, the others through the kernel as before
    mats = [fam.random(n, seed=95 + k) for k, n in enumerate([5, 40, 20, 32])]
    R = Ragged(fam, mats)
    small = Ragged(fam, mats)
    solve_blocks_alone(lib, small)                                  # (default cutoff: every block by the uniform kernel)
    old = lib.eigx_tune(fam.key, 32)
    try:
        assert old == fam.top
        assert R.run(lib) == 0
        alone = Ragged(fam, mats)
        solve_blocks_alone(lib, alone, cutoff=32)
    finally:
        assert lib.eigx_tune(fam.key, old) == 32
    assert same_bits(R, alone)
    ws, Zs, info = R.results()
    wk, Zk, _ = small.results()
    assert (info == 0).all()
    for k, A in enumerate(mats):
        fam.check_matrix(A, ws[k], Zs[k], f"key {fam.key} = 32, block {k} n={A.shape[0]}")
        if k != 1:
            assert np.array_equal(ws[k], wk[k]) and np.array_equal(Zs[k], Zk[k]), k
    # key = 0: every block through the full-size solver; a NaN block gets its own status
    mats = [fam.random(n, seed=99 + k).copy() for k, n in enumerate([6, 9, 12])]
    mats[1][2, 5] = mats[1][5, 2] = np.nan
    R = Ragged(fam, mats)
    old = lib.eigx_tune(fam.key, 0)
    try:
        rc = R.run(lib)
    finally:
        assert lib.eigx_tune(fam.key, old) == 0
    assert rc == NONFINITE
    ws, Zs, info = R.results()
    assert info.tolist() == [0, NONFINITE, 0] and np.isnan(ws[1]).all()
    for k in (0, 2):
        fam.check_matrix(mats[k], ws[k], Zs[k], f"key {fam.key} = 0, block {k}")


@pytest.mark.gpu
def test_above_the_cutoff(gpu_lib):
    check_above_cutoff(gpu_lib, S)


# errinfo after a call in which one block failed, as the library before the shared host frame (csrc/batch_frame.hip) returned it on
# a GPU: the ragged frame merges the failures of the blocks above the cutoff into the first-failure word, so both routes set -1
# (the uniform entry leaves 0 above the cutoff: tests/test_batch.py and the table of DESIGN section 8h)
ERRINFO_AFTER_FAILURE = {"kernel": -1, "loop": -1}


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["kernel", "loop"])
def test_errinfo_after_a_failed_block(gpu_lib, route):
    """device form, the three 5 x 5 matrices of tests/test_batch.py; route "loop": key 21 = 4, so that every block goes through
    eigx_s_dev"""
    R = Ragged(S, tb.errinfo_case())
    old = gpu_lib.eigx_tune(21, 4) if route == "loop" else None
    try:
        rc = R.run(gpu_lib)
        err = tb.errinfo_after(gpu_lib)
    finally:
        if old is not None:
            assert gpu_lib.eigx_tune(21, old) == 4
    ws, Zs, info = R.results()
    print(f"eigx_s_vbatch_dev, {route}: status {rc}, info {info.tolist()}, errinfo {err}")
    assert rc == NONFINITE and info.tolist() == [0, NONFINITE, 0]
    assert np.isnan(ws[1]).all() and np.isfinite(ws[0]).all() and np.isfinite(ws[2]).all()
    assert err == ERRINFO_AFTER_FAILURE[route]


# ------------------------------------------------------------------------------------------------ 7. empty blocks
def check_empty(lib, fam):
    dt = np.float64 if fam.cs == 1 else np.complex128
    none = np.zeros((0, 0), dtype=dt)
    mats = [none, fam.random(5, seed=1), none, fam.random(33, seed=2), none]
    R = Ragged(fam, mats)
    assert R.run(lib) == 0
    ws, Zs, info = R.results()
    assert (info == 0).all()
    for k in (1, 3):
        fam.check_matrix(mats[k], ws[k], Zs[k], f"block {k} between empty ones")
    E = Ragged(fam, [none, none])                                   # nothing but empty blocks
    assert E.run(lib) == 0
    _, _, info = E.results(want_z=False)
    assert (info == 0).all()
    R.refill()                                                      # batch = 0: nothing is touched
    assert R.run(lib, batch=0) == 0
    assert fam.vbatch(lib)(0, None, None, None, None, None, None, None, None, None, b"A", None) == 0
    assert fam.vbatch(lib, host=True)(0, None, None, None, None, None, None, None, None, None, b"A", None) == 0
    _, _, info = R.results(want_z=False)
    assert (R.w.cpu().numpy() == GUARD).all() and (info == 77).all()


@pytest.mark.gpu
def test_empty_blocks(gpu_lib):
    check_empty(gpu_lib, S)


# ------------------------------------------------------------------------------------------------ 8. scales
def check_scales(lib, fam):
    """blocks of scale 1e120, 1 and 1e-120 and of different sizes in one call: each is scaled by its own max|a|"""
    sizes, scales = [20, 45, 90], [1e120, 1.0, 1e-120]
    base = [fam.random(n, seed=4 + n) for n in sizes]
    R = Ragged(fam, [A * f for A, f in zip(base, scales)])
    assert R.run(lib) == 0
    ws, Zs, info = R.results()
    assert (info == 0).all()
    for k, (A, f) in enumerate(zip(base, scales)):
        wr = np.linalg.eigvalsh(A)
        werr = np.abs(ws[k] / f - wr).max() / np.abs(wr).max()
        res, orth = fam.mod._gates(A, ws[k] / f, Zs[k])
        print(f"  n={sizes[k]} scale {f:g}: |w - w_lapack| / max|w| = {werr:.2e}, residual {res:.3e}, orthogonality {orth:.3e}")
        assert werr <= 1e-12 and res < tb.GATE_RES and orth < tb.GATE_ORTH


@pytest.mark.gpu
def test_scales_in_one_call(gpu_lib):
    check_scales(gpu_lib, S)


# ------------------------------------------------------------------------------------------------ 9. host and device forms
def check_host_form(lib, fam):
    """w, z and info of the host form are those of the device form, bit for bit, every guard and the z of the failed blocks
    included"""
    mats, failed = failing_mats(fam)
    R = Ragged(fam, mats)
    assert R.run(lib) == NONFINITE
    wd, zd, idv = R.images()
    assert R.run(lib, host=True) == NONFINITE
    wh, zh, ih = R.images(host=True)
    R.results(host=True, untouched=failed)
    assert np.array_equal(wh.view(np.int64), wd.view(np.int64)) and np.array_equal(zh.view(np.int64), zd.view(np.int64))
    assert np.array_equal(ih, idv)
    # mode 'N' with z, off_z, ldz = NULL and info = NULL
    R.w_host[:] = GUARD
    R.z_host[:] = GUARD
    R.info_host[:] = 77
    assert R.run(lib, mode=b"N", z=False, info=False, host=True) == NONFINITE
    assert np.array_equal(R.w_host.view(np.int64), wd.view(np.int64)) and (R.z_host == GUARD).all() and (R.info_host == 77).all()


@pytest.mark.gpu
def test_host_and_device_forms_agree(gpu_lib):
    check_host_form(gpu_lib, S)


# ------------------------------------------------------------------------------------------------ 10., 11. arguments, timers
def check_arguments(lib, fam):
    mats = [fam.random(n, seed=n) for n in (12, 7, 30)]
    R = Ragged(fam, mats)
    nb = R.batch

    def at(v, k, x):
        v = v.copy()
        v[k] = x
        return v

    bad = [dict(batch=-1), dict(n=None), dict(a=None), dict(off_a=None), dict(lda=None), dict(w=None), dict(off_w=None),
           dict(z=None), dict(off_z=None), dict(ldz=None), dict(mode=b"X"), dict(mode=b"S"), dict(mode=b"C"), dict(mode=b"V"),
           dict(n=at(R.n, 1, -1)), dict(lda=at(R.lda, 2, 29)), dict(off_a=at(R.off_a, 0, -1)), dict(off_w=at(R.off_w, 1, -1)),
           dict(off_z=at(R.off_z, 2, -1)), dict(ldz=at(R.ldz, 0, 11))]
    for host in (False, True):
        for change in bad:
            assert R.run(lib, host=host, **change) == BAD_ARG, (host, list(change))
        assert np.array_equal(R.a_work, R.a_host, equal_nan=True)
    for host in (False, True):                                      # nothing was touched
        wb, zb, info = R.images(host)
        assert (wb == GUARD).all() and (zb == GUARD).all() and (info == 77).all()
    assert np.array_equal(R.a.cpu().numpy(), R.a_host, equal_nan=True)
    # mode 'N' does not look at ldz and off_z; lower-case mode
    assert R.run(lib, mode=b"n", ldz=at(R.ldz, 0, 0), off_z=at(R.off_z, 0, -5)) == 0
    ws, _, info = R.results(want_z=False)
    assert (info == 0).all()
    for k, A in enumerate(mats):
        fam.check_matrix(A, ws[k], None, f"mode n, block {k}")
    t = (C.c_double * 16)()
    lib.eigx_get_timers(t)
    assert t[0] > 0.0 and all(t[q] == 0.0 for q in range(1, 16))
    R.refill()
    assert R.run(lib, mode=b"a", info=False) == 0
    ws, Zs, info = R.results()
    assert (info == 77).all()
    for k, A in enumerate(mats):
        fam.check_matrix(A, ws[k], Zs[k], f"mode a, info NULL, block {k}")
    lib.eigx_get_timers(t)
    assert t[0] > 0.0 and all(t[q] == 0.0 for q in range(1, 16))


@pytest.mark.gpu
def test_arguments_and_timers(gpu_lib):
    check_arguments(gpu_lib, S)


# ------------------------------------------------------------------------------------------------ 12. two ranks
@pytest.mark.gpu
def test_vbatch_refuses_several_ranks():
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
    script = os.path.join(os.path.dirname(__file__), "vbatch_worker.py")
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


# ------------------------------------------------------------------------------------------------ 13. Fortran
def run_fortran_caller(tmp_path, name):
    """build tests/fortran/<name>.F90 against the module and run it: its output"""
    lib = os.path.join(ROOT, "eigenexa_amd", "lib")
    mod = os.path.join(ROOT, "eigenexa_amd", "fortran", "eigen_libs_mod.F90")
    src = os.path.join(ROOT, "tests", "fortran", name + ".F90")
    subprocess.check_call([FLANG, "-cpp", "-O2", "-c", mod, "-o", "eigen_libs_mod.o"], cwd=tmp_path)
    subprocess.check_call([FLANG, "-cpp", "-O2", "-c", src, "-o", name + ".o"], cwd=tmp_path)
    subprocess.check_call([FLANG, "-o", name, name + ".o", "eigen_libs_mod.o", f"-L{lib}", "-leigenexa_amd", f"-Wl,-rpath,{lib}"],
                          cwd=tmp_path)
    out = subprocess.run([str(tmp_path / name)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"max rel eigenvalue error\s*=\s*([0-9.eEdD+-]+)", out.stdout)
    assert m, out.stdout
    assert float(m.group(1).replace("D", "E").replace("d", "e")) < tb.GOLD["gates"]["frank_rel_err"], out.stdout


@pytest.mark.gpu
def test_fortran_vbatch_caller(gpu_lib, tmp_path):
    """a Fortran program calls eigen_s_vbatch of module eigen_libs_mod on Frank blocks of the orders 7, 30, 70 and 12 held in
    flat arrays with 1-based start indices"""
    if not os.path.exists(FLANG):
        pytest.skip("no flang")
    run_fortran_caller(tmp_path, "vbatch_caller")


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", SOLVERS)
def test_header_prototypes_match_the_ctypes_table(monkeypatch, name):
    """the entries are declared in include/eigenexa_amd_vbatch.h and mirrored by _lib.VBATCH_SIGNATURES: the parser of the
    other header tests, pointed at that file"""
    import c_header
    from eigenexa_amd import _lib

    monkeypatch.setattr(c_header, "HEADER", VBATCH_HEADER)
    params = c_header.prototype(name)
    restype, argtypes = _lib.VBATCH_SIGNATURES[name]
    assert restype is C.c_int and len(argtypes) == len(params) == 12
    for p, t in zip(params, argtypes):
        if p.startswith("char "):
            assert t is C.c_char
        elif "*" in p:
            assert t is C.c_void_p
        else:
            assert p.startswith("int ") and t is C.c_int
    assert [p.split()[-1].replace("_dev", "") for p in params] == ARG_NAMES
    for p in params:                                                # the descriptors: const int* / const int64_t*
        if p.split()[-1] in ("n", "lda", "ldz"):
            assert p.startswith("const int*")
        if p.split()[-1].startswith("off_"):
            assert p.startswith("const int64_t*")


def test_the_vbatch_header_is_part_of_the_public_one(monkeypatch):
    """eigenexa_amd.h includes the file, the file declares exactly the entries of the table, no name sits in two tables, and
    the loaded library has them with these signatures"""
    import c_header
    from eigenexa_amd import _lib

    main = open(os.path.join(ROOT, "include", "eigenexa_amd.h")).read()
    assert re.search(r'^#include "eigenexa_amd_vbatch\.h"$', main, flags=re.M)
    monkeypatch.setattr(c_header, "HEADER", VBATCH_HEADER)
    protos = c_header.all_prototypes()
    assert set(protos) == set(_lib.VBATCH_SIGNATURES) == set(ENTRIES)
    ret, params = protos["eigx_vbatch_plan"]
    assert ret == "int" and [p.split()[-1] for p in params] == ["batch", "n", "cutoff", "top", "order", "counts6"]
    assert [("*" in p) for p in params] == [t is C.c_void_p for t in _lib.VBATCH_SIGNATURES["eigx_vbatch_plan"][1]]
    tables = [_lib.SIGNATURES, _lib.GBATCH_SIGNATURES, _lib.HGBATCH_SIGNATURES, _lib.VBATCH_SIGNATURES, _lib.LAB_SIGNATURES]
    for i, t1 in enumerate(tables):
        for t2 in tables[i + 1:]:
            assert not set(t1) & set(t2)
    lib = _lib.load()
    for name, (restype, argtypes) in _lib.VBATCH_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes


def plan_by_numpy(n, cutoff, top):
    """the schedule restated: (order, counts6)"""
    n = np.asarray(n, dtype=np.int64)
    idx = np.arange(len(n))
    cls = np.where(n <= 32, 32, np.where(n <= 64, 64, np.where((n <= 96) | (top == 96), 96, 128)))
    served = (n >= 1) & (n <= cutoff)
    group = np.where(served, 0, np.where(n > cutoff, 1, 2))         # kernel-served, above the cutoff, empty
    # served: by class descending, then n descending, then index; the others by index alone
    k1 = np.where(served, -cls, 0)
    k2 = np.where(served, -n, 0)
    order = np.lexsort((idx, k2, k1, group))
    counts = [int((served & (cls == c)).sum()) for c in (32, 64, 96, 128)] + [int((group == 1).sum()), int((n == 0).sum())]
    return order, counts


def _plan(lib, n, cutoff, top):
    n = np.ascontiguousarray(n, dtype=np.int32)
    order = np.full(len(n), -1, dtype=np.int32)
    counts = np.full(6, -1, dtype=np.int32)
    rc = lib.eigx_vbatch_plan(len(n), n.ctypes.data, cutoff, top, order.ctypes.data, counts.ctypes.data)
    return rc, order, counts


@pytest.mark.parametrize("top", [96, 128])
@pytest.mark.parametrize("cutoff", [0, 32, 96, 128])
def test_plan_against_numpy(top, cutoff):
    """eigx_vbatch_plan (no GPU, no eigx_init) against a numpy restatement on random size vectors with zeros and sizes above
    the cutoff"""
    from eigenexa_amd import _lib

    lib = _lib.load()
    rng = np.random.default_rng(100 * top + cutoff)
    if cutoff > top:
        assert _plan(lib, [1, 2, 3], cutoff, top)[0] == BAD_ARG
        return
    cases = [rng.integers(0, 140, 500), rng.integers(0, 3, 50), rng.integers(90, 100, 64), np.full(40, 64), np.arange(130, -1, -1),
             np.zeros(7, dtype=int), np.array([5]), np.array([], dtype=int), np.array([300, 1, 0, 128, 97, 96, 65, 64, 33, 32])]
    for n in cases:
        rc, order, counts = _plan(lib, n, cutoff, top)
        assert rc == 0
        ref_order, ref_counts = plan_by_numpy(n, cutoff, top)
        assert order.tolist() == ref_order.tolist(), (n, cutoff, top)
        assert counts.tolist() == ref_counts and sum(ref_counts) == len(n)
        assert sorted(order.tolist()) == list(range(len(n)))


def test_plan_refusals():
    from eigenexa_amd import _lib

    lib = _lib.load()
    order = np.zeros(4, dtype=np.int32)
    counts = np.zeros(6, dtype=np.int32)
    n = np.array([3, -1, 5, 0], dtype=np.int32)
    good = np.array([3, 1, 5, 0], dtype=np.int32)
    assert lib.eigx_vbatch_plan(4, n.ctypes.data, 128, 128, order.ctypes.data, counts.ctypes.data) == BAD_ARG
    for top in (0, 32, 64, 127, 129, -96):
        assert lib.eigx_vbatch_plan(4, good.ctypes.data, 32, top, order.ctypes.data, counts.ctypes.data) == BAD_ARG
    assert lib.eigx_vbatch_plan(-1, good.ctypes.data, 32, 96, order.ctypes.data, counts.ctypes.data) == BAD_ARG
    assert lib.eigx_vbatch_plan(4, good.ctypes.data, -1, 96, order.ctypes.data, counts.ctypes.data) == BAD_ARG
    assert lib.eigx_vbatch_plan(4, good.ctypes.data, 97, 96, order.ctypes.data, counts.ctypes.data) == BAD_ARG
    assert lib.eigx_vbatch_plan(4, None, 32, 96, order.ctypes.data, counts.ctypes.data) == BAD_ARG
    assert lib.eigx_vbatch_plan(4, good.ctypes.data, 32, 96, None, counts.ctypes.data) == BAD_ARG
    assert lib.eigx_vbatch_plan(4, good.ctypes.data, 32, 96, order.ctypes.data, None) == BAD_ARG
    assert lib.eigx_vbatch_plan(4, good.ctypes.data, 32, 96, order.ctypes.data, counts.ctypes.data) == 0
    assert order.tolist() == [2, 0, 1, 3] and counts.tolist() == [3, 0, 0, 0, 0, 1]


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
    ok = dict(batch=3, n=n, a=np.zeros(la, dtype=dtype), off_a=off_a, lda=n, w=np.zeros(lw), off_w=off_w, z=np.zeros(la, dtype=dtype),
              off_z=off_a, ldz=n)
    bad = [dict(batch=-1), dict(batch="x"), dict(n=None), dict(a=None), dict(off_a=None), dict(lda=None), dict(w=None),
           dict(off_w=None), dict(z=None), dict(off_z=None), dict(ldz=None), dict(mode="X"), dict(mode="C"), dict(n=[4, -1, 6]),
           dict(lda=[3, 0, 6]), dict(off_a=[0, -1, 16]), dict(off_w=[-1, 4, 4]), dict(off_z=[0, 16, -16]), dict(ldz=[4, 0, 5]),
           dict(n=[4, 0]), dict(lda=[4, 0, 6, 6]), dict(n=[4.5, 0.0, 6.0]), dict(off_a="abc")]
    fn = getattr(ee, name)
    for change in bad:
        api._state["last_status"] = 0
        fn(**{**ok, **change})
        assert api.last_status() == -2, change
        err = capsys.readouterr().err
        assert err.count("\n") == 1 and f"{name}: invalid arguments" in err, change
    assert name in dir(ee)


def test_python_wrapper_rejects_bad_arguments_before_the_library(monkeypatch, capsys):
    wrapper_refusals("eigen_s_vbatch", np.float64, monkeypatch, capsys)


def test_ragged_offsets():
    from eigenexa_amd import layout

    off, total = layout.ragged_offsets([3, 0, 5, 1])
    assert off.dtype == np.int64 and off.tolist() == [0, 9, 9, 34] and total == 35
    off, total = layout.ragged_offsets([3, 0, 5, 1], ld=[4, 2, 8, 1], gap=2)
    assert off.tolist() == [0, 14, 16, 58] and total == 61
    off, total = layout.ragged_offsets([3, 0, 5, 1], ld=1)
    assert off.tolist() == [0, 3, 3, 8] and total == 9
    off, total = layout.ragged_offsets([])
    assert off.tolist() == [] and total == 0
    with pytest.raises(ValueError):
        layout.ragged_offsets([3, -1])
    with pytest.raises(ValueError):
        layout.ragged_offsets([3, 1], gap=-1)


def test_fortran_module_binds_the_vbatch_entries():
    src = open(os.path.join(ROOT, "eigenexa_amd", "fortran", "eigen_libs_mod.F90")).read()
    for which, kind in (("s", r"real\(8\)"), ("h", r"complex\(8\)")):
        assert f'bind(C, name="eigx_{which}_vbatch")' in src
        assert re.search(rf"public :: eigen_{which}_vbatch\b", src)
        m = re.search(rf"subroutine eigen_{which}_vbatch\(batch, n, a, ia, lda, w, iw, z, iz, ldz, mode, info\)(.*?)"
                      rf"end subroutine eigen_{which}_vbatch", src, flags=re.S)
        assert m
        body = m.group(1)
        assert re.search(kind + r", intent\(inout\), contiguous :: a\(:\)", body)
        assert re.search(r"integer\(8\), intent\(in\) :: ia\(\*\), iw\(\*\), iz\(\*\)", body)
        assert re.search(r"character\(\*\), intent\(in\), optional :: mode", body)
        assert re.search(r"integer, intent\(out\), optional :: info\(\*\)", body)
        # the 1-based start indices become 0-based offsets
        for i, o in (("ia", "off_a"), ("iw", "off_w"), ("iz", "off_z")):
            assert re.search(rf"{o} = {i}\(1:nb\) - 1", body)
        assert re.search(rf"eigx_{which}_vbatch\(batch, n, a, off_a, lda, w, off_w, z, off_z, ldz, md, info\)", body)
