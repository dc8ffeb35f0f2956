"""Every path of the fp64 GEMM dispatcher (csrc/gemm_f64.hip: dgemm_dev, dgemm_gather_batch_dev) through the test interface of
include/eigenexa_amd_gemm_lab.h, against alpha op(A) op(B) + beta C computed on the host in numpy.longdouble.

Bound, element-wise and derived (u = 2^-53), for any summation order:

    |got - ref|_ij <= 2 (K + 4) u ( |alpha| (|op(A)| |op(B)|)_ij + |beta| |C|_ij )

K fused accumulations, the roundings of beta/alpha, of its product with C and of the final alpha *, a factor 2 for the
higher-order terms; where the right-hand side is 0 the result is exact.  Operands are graded: randn entries, rows of op(A) and
columns of op(B) scaled by random powers of two in 2^+-20, C at the scale of its row times its column.  Leading dimensions are
larger than the row counts; every padding element (A, B and C) holds random bits and C's must come back bit for bit.  The
kernel is chosen with eigx_tune(0, v): 1 = the block kernel gemm_f64_kernel only, 3 = the ring kernel gemm2_kernel wherever
its preconditions hold.  Each test prints one GEMM-MARGIN line (pytest -s) with the worst err / bound it saw
(profiles/gemm_paths_margins.log).  The CPU tests at the end hold _lib.LAB_SIGNATURES against the header and the size of the
tri_mode 2 launch against the count from the definition (a launch that is too large changes no result)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAB_HEADER = os.path.join(ROOT, "include", "eigenexa_amd_gemm_lab.h")

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "the reference needs an extended long double (x86)"
U = LD(2.0) ** -53
TN_MAX = 0x7FFFFFFF
G1 = (1, 0, 1, 0)
OPS = [("N", "N"), ("N", "T"), ("T", "N"), ("T", "T")]
ALPHA_BETA = [(-1.0, 1.0), (0.3, -0.7), (1.0, 0.0)]
K_EDGES = [1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 33]
BAD_ARG = -2

gpu = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ host side
def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def _random_bits(rng, size):
    return rng.integers(-2 ** 63, 2 ** 63 - 1, size=size, dtype=np.int64, endpoint=True).view(np.float64)


def _view(buf, off, rows, cols, ld):
    """element (i, j) of the column-major block at buf[off + i + j ld]"""
    return np.lib.stride_tricks.as_strided(buf[off:], (rows, cols), (buf.itemsize, buf.itemsize * ld))


def _store(rng, X, ld, off=0, fill=None):
    """a flat buffer that holds X column-major with leading dimension ld from element off; everything else is random bits
    (or ``fill``)"""
    rows, cols = X.shape
    size = off + ld * cols + 3
    buf = _random_bits(rng, size) if fill is None else np.full(size, fill)
    _view(buf, off, rows, cols, ld)[...] = X
    return buf


def _graded(rng, M, N, K, ra=None):
    """graded op(A), op(B), C; ``ra``: the row scales of an op(A) that several products share (C follows its rows)"""
    ra = np.ldexp(1.0, rng.integers(-20, 21, M)) if ra is None else ra
    cb = np.ldexp(1.0, rng.integers(-20, 21, N))
    opA = rng.standard_normal((M, K)) * ra[:, None]
    opB = rng.standard_normal((K, N)) * cb[None, :]
    Cm = rng.standard_normal((M, N)) * ra[:, None] * cb[None, :]
    return opA, opB, Cm


class _Product:
    """op(A) op(B) in long double and |op(A)| |op(B)|, computed once and shared by every (alpha, beta) and kernel"""

    def __init__(self, opA, opB):
        self.K = opA.shape[1]
        if self.K:
            self.P = opA.astype(LD) @ opB.astype(LD)
            self.absP = np.abs(opA) @ np.abs(opB)
        else:
            self.P = np.zeros((opA.shape[0], opB.shape[1]), LD)
            self.absP = np.zeros(self.P.shape)

    def ref_bound(self, alpha, beta, C0, k=None):
        """(ref, bound); alpha == 0 does not reference the product, beta == 0 does not reference C"""
        k = self.K if k is None else k
        ref = np.zeros(self.P.shape, LD)
        mag = np.zeros(self.P.shape, LD)
        if alpha != 0.0:
            ref += LD(alpha) * self.P
            mag += abs(alpha) * self.absP.astype(LD)
        if beta != 0.0:
            ref += LD(beta) * C0.astype(LD)
            mag += abs(beta) * np.abs(C0).astype(LD)
        return ref, 2 * (k + 4) * U * mag


class _Checker:
    """one launch's C buffer before and after: products are checked against the bound where they must be updated, and
    finish() requires every other element of the buffer to hold its bits"""

    def __init__(self, got, before):
        self.got, self.before = got, before
        self.touched = np.zeros(got.size, bool)
        self.margin = 0.0

    def product(self, off, M, N, ld, ref, bound, upd=None):
        tv = np.lib.stride_tricks.as_strided(self.touched[off:], (M, N), (1, ld))
        sel = np.ones((M, N), bool) if upd is None else upd
        tv[sel] = True
        g = _view(self.got, off, M, N, ld)[sel]
        err = np.abs(g.astype(LD) - ref[sel])
        bnd = bound[sel]
        bad = ~(err <= bnd)   # a NaN in the result fails
        pos = bnd > 0
        assert not bad.any(), f"{int(bad.sum())} elements beyond the bound; err/bound up to " \
                              f"{float(np.nanmax(err[pos] / bnd[pos])) if pos.any() else float('inf')}"
        if pos.any():
            self.margin = max(self.margin, float((err[pos] / bnd[pos]).max()))
        return self

    def finish(self):
        keep = ~self.touched
        assert np.array_equal(_bits(self.got[keep]), _bits(self.before[keep])), "an element outside the update changed"
        return self.margin


def _report(case, what, margin):
    print(f"GEMM-MARGIN case {case} {what}: worst err/bound = {margin:.3f}")
    assert margin <= 1.0


# ------------------------------------------------------------------------------------------------ device side
def _up(buf):
    import torch

    return torch.from_numpy(_bits(buf).copy()).to("cuda:0")


def _down(t):
    return t.cpu().numpy().view(np.float64)


def _up_map(m):
    import torch

    return torch.from_numpy(np.ascontiguousarray(m, dtype=np.int32)).to("cuda:0")


def _ptr(t, off=0):
    return t.data_ptr() + t.element_size() * off if t is not None else None


class _variant:
    """eigx_tune(0, v) for the body, the previous value put back afterwards"""

    def __init__(self, lib, v):
        self.lib, self.v = lib, v

    def __enter__(self):
        self.old = self.lib.eigx_tune(0, self.v)

    def __exit__(self, *exc):
        self.lib.eigx_tune(0, self.old)


def _gemm(lib, opa, opb, M, N, K, alpha, dA, lda, dB, ldb, beta, dC, ldc, offA=0, offB=0, offC=0, tri=0, grid=G1, batch=1,
          sA=0, sB=0, sC=0, batch2=1, sA2=0, sB2=0, sC2=0, tn=(0, TN_MAX), ka=None, kb=None, expect=0):
    rc = lib.eigx_dgemm_ex_dev(opa.encode(), opb.encode(), M, N, K, alpha, _ptr(dA, offA), lda, _ptr(dB, offB), ldb, beta,
                               _ptr(dC, offC), ldc, tri, grid[0], grid[1], grid[2], grid[3], batch, sA, sB, sC, batch2, sA2,
                               sB2, sC2, tn[0], tn[1], _ptr(ka), _ptr(kb))
    assert rc == expect
    return rc


def _stored(op, X):
    """the stored matrix whose op() is X"""
    return X if op == "N" else X.T


def _pad_ld(rows, extra, even=True):
    ld = rows + extra
    if even and ld & 1:
        ld += 1
    return ld


def _full_case(lib, seed, opa, opb, M, N, K, variants, alpha_beta=ALPHA_BETA, lda=None, ldb=None, ldc=None, offA=0, offB=0,
               offC=0, c_nan=False, ab_nan=False, exact_beta_c=False):
    """one full-mode product under every variant and (alpha, beta): the result within the bound, everything else of C's
    buffer bit for bit; returns the worst err / bound"""
    rng = np.random.default_rng(seed)
    opA, opB, Cm = _graded(rng, M, N, K)
    sa, sb = _stored(opa, opA), _stored(opb, opB)
    lda = _pad_ld(sa.shape[0], 2) if lda is None else lda
    ldb = _pad_ld(sb.shape[0], 4) if ldb is None else ldb
    ldc = _pad_ld(M, 6) if ldc is None else ldc
    prod = _Product(opA, opB)
    if ab_nan:
        sa, sb = np.full(sa.shape, np.nan), np.full(sb.shape, np.nan)
    bufA, bufB = _store(rng, sa, lda, offA), _store(rng, sb, ldb, offB)
    bufC = _store(rng, Cm, ldc, offC)
    if c_nan:
        bufC[:] = np.nan
    dA, dB = _up(bufA), _up(bufB)
    worst = 0.0
    for v in variants:
        with _variant(lib, v):
            for alpha, beta in alpha_beta:
                assert not (c_nan and beta != 0.0)
                dC = _up(bufC)
                _gemm(lib, opa, opb, M, N, K, alpha, dA, lda, dB, ldb, beta, dC, ldc, offA, offB, offC)
                got = _down(dC)
                ref, bound = prod.ref_bound(alpha, beta, Cm)
                worst = max(worst, _Checker(got, bufC).product(offC, M, N, ldc, ref, bound).finish())
                g = _view(got, offC, M, N, ldc)
                assert np.isfinite(g).all()
                if exact_beta_c and beta != 0.0:
                    assert np.array_equal(_bits(g), _bits(beta * Cm))
                elif exact_beta_c:
                    assert not g.any()
    return worst


# ------------------------------------------------------------------------------------------------ 1. K edges
@gpu
@pytest.mark.parametrize("opa,opb", OPS)
def test_k_edges(gpu_lib, opa, opb):
    """(131, 130) with K across the ring's 8-deep slab, its S - 1 = 3 prologue slabs and the block kernel's 16-deep slab, both
    kernels (odd K with a k-contiguous operand falls back to the block kernel under variant 3)"""
    worst = 0.0
    for K in K_EDGES:
        worst = max(worst, _full_case(gpu_lib, 100 + K, opa, opb, 131, 130, K, (1, 3)))
    _report(1, f"k_edges {opa}{opb}", worst)


# ------------------------------------------------------------------------------------------------ 2. shapes
@gpu
@pytest.mark.parametrize("opa,opb", OPS)
@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 3, 2), (129, 257, 16), (1100, 300, 18), (256, 128, 18), (512, 128, 18),
                                   (257, 131, 18)],
                         ids=lambda s: "x".join(map(str, s)))
def test_shapes(gpu_lib, shape, opa, opb):
    """both kernels on: M < 2 (falls back under variant 3); (1100, 300): nine tile rows of the ring, a partial second row
    group and an uneven XCD share; the block kernel's 64-wide tiles with ntiles % 8 == 0 (256, 128: the XCD remap with one
    tile per XCD, where it is the identity; 512, 128: two per XCD) and without (257, 131)"""
    M, N, K = shape
    worst = _full_case(gpu_lib, 200 + M + N, opa, opb, M, N, K, (1, 3))
    _report(2, f"shape {M}x{N}x{K} {opa}{opb}", worst)


@gpu
@pytest.mark.parametrize("opa,opb", [("N", "T"), ("T", "N")])
@pytest.mark.parametrize("M", [2048, 2049])
def test_block_kernel_wide_tiles(gpu_lib, M, opa, opb):
    """the block kernel's 128-wide tiles need >= 192 tiles: (2048, 1536) has 192 and takes the ntiles % 8 == 0 remap,
    (2049, 1536) has 204 and does not.  Variant 1 only; the largest shapes of the file."""
    worst = _full_case(gpu_lib, 300 + M, opa, opb, M, 1536, 18, (1,), alpha_beta=[(0.3, -0.7)])
    _report(2, f"wide tiles {M}x1536x18 {opa}{opb}", worst)


# ------------------------------------------------------------------------------------------------ 3. ring fall-back
FALLBACKS = [
    ("odd_lda", "N", "T", 18, dict(lda_odd=True)),
    ("odd_ldb", "N", "T", 18, dict(ldb_odd=True)),
    ("odd_ldc", "N", "T", 18, dict(ldc_odd=True)),
    ("odd_lda_T", "T", "N", 18, dict(lda_odd=True)),
    ("base_a_8_bytes", "N", "T", 18, dict(offA=1)),
    ("base_b_8_bytes", "N", "T", 18, dict(offB=1)),
    ("base_c_8_bytes", "N", "T", 18, dict(offC=1)),
    ("odd_k_T_a", "T", "T", 17, {}),
    ("odd_k_N_b", "N", "N", 17, {}),
]


@gpu
@pytest.mark.parametrize("name,opa,opb,K,how", FALLBACKS, ids=[f[0] for f in FALLBACKS])
def test_ring_fallback(gpu_lib, name, opa, opb, K, how):
    """variant 3 with one precondition of the ring kernel broken at a time (gemm2_ok): the answer is still right"""
    M, N = 257, 131
    rows_a = M if opa == "N" else K
    rows_b = K if opb == "N" else N
    kw = dict(offA=how.get("offA", 0), offB=how.get("offB", 0), offC=how.get("offC", 0))
    kw["lda"] = _pad_ld(rows_a, 2) + (1 if how.get("lda_odd") else 0)
    kw["ldb"] = _pad_ld(rows_b, 4) + (1 if how.get("ldb_odd") else 0)
    kw["ldc"] = _pad_ld(M, 6) + (1 if how.get("ldc_odd") else 0)
    worst = _full_case(gpu_lib, 400 + len(name), opa, opb, M, N, K, (3, 1), **kw)
    _report(3, f"fallback {name}", worst)


@gpu
@pytest.mark.parametrize("opb", ["N", "T"])
def test_ring_fallback_lda_below_k(gpu_lib, opb):
    """'T' A with lda < K: the columns of the stored A overlap (op(A)(m, k) = a[k + m lda]), which the ring kernel's
    k-contiguous image does not serve"""
    M, N, K, lda = 131, 130, 18, 16
    rng = np.random.default_rng(77)
    a = rng.standard_normal(K + (M - 1) * lda + 2)
    opA = np.array(np.lib.stride_tricks.as_strided(a, (M, K), (8 * lda, 8)))
    _, opB, Cm = _graded(rng, M, N, K)
    sb = _stored(opb, opB)
    ldb, ldc = _pad_ld(sb.shape[0], 4), _pad_ld(M, 6)
    bufB, bufC = _store(rng, sb, ldb), _store(rng, Cm, ldc)
    prod = _Product(opA, opB)
    dA, dB = _up(a), _up(bufB)
    worst = 0.0
    for v in (3, 1):
        with _variant(gpu_lib, v):
            for alpha, beta in ALPHA_BETA:
                dC = _up(bufC)
                _gemm(gpu_lib, "T", opb, M, N, K, alpha, dA, lda, dB, ldb, beta, dC, ldc)
                ref, bound = prod.ref_bound(alpha, beta, Cm)
                worst = max(worst, _Checker(_down(dC), bufC).product(0, M, N, ldc, ref, bound).finish())
    _report(3, f"fallback lda<K T{opb}", worst)


# ------------------------------------------------------------------------------------------------ 4. beta == 0
@gpu
@pytest.mark.parametrize("opa,opb", OPS)
def test_beta_zero_does_not_read_c(gpu_lib, opa, opb):
    """C and its padding hold NaN (the library passes beta = 0 into pool workspace): the result is finite and within the
    bound, the padding still holds its NaN bits.  Both kernels, 64-wide and (tri-free) ring tiles."""
    worst = 0.0
    for M, N, K in [(131, 130, 18), (257, 131, 7)]:
        worst = max(worst, _full_case(gpu_lib, 500 + M, opa, opb, M, N, K, (1, 3), alpha_beta=[(1.0, 0.0), (-0.3, 0.0)],
                                      c_nan=True))
    _report(4, f"beta=0 {opa}{opb}", worst)


def _gather_operands(rng, M, N, K, extra_a=7, extra_b=5):
    """graded op(A), op(B) scattered over distinct random columns of a wider A (M x (K + extra_a)) and B (N x (K + extra_b));
    the other columns hold random bits"""
    opA, opB, Cm = _graded(rng, M, N, K)
    ka = rng.permutation(K + extra_a)[:K]
    kb = rng.permutation(K + extra_b)[:K]
    lda, ldb = _pad_ld(M, 2), _pad_ld(N, 4)
    bufA = _random_bits(rng, lda * (K + extra_a) + 3)
    bufB = _random_bits(rng, ldb * (K + extra_b) + 3)
    _view(bufA, 0, M, K + extra_a, lda)[:, ka] = opA
    _view(bufB, 0, N, K + extra_b, ldb)[:, kb] = opB.T
    return opA, opB, Cm, ka, kb, bufA, lda, bufB, ldb


def _gather_case(lib, seed, M, N, K, alpha_beta, c_nan=False):
    rng = np.random.default_rng(seed)
    opA, opB, Cm, ka, kb, bufA, lda, bufB, ldb = _gather_operands(rng, M, N, K)
    ldc = _pad_ld(M, 6)
    bufC = _store(rng, Cm, ldc)
    if c_nan:
        bufC[:] = np.nan
    prod = _Product(opA, opB)
    dA, dB, dka, dkb = _up(bufA), _up(bufB), _up_map(ka), _up_map(kb)
    worst = 0.0
    for v in (1, 3):
        with _variant(lib, v):
            for alpha, beta in alpha_beta:
                dC = _up(bufC)
                _gemm(lib, "N", "T", M, N, K, alpha, dA, lda, dB, ldb, beta, dC, ldc, ka=dka, kb=dkb)
                got = _down(dC)
                ref, bound = prod.ref_bound(alpha, beta, Cm)
                worst = max(worst, _Checker(got, bufC).product(0, M, N, ldc, ref, bound).finish())
                assert np.isfinite(_view(got, 0, M, N, ldc)).all()
    return worst


@gpu
def test_beta_zero_does_not_read_c_gather(gpu_lib):
    """the same for the gather form (dc.hip's Qb), both kernels"""
    worst = max(_gather_case(gpu_lib, 550 + K, 333, 210, K, [(1.0, 0.0)], c_nan=True) for K in (9, 24))
    _report(4, "beta=0 gather", worst)


# ------------------------------------------------------------------------------------------------ 5. alpha == 0, K == 0
@gpu
@pytest.mark.parametrize("opa,opb", OPS)
def test_alpha_zero_and_k_zero(gpu_lib, opa, opb):
    """alpha == 0: beta C bit for bit (zeros at beta == 0), with finite A and B and with NaN-filled ones -- A and B are not
    referenced, as in BLAS (dgemm_dev runs alpha == 0 as K = 0).  K == 0: beta C within the bound (K = 0: four roundings)."""
    M, N, K = 131, 130, 17
    worst = 0.0
    for ab_nan in (False, True):
        worst = max(worst, _full_case(gpu_lib, 600, opa, opb, M, N, K, (1, 3), alpha_beta=[(0.0, 1.5), (0.0, 0.0)],
                                      ab_nan=ab_nan, exact_beta_c=True))
    worst = max(worst, _full_case(gpu_lib, 601, opa, opb, M, N, 0, (1, 3)))
    worst = max(worst, _full_case(gpu_lib, 602, opa, opb, M, N, 0, (1, 3), alpha_beta=[(1.0, 0.0)], c_nan=True))
    _report(5, f"alpha=0 / K=0 {opa}{opb}", worst)


@gpu
def test_alpha_zero_gather_and_tri(gpu_lib):
    """alpha == 0 through the gather form (NaN in every column of A and B, mapped or not) and through tri_mode 1 (only the
    upper tiles are scaled by beta)"""
    rng = np.random.default_rng(610)
    M, N, K = 131, 130, 17
    opA, opB, Cm, ka, kb, bufA, lda, bufB, ldb = _gather_operands(rng, M, N, K)
    bufA[:] = np.nan
    bufB[:] = np.nan
    ldc = _pad_ld(M, 6)
    bufC = _store(rng, Cm, ldc)
    dA, dB, dka, dkb = _up(bufA), _up(bufB), _up_map(ka), _up_map(kb)
    for v in (1, 3):
        with _variant(gpu_lib, v):
            dC = _up(bufC)
            _gemm(gpu_lib, "N", "T", M, N, K, 0.0, dA, lda, dB, ldb, 1.5, dC, ldc, ka=dka, kb=dkb)
            got = _down(dC)
            assert np.array_equal(_bits(_view(got, 0, M, N, ldc)), _bits(1.5 * Cm))
            _Checker(got, bufC).product(0, M, N, ldc, (1.5 * Cm).astype(LD), np.zeros((M, N), LD)).finish()
            n = 257
            Cq = rng.standard_normal((n, n))
            ldq = _pad_ld(n, 3)
            bufQ = _store(rng, Cq, ldq)
            dQ, dT = _up(bufQ), _up(np.full(ldq * K + 3, np.nan))
            _gemm(gpu_lib, "N", "T", n, n, K, 0.0, dT, ldq, dT, ldq, 1.5, dQ, ldq, tri=1)
            t = np.arange(n) // 128
            upd = t[:, None] <= t[None, :]
            _Checker(_down(dQ), bufQ).product(0, n, n, ldq, (1.5 * Cq).astype(LD), np.zeros((n, n), LD), upd).finish()
    _report(5, "alpha=0 gather / tri", 0.0)


# ------------------------------------------------------------------------------------------------ 6. batches
def _batch_case(lib, seed, opa, opb, M, N, K, batch, batch2, gap, variants, share_a=(), alpha_beta=ALPHA_BETA):
    """batch x batch2 products; ``gap`` doubles between consecutive operands (its parity is the strides' parity);
    share_a: the batch levels (1, 2) whose stride on A is 0, so that the products along that level share op(A).  Returns the
    worst err / bound; memory between the C blocks keeps its bits."""
    rng = np.random.default_rng(seed)
    ra, ca = (M, K) if opa == "N" else (K, M)
    rb, cb = (K, N) if opb == "N" else (N, K)
    lda, ldb, ldc = _pad_ld(ra, 2), _pad_ld(rb, 4), _pad_ld(M, 6)
    sA, sB, sC = lda * ca + gap, ldb * cb + gap, ldc * N + gap
    sA2, sB2, sC2 = batch * sA + 2 * gap, batch * sB + 2 * gap, batch * sC + 2 * gap
    if 1 in share_a:
        sA, sA2 = 0, lda * ca + 2 * gap
    if 2 in share_a:
        sA2 = 0
    total = lambda s, s2, one: (batch - 1) * s + (batch2 - 1) * s2 + one + 3
    bufA = _random_bits(rng, total(sA, sA2, lda * ca))
    bufB = _random_bits(rng, total(sB, sB2, ldb * cb))
    bufC = _random_bits(rng, total(sC, sC2, ldc * N))
    prods = {}
    for j in range(batch2):
        for i in range(batch):
            src = (0 if 1 in share_a else i, 0 if 2 in share_a else j)   # the product whose op(A) this one reads
            if src == (i, j):
                opA, opB, Cm = _graded(rng, M, N, K)
            else:
                opA = prods[src][0]
                _, opB, Cm = _graded(rng, M, N, K, ra=np.ldexp(1.0, np.frexp(np.abs(opA).max(axis=1))[1]))
            _view(bufA, i * sA + j * sA2, ra, ca, lda)[...] = _stored(opa, opA)
            _view(bufB, i * sB + j * sB2, rb, cb, ldb)[...] = _stored(opb, opB)
            _view(bufC, i * sC + j * sC2, M, N, ldc)[...] = Cm
            prods[(i, j)] = (opA, opB, Cm)
    for key, (opA, opB, Cm) in list(prods.items()):
        prods[key] = (_Product(opA, opB), Cm)
    dA, dB = _up(bufA), _up(bufB)
    worst = 0.0
    for v in variants:
        with _variant(lib, v):
            for alpha, beta in alpha_beta:
                dC = _up(bufC)
                _gemm(lib, opa, opb, M, N, K, alpha, dA, lda, dB, ldb, beta, dC, ldc, batch=batch, sA=sA, sB=sB, sC=sC,
                      batch2=batch2, sA2=sA2, sB2=sB2, sC2=sC2)
                chk = _Checker(_down(dC), bufC)
                for (i, j), (prod, Cm) in prods.items():
                    ref, bound = prod.ref_bound(alpha, beta, Cm)
                    chk.product(i * sC + j * sC2, M, N, ldc, ref, bound)
                worst = max(worst, chk.finish())
    return worst


@gpu
@pytest.mark.parametrize("opa,opb", [("N", "N"), ("T", "N"), ("N", "T")])
@pytest.mark.parametrize("shape", [(70, 66, 34), (130, 5, 9)], ids=lambda s: "x".join(map(str, s)))
def test_batches(gpu_lib, shape, opa, opb):
    """batch = 3, batch2 = 2 with non-zero strides on all three operands, as tri.hip (the pairs of a level: batch along the
    diagonal, batch2 over the outer blocks), ztri.hip through zgemm_planes, and trbak.hip (Gram partials, T levels) launch
    them: even strides under both kernels, odd strides (variant 3 falls back).  The zero-stride (shared operand) patterns
    are those of test_batches_shared_a."""
    M, N, K = shape
    worst = _batch_case(gpu_lib, 700 + M, opa, opb, M, N, K, 3, 2, 10, (1, 3))
    worst = max(worst, _batch_case(gpu_lib, 701 + M, opa, opb, M, N, K, 3, 2, 11, (3,)))
    _report(6, f"batches {M}x{N}x{K} {opa}{opb}", worst)


# (name, opa, opb, batch, batch2, levels that share A)
SHARED_A = [
    ("herm_675", "T", "N", 2, 1, (1,)),
    ("herm_882", "T", "N", 3, 2, (2,)),
    ("herm_1139", "T", "N", 1, 2, (2,)),
    ("herm_1108", "N", "T", 4, 1, (1,)),
]


@gpu
@pytest.mark.parametrize("name,opa,opb,batch,batch2,share", SHARED_A, ids=[c[0] for c in SHARED_A])
@pytest.mark.parametrize("shape", [(70, 66, 34), (130, 5, 10)], ids=lambda s: "x".join(map(str, s)))
def test_batches_shared_a(gpu_lib, shape, name, opa, opb, batch, batch2, share):
    """the zero-stride patterns that callers use, all on A and all in herm.hip, under both kernels (even K and even strides,
    so that variant 3 takes the ring kernel):
      herm.hip:675  (h_bt_block)  'T','N', batch = 2 over the planes Zr / Zi, strideA = 0: the stacked reflectors Vs are shared;
      herm.hip:882  (T factors, one GPU)  'T','N', batch = nblk with non-zero strides, batch2 = 2 with strideA2 = 0: the block's
                    Vr or Vi against both planes;
      herm.hip:1139 (T factors, several ranks)  'T','N', batch = 1 with strides 0, 0, 0 and batch2 = 2 with strideA2 = 0;
      herm.hip:1108 (the multi-rank Hermitian trailing update)  'N','T', batch = gfull >= 3 with strideA = 0: the panels P1 / P2
                    are shared by the rank's tile columns, beta = 1.
    No caller passes a zero stride on B or C where the batch level has more than one product.  The products that share op(A)
    have their own op(B) and C, C at the scale of the shared rows."""
    M, N, K = shape
    worst = _batch_case(gpu_lib, 750 + M + len(name), opa, opb, M, N, K, batch, batch2, 10, (1, 3), share_a=share)
    _report(6, f"shared A {name} {M}x{N}x{K} {opa}{opb}", worst)


# ------------------------------------------------------------------------------------------------ 7. tri_mode 1, block kernel
def _tile_mask(M, N, grid, tn=(0, TN_MAX)):
    """the header's definition: tile (tm, tn) is updated iff tm 128 Px + px <= min(tn 128 + 127, N - 1) Py + py and
    tn_lo <= tn < tn_hi; expanded to elements"""
    Px, px, Py, py = grid
    tm = np.arange(M) // 128
    tc = np.arange(N) // 128
    grow_min = tm * 128 * Px + px
    gcol_max = np.minimum(tc * 128 + 127, N - 1) * Py + py
    return (grow_min[:, None] <= gcol_max[None, :]) & ((tc >= tn[0]) & (tc < tn[1]))[None, :]


@gpu
@pytest.mark.parametrize("odd_ld", [False, True], ids=["even_ld", "odd_ld"])
@pytest.mark.parametrize("n", [700, 1000, 1153])
def test_tri_mode_1_block_kernel(gpu_lib, n, odd_ld):
    """variant 1, K = 18; n = 1000 has eight tile columns (the XCD-dealt order of tiles_n % 8 == 0).  Tiles tm <= tn within
    the bound, tiles strictly below bit for bit; with NaN in the strictly lower tiles the upper result is bit-identical."""
    K = 18
    rng = np.random.default_rng(800 + n)
    opA, opB, Cm = _graded(rng, n, n, K)
    ld = _pad_ld(n, 2) + (1 if odd_ld else 0)
    bufA, bufB, bufC = _store(rng, opA, ld), _store(rng, opB.T, ld), _store(rng, Cm, ld)
    upd = _tile_mask(n, n, G1)
    Cn = np.where(upd, Cm, np.nan)
    bufN = bufC.copy()
    _view(bufN, 0, n, n, ld)[...] = Cn
    prod = _Product(opA, opB)
    dA, dB = _up(bufA), _up(bufB)
    worst = 0.0
    with _variant(gpu_lib, 1):
        for alpha, beta in ALPHA_BETA:
            dC = _up(bufC)
            _gemm(gpu_lib, "N", "T", n, n, K, alpha, dA, ld, dB, ld, beta, dC, ld, tri=1)
            got = _down(dC)
            ref, bound = prod.ref_bound(alpha, beta, Cm)
            worst = max(worst, _Checker(got, bufC).product(0, n, n, ld, ref, bound, upd).finish())
            dN = _up(bufN)
            _gemm(gpu_lib, "N", "T", n, n, K, alpha, dA, ld, dB, ld, beta, dN, ld, tri=1)
            gn = _down(dN)
            assert np.array_equal(_bits(_view(gn, 0, n, n, ld)[upd]), _bits(_view(got, 0, n, n, ld)[upd]))
            _Checker(gn, bufN).product(0, n, n, ld, ref, bound, upd).finish()
    _report(7, f"tri 1 block kernel n={n} ld={ld}", worst)


# ------------------------------------------------------------------------------------------------ 8. tri_mode 2
GRIDS = [(1, 0, 1, 0), (2, 1, 1, 0), (1, 0, 3, 2), (2, 1, 4, 3), (4, 0, 2, 1), (3, 2, 3, 0)]
# (1153, 1300): ten tile rows = two row groups of the ring's active-region launch (rg_h = 8), M != N both ways with
# (1300, 257) and (130, 1153); (257, 257) on grid (1, 0, 1, 0) has a tile whose first row equals its last column (256)
TRI2_SHAPES = [(1153, 1300), (1300, 257), (130, 1153), (2, 2), (257, 257)]


@gpu
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "grid" + "_".join(map(str, g)))
@pytest.mark.parametrize("shape", TRI2_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tri_mode_2(gpu_lib, shape, grid):
    """the local block of a 2-D cyclic distribution, both kernels, 'N','T' with K = 18 (band_reduce.hip) and, on the grid
    (2, 1, 4, 3), 'N','N' (hgev.hip's SUMMA step).  Windows (0, max), (t, max), (0, t) for t in {1, 3, tiles_n} and an
    empty one: the tiles of the header's definition are within the bound over the whole tile, every other tile and all
    padding keep their bits (also where nothing is active).  (t, max) then (0, t) equals the full window bit for bit (the
    look-ahead split of the reduction); NaN in the tiles that must not be touched leaves the others bit-identical."""
    M, N = shape
    K = 18
    rng = np.random.default_rng(900 + M + N)
    opA, opB, Cm = _graded(rng, M, N, K)
    tiles_n = (N + 127) // 128
    windows = [(0, TN_MAX), (2, 2)]
    for t in (1, 3, tiles_n):
        for w in ((t, TN_MAX), (0, t)):
            if w not in windows:
                windows.append(w)
    lda, ldc = _pad_ld(M, 2), _pad_ld(M, 6)
    bufA, bufC = _store(rng, opA, lda), _store(rng, Cm, ldc)
    prod = _Product(opA, opB)
    dA = _up(bufA)
    worst = 0.0
    for opb in ("T", "N") if grid == (2, 1, 4, 3) else ("T",):
        sb = _stored(opb, opB)
        ldb = _pad_ld(sb.shape[0], 4)
        dB = _up(_store(rng, sb, ldb))
        for v in (1, 3):
            with _variant(gpu_lib, v):
                for alpha, beta in [(-1.0, 1.0), (0.3, -0.7)]:
                    ref, bound = prod.ref_bound(alpha, beta, Cm)
                    full = None
                    for w in windows if alpha == -1.0 else windows[:1]:
                        upd = _tile_mask(M, N, grid, w)
                        dC = _up(bufC)
                        _gemm(gpu_lib, "N", opb, M, N, K, alpha, dA, lda, dB, ldb, beta, dC, ldc, tri=2, grid=grid, tn=w)
                        got = _down(dC)
                        worst = max(worst, _Checker(got, bufC).product(0, M, N, ldc, ref, bound, upd).finish())
                        if w == (0, TN_MAX):
                            full, full_upd = got, upd
                    if alpha != -1.0:
                        continue
                    for t in (1, 3):
                        dC = _up(bufC)
                        _gemm(gpu_lib, "N", opb, M, N, K, alpha, dA, lda, dB, ldb, beta, dC, ldc, tri=2, grid=grid, tn=(t, TN_MAX))
                        _gemm(gpu_lib, "N", opb, M, N, K, alpha, dA, lda, dB, ldb, beta, dC, ldc, tri=2, grid=grid, tn=(0, t))
                        assert np.array_equal(_bits(_down(dC)), _bits(full))
                    bufN = bufC.copy()
                    _view(bufN, 0, M, N, ldc)[~full_upd] = np.nan
                    dN = _up(bufN)
                    _gemm(gpu_lib, "N", opb, M, N, K, alpha, dA, lda, dB, ldb, beta, dN, ldc, tri=2, grid=grid)
                    gn = _down(dN)
                    _Checker(gn, bufN).product(0, M, N, ldc, ref, bound, full_upd).finish()
                    assert np.array_equal(_bits(_view(gn, 0, M, N, ldc)[full_upd]), _bits(_view(full, 0, M, N, ldc)[full_upd]))
    _report(8, f"tri 2 {M}x{N} grid {grid}", worst)


# ------------------------------------------------------------------------------------------------ 9. gather
@gpu
@pytest.mark.parametrize("K", K_EDGES)
def test_gather_single(gpu_lib, K):
    """one gather product (333, 210) through both kernels, maps = distinct random columns of wider A and B"""
    _report(9, f"gather K={K}", _gather_case(gpu_lib, 1000 + K, 333, 210, K, ALPHA_BETA))


@gpu
def test_gather_table(gpu_lib):
    """dgemm_gather_batch_dev: five products of different shapes in one launch, each with its own offsets into shared A, B, C
    and into the two maps; C is NaN-filled (the launch has beta = 0) and the memory between the C blocks keeps its bits.
    A sixth entry has K = 0: dc.hip's table builder emits one when every kept column of a merge is of the bottom type
    (ktop = 0) or of the top type (kbot = 0) -- add() drops only rows <= 0 -- and the block is then zeroed."""
    rng = np.random.default_rng(1100)
    shapes = [(1, 1, 1), (64, 64, 16), (65, 130, 17), (200, 3, 33), (5, 70, 40), (37, 21, 0)]
    lda, ldb, ldc = 400, 300, 206
    ncol_a, ncol_b = 64, 60
    bufA = _random_bits(rng, lda * ncol_a + 300)
    bufB = _random_bits(rng, ldb * ncol_b + 300)
    mapA, mapB = np.zeros(400, np.int32), np.zeros(400, np.int32)
    entries, blocks = [], []
    offC, offK = 3, 2
    # A and B are shared: every product reads the same columns region from its own row offset, so the graded operands are
    # written once for all -- rows [offA, offA + M) of A's mapped columns, rows [offB, offB + N) of B's -- with disjoint rows
    rowA, rowB = 0, 0
    for M, N, K in shapes:
        opA, opB, Cm = _graded(rng, M, N, K)
        ka = rng.permutation(ncol_a)[:K]
        kb = rng.permutation(ncol_b)[:K]
        _view(bufA, rowA, M, ncol_a, lda)[:, ka] = opA
        _view(bufB, rowB, N, ncol_b, ldb)[:, kb] = opB.T
        mapA[offK:offK + K] = ka
        mapB[offK + 1:offK + 1 + K] = kb
        entries += [M, N, K, rowA, rowB, offC, offK, offK + 1]
        blocks.append((offC, M, N, _Product(opA, opB)))
        rowA += M + 1
        rowB += N + 1
        offC += ldc * N + 5
        offK += K + 3
    assert rowA <= lda and rowB <= ldb and offK + 1 <= mapA.size
    bufC = np.full(offC + 3, np.nan)
    tab = np.array(entries, np.int64)
    dA, dB, dka, dkb = _up(bufA), _up(bufB), _up_map(mapA), _up_map(mapB)
    dC = _up(bufC)
    rc = gpu_lib.eigx_dgemm_gather_table_dev(len(shapes), tab.ctypes.data, _ptr(dA), lda, _ptr(dB), ldb, _ptr(dC), ldc,
                                             _ptr(dka), _ptr(dkb))
    assert rc == 0
    chk = _Checker(_down(dC), bufC)
    for off, M, N, prod in blocks:
        ref, bound = prod.ref_bound(1.0, 0.0, None)
        chk.product(off, M, N, ldc, ref, bound)
        assert np.isfinite(_view(chk.got, off, M, N, ldc)).all()
    _report(9, "gather table", chk.finish())


@gpu
def test_lab_entries_refuse_what_the_dispatcher_aborts_on(gpu_lib):
    """a gather without 'N','T' and both maps, a tri_mode or grid position out of range, a bad table: EIGX_ERR_BAD_ARG and C
    untouched"""
    rng = np.random.default_rng(1200)
    M = N = K = 8
    buf = _store(rng, rng.standard_normal((M, K)), 10)
    dA, dB, dC = _up(buf), _up(buf), _up(buf)
    m = _up_map(np.arange(K))
    args = (gpu_lib, "N", "T", M, N, K, 1.0, dA, 10, dB, 10, 0.0, dC, 10)
    _gemm(*args, ka=m, expect=BAD_ARG)
    _gemm(*args, kb=m, expect=BAD_ARG)
    for opa, opb in (("T", "T"), ("N", "N"), ("T", "N")):
        _gemm(gpu_lib, opa, opb, *args[3:], ka=m, kb=m, expect=BAD_ARG)
    _gemm(*args, tri=3, expect=BAD_ARG)
    _gemm(*args, tri=-1, expect=BAD_ARG)
    for grid in ((0, 0, 1, 0), (2, 2, 1, 0), (1, 0, 2, -1), (1, 0, 2, 2)):
        _gemm(*args, tri=2, grid=grid, expect=BAD_ARG)
    tab = np.array([4, 4, -1, 0, 0, 0, 0, 0], np.int64)
    assert gpu_lib.eigx_dgemm_gather_table_dev(1, tab.ctypes.data, _ptr(dA), 10, _ptr(dB), 10, _ptr(dC), 10, _ptr(m),
                                               _ptr(m)) == BAD_ARG
    assert gpu_lib.eigx_dgemm_gather_table_dev(-1, None, _ptr(dA), 10, _ptr(dB), 10, _ptr(dC), 10, _ptr(m), _ptr(m)) == BAD_ARG
    assert gpu_lib.eigx_dgemm_gather_table_dev(0, None, _ptr(dA), 10, _ptr(dB), 10, _ptr(dC), 10, _ptr(m), _ptr(m)) == 0
    assert np.array_equal(_bits(_down(dC)), _bits(buf))


# ------------------------------------------------------------------------------------------------ CPU
LAB_ENTRIES = {"eigx_dgemm_ex_dev": 30, "eigx_dgemm_gather_table_dev": 10, "eigx_dgemm_tri2_launch_tiles": 8}


@pytest.mark.parametrize("name", sorted(LAB_ENTRIES))
def test_lab_header_prototypes_match_the_ctypes_table(monkeypatch, name):
    """the entries are declared in include/eigenexa_amd_gemm_lab.h and mirrored by _lib.LAB_SIGNATURES: the parser of the
    other header tests, pointed at that file"""
    import c_header
    from eigenexa_amd import _lib

    monkeypatch.setattr(c_header, "HEADER", LAB_HEADER)
    params = c_header.prototype(name)
    restype, argtypes = _lib.LAB_SIGNATURES[name]
    assert restype is C.c_int and len(argtypes) == len(params) == LAB_ENTRIES[name]
    for p, t in zip(params, argtypes):
        if p.startswith("char "):
            assert t is C.c_char
        elif "*" in p:
            assert t is C.c_void_p
        elif p.startswith("int64_t "):
            assert t is C.c_int64
        elif p.startswith("double "):
            assert t is C.c_double
        else:
            assert p.startswith("int ") and t is C.c_int


def test_the_lab_header_is_a_test_interface_of_its_own():
    """eigenexa_amd.h does not include the file and the file says what it is; it declares exactly the entries of the table;
    no name sits in two of the four tables; the loaded library has the entries with these signatures"""
    import c_header
    from eigenexa_amd import _lib

    main = open(os.path.join(ROOT, "include", "eigenexa_amd.h")).read()
    assert "eigenexa_amd_gemm_lab" not in main
    assert "TEST INTERFACE" in open(LAB_HEADER).read()
    old = c_header.HEADER
    try:
        c_header.HEADER = LAB_HEADER
        protos = c_header.all_prototypes()
    finally:
        c_header.HEADER = old
    assert set(protos) == set(_lib.LAB_SIGNATURES) == set(LAB_ENTRIES)
    tables = [_lib.SIGNATURES, _lib.GBATCH_SIGNATURES, _lib.HGBATCH_SIGNATURES, _lib.LAB_SIGNATURES]
    for i, a in enumerate(tables):
        for b in tables[i + 1:]:
            assert not set(a) & set(b)
    assert not set(LAB_ENTRIES) & set(c_header.all_prototypes())   # nor does the public header declare them
    lib = _lib.load()
    for name, (restype, argtypes) in _lib.LAB_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes


def _launch_tiles_from_the_definition(M, N, grid, tn):
    """row groups of 8 tile rows; group q takes the tile columns of the window at which its first tile row is updated"""
    tiles_m, tiles_n = (M + 127) // 128, (N + 127) // 128
    active = _tile_mask(M, N, grid, tn)[::128][:, ::128]   # per tile: every element of a tile has its tile's value
    assert active.shape == (tiles_m, tiles_n)
    return sum(min(8, tiles_m - q) * int(active[q].sum()) for q in range(0, tiles_m, 8))


def test_tri_mode_2_launch_size_matches_the_definition():
    """the ring kernel's tri_mode 2 launch (host arithmetic: tri2_c0 with its reciprocal division, the window clip, the row
    groups) has exactly the tiles of the definition: a first column that is too small would only cost workgroups that return
    at once, which no result shows -- here it does.  Shapes and grids of test_tri_mode_2, and grids at which the first
    global row of the second row group, seen from the rank's first column, is a multiple of 128 Py (the reciprocal's edge:
    x / Py exact and a multiple of the tile width) or one short of it."""
    from eigenexa_amd import _lib

    lib = _lib.load()
    grids = GRIDS + [(3, 0, 3, 2), (3, 1, 3, 0), (1, 0, 8, 0), (1, 0, 8, 7), (1, 0, 5, 4), (5, 0, 5, 4), (3, 0, 6, 5),
                     (7, 3, 7, 3), (1, 0, 2, 0), (2, 0, 1, 0), (2, 0, 2, 1)]
    shapes = TRI2_SHAPES + [(1025, 1300), (1024, 1300), (2177, 2200), (2050, 129), (129, 2050)]
    for M, N in shapes:
        tiles_n = (N + 127) // 128
        for grid in grids:
            for tn in [(0, TN_MAX), (2, 2), (1, TN_MAX), (0, 1), (3, TN_MAX), (0, 3), (tiles_n, TN_MAX), (0, tiles_n), (2, 9)]:
                got = lib.eigx_dgemm_tri2_launch_tiles(M, N, grid[0], grid[1], grid[2], grid[3], tn[0], tn[1])
                assert got == _launch_tiles_from_the_definition(M, N, grid, tn), (M, N, grid, tn)
    assert lib.eigx_dgemm_tri2_launch_tiles(300, 300, 2, 2, 1, 0, 0, TN_MAX) == BAD_ARG
    assert lib.eigx_dgemm_tri2_launch_tiles(0, 300, 1, 0, 1, 0, 0, TN_MAX) == 0


def test_the_reference_and_the_tile_rule_on_the_host():
    """the long-double reference resolves what fp64 cannot, and the tile rule gives the block triangle on one rank"""
    a = np.array([[1.0, 2.0 ** -60]])
    b = np.array([[1.0], [1.0]])
    prod = _Product(a, b)
    assert prod.P[0, 0] != LD(1.0) and float(prod.P[0, 0]) == 1.0
    ref, bound = prod.ref_bound(0.0, 0.0, np.full((1, 1), np.nan))
    assert ref[0, 0] == 0 and bound[0, 0] == 0
    m = _tile_mask(257, 300, G1)
    assert m[0, 0] and m[127, 299] and not m[128, 127] and m[256, 256] and not m[256, 255]
    assert not _tile_mask(257, 300, G1, (1, 2))[:, :128].any() and not _tile_mask(257, 300, G1, (1, 2))[:, 256:].any()
    assert re.search(r"int\s+eigx_dgemm_ex_dev", open(LAB_HEADER).read())
