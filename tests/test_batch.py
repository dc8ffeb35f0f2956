"""Batched small symmetric eigensolves (eigen_s_batch, an EXTENSION: the reference solves one matrix per call): one kernel
launch, one workgroup per matrix with the matrix in LDS (Householder tridiagonalisation + implicit QL), n <= 128; larger n
falls back to eigen_s matrix by matrix.  GPU tests are marked; the CPU tests at the end check the ctypes table, the Python
wrapper's argument checks, the Fortran binding and tune key 21."""
import ctypes as C
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
FLANG = os.environ.get("FC", "/opt/rocm/lib/llvm/bin/flang")
GUARD = -7.25
BAD_ARG, NONFINITE = -2, -5


def _dev():
    import torch

    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ matrices
# (tools/gpu_frame_dump.py imports _families for its batch section)
def _families(n, seed=0):
    """random symmetric, Frank, three clusters Q D Q^T, graded by 1e-12 across rows and columns, Wilkinson, identity, zero,
    diagonal -- and a second random matrix"""
    from eigenexa_amd import layout

    rng = np.random.default_rng(1000 + 17 * n + seed)
    i = np.arange(n)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    D = np.array([-1.0, 0.5, 2.0])[i % 3] + 1e-10 * rng.random(n)
    clustered = (Q * D) @ Q.T
    g = 10.0 ** (-12.0 * i / max(n - 1, 1))
    R = rng.standard_normal((n, n))
    graded = g[:, None] * (R + R.T) * g[None, :]
    wilk = np.diag(np.abs((n - 1) / 2.0 - i)) + np.diag(np.ones(max(n - 1, 0)), 1)[:n, :n] + np.diag(np.ones(max(n - 1, 0)), -1)[:n, :n]
    mats = [layout.random_symmetric(n, seed=5 + n + seed), layout.frank(n), 0.5 * (clustered + clustered.T), graded, wilk,
            np.eye(n), np.zeros((n, n)), np.diag(rng.standard_normal(n)), layout.random_symmetric(n, seed=77 + n + seed) - 1.0]
    return [np.ascontiguousarray(M, dtype=np.float64) for M in mats]


class Batch:
    """device buffers of one call: a with NaN in the strict lower triangles, the padding rows and the gaps; w, z and info
    prefilled with a guard"""

    def __init__(self, mats, lda=None, stride_a=None, ldz=None, ldw=None, stride_z=None):
        import torch

        self.mats = mats
        self.n = n = mats[0].shape[0]
        self.batch = b = len(mats)
        self.lda = n + 3 if lda is None else lda
        self.ldz = n + 1 if ldz is None else ldz
        self.ldw = n + 2 if ldw is None else ldw
        self.stride_a = self.lda * n + 5 if stride_a is None else stride_a
        self.stride_z = self.ldz * n + 7 if stride_z is None else stride_z
        self.a_host = self.image()
        self.a = torch.from_numpy(self.a_host).to(_dev())
        self.w = torch.full((self.ldw * b,), GUARD, dtype=torch.float64, device=_dev())
        self.z = torch.full((self.stride_z * b,), GUARD, dtype=torch.float64, device=_dev())
        self.info = torch.full((b,), 77, dtype=torch.int32, device=_dev())

    def image(self):
        n = self.n
        buf = np.full(self.stride_a * self.batch, np.nan)
        for k, M in enumerate(self.mats):
            v = buf[k * self.stride_a:k * self.stride_a + self.lda * n].reshape(n, self.lda)   # v[j, i] = a(i, j)
            v[:, :n] = np.where(np.tri(n, dtype=bool), M.T, np.nan)
        return buf

    def refill(self):
        import torch

        self.a.copy_(torch.from_numpy(self.a_host))
        self.w.fill_(GUARD)
        self.z.fill_(GUARD)
        self.info.fill_(77)

    def run(self, lib, mode=b"A", info=True, z=True):
        return lib.eigx_s_batch_dev(self.n, self.batch, self.a.data_ptr(), self.lda, self.stride_a, self.w.data_ptr(), self.ldw,
                                    self.z.data_ptr() if z else None, self.ldz, self.stride_z, mode,
                                    self.info.data_ptr() if info else None)

    def results(self, want_z=True):
        """w (batch, n), Z (batch, n, n) with Z[k][:, j] the j-th eigenvector, info; asserts that the guards survived"""
        n, b = self.n, self.batch
        w = self.w.cpu().numpy().reshape(b, self.ldw)
        assert (w[:, n:] == GUARD).all(), "w beyond n was touched"
        zb = self.z.cpu().numpy().reshape(b, self.stride_z)
        assert (zb[:, self.ldz * n:] == GUARD).all(), "the gaps between the eigenvector matrices were touched"
        zz = zb[:, :self.ldz * n].reshape(b, n, self.ldz)
        assert (zz[:, :, n:] == GUARD).all(), "rows of z beyond n were touched"
        if not want_z:
            assert (zz == GUARD).all(), "z was touched"
        return w[:, :n].copy(), np.transpose(zz[:, :, :n], (0, 2, 1)).copy(), self.info.cpu().numpy()


def _gates(A, w, Z):
    """layout.accuracy_metrics; for the zero matrix, whose residual gate ||A Z - Z W||_F < 768 n eps ||A||_F = 0 leaves no
    room, w = 0 exactly is asked instead"""
    from eigenexa_amd import layout

    if not A.any():
        assert (w == 0.0).all()
        return 0.0, layout.accuracy_metrics(np.eye(A.shape[0]), np.ones(A.shape[0]), Z)[1]
    return layout.accuracy_metrics(A, w, Z)


def _check_matrix(A, w, Z=None, tag=""):
    """eigenvalues against numpy.linalg.eigvalsh to 1e-12 max(1, max|w|), ascending, and both gates"""
    wr = np.linalg.eigvalsh(A)
    tol = 1e-12 * max(1.0, np.abs(wr).max())
    werr = np.abs(w - wr).max()
    assert (np.diff(w) >= 0).all(), tag
    res = orth = 0.0
    if Z is not None:
        res, orth = _gates(A, w, Z)
    print(f"  {tag}: |w - w_lapack| = {werr:.2e} (tol {tol:.2e}), residual {res:.3e}, orthogonality {orth:.3e}")
    assert werr <= tol, tag
    assert res < GATE_RES and orth < GATE_ORTH, tag
    return res, orth


# ------------------------------------------------------------------------------------------------ 1. sizes and families
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 5, 17, 32, 33, 64, 65, 127, 128])
def test_sizes_and_families(gpu_lib, n):
    B = Batch(_families(n))
    assert B.run(gpu_lib) == 0
    w, Z, info = B.results()
    assert (info == 0).all()
    worst = [0.0, 0.0]
    for k, A in enumerate(B.mats):
        r, o = _check_matrix(A, w[k], Z[k], f"n={n} matrix {k}")
        worst = [max(worst[0], r), max(worst[1], o)]
    print(f"n={n}: worst residual {worst[0]:.3e}, worst orthogonality {worst[1]:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [96, 97])
def test_class_boundary_96(gpu_lib, n):
    """the kernel is instantiated for n <= 32, 64, 96 and 128: both sides of the one boundary the sizes above leave out"""
    from eigenexa_amd import layout

    mats = [layout.random_symmetric(n, seed=n), layout.frank(n), _families(n)[3]]
    B = Batch(mats)
    assert B.run(gpu_lib) == 0
    w, Z, info = B.results()
    assert (info == 0).all()
    for k, A in enumerate(mats):
        _check_matrix(A, w[k], Z[k], f"n={n} matrix {k}")


@pytest.mark.gpu
def test_more_workgroups_than_the_card_holds(gpu_lib):
    """batch = 1500 at n = 17: every matrix is checked"""
    n, nb = 17, 1500
    fam = _families(n)
    rng = np.random.default_rng(3)
    mats = []
    for k in range(nb):
        if k % 10 == 9:
            mats.append(fam[(k // 10) % len(fam)])
        else:
            R = rng.standard_normal((n, n))
            mats.append(R + R.T)
    B = Batch(mats)
    assert B.run(gpu_lib) == 0
    w, Z, info = B.results()
    assert (info == 0).all()
    wr = np.linalg.eigvalsh(np.stack(mats))
    tol = 1e-12 * np.maximum(1.0, np.abs(wr).max(axis=1))
    assert (np.abs(w - wr).max(axis=1) <= tol).all()
    eps = np.finfo(np.float64).eps
    Am = np.stack(mats)
    anorm = np.linalg.norm(Am, axis=(1, 2))
    res = np.linalg.norm(Am @ Z - Z * w[:, None, :], axis=(1, 2))
    orth = np.linalg.norm(np.transpose(Z, (0, 2, 1)) @ Z - np.eye(n), axis=(1, 2)) / (n * eps)
    zero = anorm == 0.0
    assert (res[zero] == 0.0).all()
    resg = res[~zero] / (n * eps * anorm[~zero])
    print(f"batch {nb}, n={n}: worst residual {resg.max():.3e}, worst orthogonality {orth.max():.3e}")
    assert resg.max() < GATE_RES and orth.max() < GATE_ORTH


# ------------------------------------------------------------------------------------------------ 2. mode 'N'
@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 33, 80, 100])
def test_mode_n_matches_mode_a(gpu_lib, n):
    B = Batch(_families(n))
    assert B.run(gpu_lib) == 0
    wa, _, _ = B.results()
    B.refill()
    assert B.run(gpu_lib, mode=b"N", z=False) == 0
    wn, _, info = B.results(want_z=False)
    assert (info == 0).all()
    for k in range(B.batch):
        assert np.abs(wn[k] - wa[k]).max() <= 1e-12 * max(1.0, np.abs(wa[k]).max())
        _check_matrix(B.mats[k], wn[k], None, f"mode N n={n} matrix {k}")


# ------------------------------------------------------------------------------------------------ 3. scale
@pytest.mark.gpu
@pytest.mark.parametrize("n", [20, 90])
def test_scales_in_one_batch(gpu_lib, n):
    """copies of one matrix scaled by 1e120, 1 and 1e-120: each is scaled by its own max|a|"""
    from eigenexa_amd import layout

    A0 = layout.random_symmetric(n, seed=4)
    wr = np.linalg.eigvalsh(A0)
    B = Batch([A0 * 1e120, A0, A0 * 1e-120])
    assert B.run(gpu_lib) == 0
    w, Z, info = B.results()
    assert (info == 0).all()
    for k, f in enumerate((1e120, 1.0, 1e-120)):
        werr = np.abs(w[k] / f - wr).max() / np.abs(wr).max()
        res, orth = layout.accuracy_metrics(A0, w[k] / f, Z[k])
        print(f"  scale {f:g}: |w - w_lapack| / max|w| = {werr:.2e}, residual {res:.3e}, orthogonality {orth:.3e}")
        assert werr <= 1e-12 and res < GATE_RES and orth < GATE_ORTH


# ------------------------------------------------------------------------------------------------ 4. failures are local
@pytest.mark.gpu
def test_failures_are_local(gpu_lib):
    from eigenexa_amd import layout

    n = 33
    mats = [layout.random_symmetric(n, seed=60 + k) for k in range(5)]
    mats[1][4, 20] = mats[1][20, 4] = np.nan
    mats[3][0, 32] = mats[3][32, 0] = np.inf
    B = Batch(mats)
    assert B.run(gpu_lib) == NONFINITE
    w, Z, info = B.results()
    assert info.tolist() == [0, NONFINITE, 0, NONFINITE, 0]
    for k in (1, 3):
        assert np.isnan(w[k]).all() and (Z[k] == GUARD).all()
    for k in (0, 2, 4):
        _check_matrix(mats[k], w[k], Z[k], f"matrix {k} beside failed ones")


def errinfo_case():
    """three 5 x 5 matrices, a NaN in the upper triangle of the second (tests/test_vbatch.py uses them too)"""
    from eigenexa_amd import layout

    mats = [layout.random_symmetric(5, seed=40 + k) for k in range(3)]
    mats[1][1, 3] = mats[1][3, 1] = np.nan
    return mats


def errinfo_after(lib):
    err = C.c_int64(77)
    assert lib.eigx_get_errinfo(C.byref(err)) == 0
    return err.value


# errinfo after a call in which one matrix failed, as the library before the shared host frame (csrc/batch_frame.hip) returned it
# on a GPU: the kernel's first-failure word sets -1, the loop above the cutoff leaves the 0 the call began with (the table of
# DESIGN section 8h)
ERRINFO_AFTER_FAILURE = {"kernel": -1, "loop": 0}


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["kernel", "loop"])
def test_errinfo_after_a_failed_matrix(gpu_lib, route):
    """device form; route "loop": key 21 = 4, so that n = 5 goes matrix by matrix through eigx_s_dev"""
    B = Batch(errinfo_case())
    old = gpu_lib.eigx_tune(21, 4) if route == "loop" else None
    try:
        rc = B.run(gpu_lib)
        err = errinfo_after(gpu_lib)
    finally:
        if old is not None:
            assert gpu_lib.eigx_tune(21, old) == 4
    w, Z, info = B.results()
    print(f"eigx_s_batch_dev, {route}: status {rc}, info {info.tolist()}, errinfo {err}")
    assert rc == NONFINITE and info.tolist() == [0, NONFINITE, 0]
    assert np.isnan(w[1]).all() and np.isfinite(w[[0, 2]]).all()
    assert err == ERRINFO_AFTER_FAILURE[route]


# ------------------------------------------------------------------------------------------------ 5. position independence
@pytest.mark.gpu
def test_position_independence_and_reproducibility(gpu_lib):
    n, nb = 40, 40
    fam = _families(n)
    rng = np.random.default_rng(8)
    mats = [fam[k] if k < len(fam) else (lambda R: R + R.T)(rng.standard_normal((n, n))) for k in range(nb)]
    B = Batch(mats)
    assert B.run(gpu_lib) == 0
    w1, Z1, _ = B.results()
    B.refill()
    assert B.run(gpu_lib) == 0
    w2, Z2, _ = B.results()
    assert (w1 == w2).all() and (Z1 == Z2).all()
    for k in range(nb):
        S = Batch([mats[k]])
        assert S.run(gpu_lib) == 0
        ws, Zs, _ = S.results()
        assert (ws[0] == w1[k]).all() and (Zs[0] == Z1[k]).all(), k


# ------------------------------------------------------------------------------------------------ 6. fallback
@pytest.mark.gpu
def test_fallback_is_eigen_s(gpu_lib):
    """key 21 = 32: n = 40 goes through eigx_s_dev matrix by matrix, bit for bit; default key: n = 130"""
    import torch
    from eigenexa_amd import layout

    n = 40
    mats = [layout.random_symmetric(n, seed=90 + k) for k in range(3)]
    B = Batch(mats)
    old = gpu_lib.eigx_tune(21, 32)
    try:
        assert old == 128
        assert B.run(gpu_lib) == 0
    finally:
        assert gpu_lib.eigx_tune(21, old) == 32
    w, Z, info = B.results()
    assert (info == 0).all()
    for k in range(3):
        S = Batch([mats[k]])
        assert gpu_lib.eigx_s_dev(n, n, S.a.data_ptr(), S.lda, S.w.data_ptr(), S.z.data_ptr(), S.ldz, 48, 128, b"A") == 0
        ws, Zs, _ = S.results()
        assert (ws[0] == w[k]).all() and (Zs[0] == Z[k]).all(), k
        _check_matrix(mats[k], w[k], Z[k], f"fallback n={n} matrix {k}")
    n = 130
    mats = [layout.random_symmetric(n, seed=95), layout.frank(n)]
    B = Batch(mats)
    assert B.run(gpu_lib) == 0
    w, Z, info = B.results()
    assert (info == 0).all()
    for k in range(2):
        _check_matrix(mats[k], w[k], Z[k], f"fallback n={n} matrix {k}")
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 7. host and device forms
@pytest.mark.gpu
def test_host_and_device_forms_agree(gpu_lib):
    import eigenexa_amd as ee
    from eigenexa_amd import api

    n, nb = 33, 5
    mats = _families(n)[:nb]
    B = Batch(mats)
    assert B.run(gpu_lib) == 0
    wd, Zd, _ = B.results()
    lda, ldz = n + 3, n + 1
    a = np.full((lda, n, nb), np.nan, order="F")
    for k in range(nb):
        a[:n, :, k] = np.where(np.tri(n, dtype=bool).T, mats[k], np.nan)
    z = np.full((ldz, n, nb), GUARD, order="F")
    w = np.full((n, nb), GUARD, order="F")
    info = np.full(nb, 77, dtype=np.int32)
    ee.eigen_s_batch(n, nb, a, lda, w, z, ldz, info=info)
    assert api.last_status() == 0 and (info == 0).all()
    assert (z[n:] == GUARD).all()
    for k in range(nb):
        assert (w[:, k] == wd[k]).all() and (z[:n, :, k] == Zd[k]).all()
    # the torch route of the wrapper, mode 'N'
    B.refill()
    ee.eigen_s_batch(n, nb, B.a, B.lda, B.w, None, 0, mode="N", stride_a=B.stride_a, ldw=B.ldw)
    assert api.last_status() == 0
    wn, _, _ = B.results(want_z=False)
    assert np.abs(wn - wd).max() <= 1e-12 * max(1.0, np.abs(wd).max())
    # a failed matrix in the host form: its z stays as it was
    for k in range(nb):
        a[:n, :, k] = np.where(np.tri(n, dtype=bool).T, mats[k], np.nan)
    a[1, 2, 2] = np.inf
    z[:] = GUARD
    ee.eigen_s_batch(n, nb, a, lda, w, z, ldz, info=info)
    assert api.last_status() == NONFINITE and info.tolist() == [0, 0, NONFINITE, 0, 0]
    assert np.isnan(w[:, 2]).all() and (z[:, :, 2] == GUARD).all()
    for k in (0, 1, 3, 4):
        assert (w[:, k] == wd[k]).all() and (z[:n, :, k] == Zd[k]).all()


# ------------------------------------------------------------------------------------------------ 8. arguments
@pytest.mark.gpu
def test_arguments(gpu_lib):
    from eigenexa_amd import layout

    n, nb = 12, 3
    mats = [layout.random_symmetric(n, seed=k) for k in range(nb)]
    B = Batch(mats)
    pa, pw, pz, pi = B.a.data_ptr(), B.w.data_ptr(), B.z.data_ptr(), B.info.data_ptr()
    lda, ldw, ldz, sa, sz = B.lda, B.ldw, B.ldz, B.stride_a, B.stride_z
    ah = B.a_host.copy()
    wh = np.full(ldw * nb, GUARD)
    zh = np.full(sz * nb, GUARD)
    ih = np.full(nb, 77, dtype=np.int32)
    for fn, (a, w, z, i) in ((gpu_lib.eigx_s_batch_dev, (pa, pw, pz, pi)),
                             (gpu_lib.eigx_s_batch, (ah.ctypes.data, wh.ctypes.data, zh.ctypes.data, ih.ctypes.data))):
        assert fn(0, nb, a, lda, sa, w, ldw, z, ldz, sz, b"A", i) == BAD_ARG
        assert fn(-2, nb, a, lda, sa, w, ldw, z, ldz, sz, b"A", i) == BAD_ARG
        assert fn(n, -1, a, lda, sa, w, ldw, z, ldz, sz, b"A", i) == BAD_ARG
        assert fn(n, nb, a, n - 1, sa, w, ldw, z, ldz, sz, b"A", i) == BAD_ARG
        assert fn(n, nb, a, lda, sa, w, n - 1, z, ldz, sz, b"A", i) == BAD_ARG
        assert fn(n, nb, a, lda, lda * n - 1, w, ldw, z, ldz, sz, b"A", i) == BAD_ARG
        assert fn(n, nb, a, lda, sa, w, ldw, z, n - 1, sz, b"A", i) == BAD_ARG
        assert fn(n, nb, a, lda, sa, w, ldw, z, ldz, ldz * n - 1, b"A", i) == BAD_ARG
        assert fn(n, nb, a, lda, sa, w, ldw, None, ldz, sz, b"A", i) == BAD_ARG
        for mode in (b"X", b"S", b"C", b"V"):
            assert fn(n, nb, a, lda, sa, w, ldw, z, ldz, sz, mode, i) == BAD_ARG
        assert fn(n, 0, a, lda, sa, w, ldw, z, ldz, sz, b"A", i) == 0          # empty batch
        assert fn(n, 0, None, lda, 0, None, ldw, None, ldz, 0, b"A", None) == 0
    B.results()                                                                  # nothing was touched ...
    assert (B.z.cpu().numpy() == GUARD).all() and (B.w.cpu().numpy() == GUARD).all() and (B.info.cpu().numpy() == 77).all()
    assert np.array_equal(B.a.cpu().numpy(), B.a_host, equal_nan=True)
    assert np.array_equal(ah, B.a_host, equal_nan=True) and (wh == GUARD).all() and (zh == GUARD).all() and (ih == 77).all()
    # one matrix: the strides are not looked at; lower-case mode; ldz and stride_z ignored in mode 'N'; info = NULL
    S = Batch(mats[:1])
    assert gpu_lib.eigx_s_batch_dev(n, 1, S.a.data_ptr(), S.lda, 0, S.w.data_ptr(), S.ldw, S.z.data_ptr(), S.ldz, 0, b"a", None) == 0
    w, Z, info = S.results()
    assert (info == 77).all()
    _check_matrix(mats[0], w[0], Z[0], "one matrix, strides 0, info NULL")
    assert B.run(gpu_lib, info=False) == 0
    w, Z, info = B.results()
    assert (info == 77).all()
    for k in range(nb):
        _check_matrix(mats[k], w[k], Z[k], f"info NULL matrix {k}")
    B.refill()
    assert gpu_lib.eigx_s_batch_dev(n, nb, pa, lda, sa, pw, ldw, None, 0, 0, b"n", None) == 0
    wn, _, _ = B.results(want_z=False)
    assert np.abs(wn - w).max() <= 1e-12 * max(1.0, np.abs(w).max())
    t = (C.c_double * 16)()
    gpu_lib.eigx_get_timers(t)
    assert t[0] > 0.0 and all(t[q] == 0.0 for q in range(1, 16))


# ------------------------------------------------------------------------------------------------ 9. two ranks
@pytest.mark.gpu
def test_batch_refuses_several_ranks():
    """two ranks on the one card: both entries return EIGX_ERR_BAD_ARG on both ranks and the processes exit cleanly"""
    import socket

    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = os.path.join(os.path.dirname(__file__), "batch_worker.py")
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
def test_fortran_batch_caller(gpu_lib, tmp_path):
    """a Fortran program calls eigen_s_batch of module eigen_libs_mod on four scaled Frank matrices of n = 30"""
    if not os.path.exists(FLANG):
        pytest.skip("no flang")
    lib = os.path.join(ROOT, "eigenexa_amd", "lib")
    mod = os.path.join(ROOT, "eigenexa_amd", "fortran", "eigen_libs_mod.F90")
    src = os.path.join(ROOT, "tests", "fortran", "batch_caller.F90")
    subprocess.check_call([FLANG, "-cpp", "-O2", "-c", mod, "-o", "eigen_libs_mod.o"], cwd=tmp_path)
    subprocess.check_call([FLANG, "-cpp", "-O2", "-c", src, "-o", "batch_caller.o"], cwd=tmp_path)
    subprocess.check_call([FLANG, "-o", "batch_caller", "batch_caller.o", "eigen_libs_mod.o", f"-L{lib}", "-leigenexa_amd",
                           f"-Wl,-rpath,{lib}"], cwd=tmp_path)
    out = subprocess.run([str(tmp_path / "batch_caller")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"max rel eigenvalue error\s*=\s*([0-9.eEdD+-]+)", out.stdout)
    assert m, out.stdout
    assert float(m.group(1).replace("D", "E").replace("d", "e")) < GOLD["gates"]["frank_rel_err"]


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", ["eigx_s_batch", "eigx_s_batch_dev"])
def test_header_prototypes_match_the_ctypes_table(name):
    from eigenexa_amd import _lib

    params = _prototype(name)
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is C.c_int and len(argtypes) == len(params) == 12
    for p, t in zip(params, argtypes):
        if p.startswith("char "):
            assert t is C.c_char
        elif "*" in p:
            assert t is C.c_void_p
        elif p.startswith("int64_t "):
            assert t is C.c_int64
        else:
            assert p.startswith("int ") and t is C.c_int
    names = [p.split()[-1].replace("_dev", "") for p in params]
    assert names == ["n", "batch", "a", "lda", "stride_a", "w", "ldw", "z", "ldz", "stride_z", "mode", "info"]
    txt = open(os.path.join(ROOT, "include", "eigenexa_amd.h")).read()
    assert re.search(r"#define\s+EIGX_BATCH_NMAX\s+128\b", txt)


def test_python_wrapper_rejects_bad_arguments_before_the_library(monkeypatch, capsys):
    """every EIGX_ERR_BAD_ARG case of the contract: status -2 and one warning line each, without loading the library"""
    import eigenexa_amd as ee
    from eigenexa_amd import _lib, api

    def boom():
        raise AssertionError("the library must not be touched")

    monkeypatch.setattr(_lib, "load", boom)
    n, nb = 6, 3
    a = np.zeros((n, n, nb), order="F")
    z = np.zeros((n, n, nb), order="F")
    w = np.zeros((n, nb), order="F")
    ok = dict(n=n, batch=nb, a=a, lda=n, w=w, z=z, ldz=n)
    bad = [dict(n=0), dict(n=-1), dict(batch=-1), dict(lda=n - 1), dict(ldw=n - 1), dict(stride_a=n * n - 1), dict(ldz=n - 1),
           dict(stride_z=n * n - 1), dict(z=None), dict(mode="X"), dict(mode="C"), dict(n="x")]
    for change in bad:
        api._state["last_status"] = 0
        ee.eigen_s_batch(**{**ok, **change})
        assert api.last_status() == -2, change
        err = capsys.readouterr().err
        assert err.count("\n") == 1 and "eigen_s_batch: invalid arguments" in err
    assert "eigen_s_batch" in dir(ee)


def test_fortran_module_binds_the_batch_entry():
    src = open(os.path.join(ROOT, "eigenexa_amd", "fortran", "eigen_libs_mod.F90")).read()
    assert 'bind(C, name="eigx_s_batch")' in src
    assert re.search(r"public :: eigen_s_batch\b", src)
    assert re.search(r"subroutine eigen_s_batch\(n, batch, a, lda, w, z, ldz, mode, info\)", src)


def test_tune_key_21_refuses_values_outside_its_range():
    """key 21 (no GPU needed): default 128, takes 0 .. 128; anything else is refused with -1 and changes nothing"""
    from eigenexa_amd import _lib

    lib = _lib.load()
    assert lib.eigx_tune(21, 32) == 128
    assert lib.eigx_tune(21, 129) == -1 and lib.eigx_tune(21, -1) == -1 and lib.eigx_tune(21, 1 << 20) == -1
    assert lib.eigx_tune(21, 0) == 32             # the refused values changed nothing
    assert lib.eigx_tune(21, 128) == 0
    assert lib.eigx_tune(21, 128) == 128
