"""KMATH_EIGEN_GEV_RANGE (an EXTENSION: the reference has no Cholesky-route or index-range generalised solver): blocked
Cholesky B = U^T U, triangular solves by block inversion, C = U^-T A U^-1, the index-range solve of C, Z = U^-1 Y.
Matrices and tolerances are those of test_gev_matches_oracle / tests/test_hgev.py: with scale = max(1, max|w_ref|),
eigenvalues to 1e-12 scale, ||A Z - B Z W||_F < 1e-12 scale n, ||Z^T B Z - I||_F < 1e-12 n.  GPU tests are marked; the CPU
tests at the end check the ctypes table, the export and the wrapper's argument checks."""
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
GEVR_SYMBOLS = ["eigx_gev_range", "eigx_gev_range_dev", "eigx_chol_dev", "eigx_trsm_upper_dev", "eigx_gev_reduce_dev"]
STAGE_N = [1, 2, 5, 63, 64, 65, 130, 517, 1100]
NB_KEYS = [64, 128, "default"]


def _dev():
    import torch

    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ inputs, computed once
@functools.lru_cache(maxsize=None)
def _pencil(n, kind="helmert"):
    """A = random_symmetric(n, seed=3); B = the Helmert matrix of test_gev_matches_oracle (cond about 1.2), or
    Q diag(logspace(0, -4, n)) Q^T with a seeded orthogonal Q (cond 1e4).  Read-only."""
    from eigenexa_amd import layout

    A = layout.random_symmetric(n, seed=3)
    if kind == "helmert":
        B = layout.helmert_spectrum_matrix(n, 10)[0] if n > 1 else np.array([[10.0]])
    else:
        Q, _ = np.linalg.qr(np.random.default_rng(11).standard_normal((n, n)))
        B = (Q * np.logspace(0, -4, n)) @ Q.T
        B = (B + B.T) / 2
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


@functools.lru_cache(maxsize=None)
def _reference(n, kind="helmert"):
    import scipy.linalg

    A, B = _pencil(n, kind)
    w = scipy.linalg.eigh(A, B, eigvals_only=True)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _factor(n):
    U = np.linalg.cholesky(_pencil(n)[1]).T.copy()
    U.setflags(write=False)
    return U


def _upper_with_nan(M):
    return np.triu(M) + np.tril(np.full(M.shape, np.nan), -1)


def _to_dev(M, ld):
    """column-major image of M (rows x cols) with leading dimension ld: tensor (cols, ld), t[j, i] = M(i, j)"""
    import torch

    t = torch.zeros(M.shape[1], ld, dtype=torch.float64, device=_dev())
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


@pytest.fixture
def all_sizes(gpu_lib):
    """size rule off (eigx_tune key 17 = 100 %), as in test_range.py: the inner call takes the subset path"""
    old = gpu_lib.eigx_tune(17, 100)
    yield gpu_lib
    gpu_lib.eigx_tune(17, old)


def _windows(n, m):
    """the windows of tests/test_range.py::_windows"""
    mid = max(1, (n - m) // 2)
    return [(1, m), (n - m + 1, n), (mid, mid + m - 1), (n // 3 + 1, n // 3 + 1), (1, n)]


def _gates(A, B, w, Z, wref_window, scale, what):
    n = A.shape[0]
    m = len(w)
    werr = np.abs(w - wref_window).max()
    res = np.linalg.norm(A @ Z - B @ Z * w)
    orth = np.linalg.norm(Z.T @ B @ Z - np.eye(m))
    print(f"  {what}: |w - w_ref| = {werr:.2e} (gate {1e-12 * scale:.2e}), ||AZ - BZW|| = {res:.2e} (gate {1e-12 * scale * n:.2e}), "
          f"||Z^T B Z - I|| = {orth:.2e} (gate {1e-12 * n:.2e})")
    assert werr < 1e-12 * scale
    assert res < 1e-12 * scale * n
    assert orth < 1e-12 * n


# ------------------------------------------------------------------------------------------------ stages
@pytest.mark.gpu
@pytest.mark.parametrize("n", STAGE_N)
def test_cholesky_stage(tri_nb, n):
    """eigx_chol_dev: leading dimension n + 2, NaN below the diagonal; U read from the upper triangle only"""
    B = _pencil(n)[1]
    ld = n + 2
    b = _to_dev(_upper_with_nan(B), ld)
    assert tri_nb.eigx_chol_dev(n, b.data_ptr(), ld) == 0
    U = np.triu(np.nan_to_num(_from_dev(b, n), nan=0.0))
    Uref = _factor(n)
    e1 = np.linalg.norm(U.T @ U - B)
    e2 = np.abs(U - Uref).max()
    print(f"  n={n}: ||U^T U - B|| = {e1:.2e} (gate {1e-12 * n * np.linalg.norm(B):.2e}), max|U - U_ref| = {e2:.2e}")
    assert np.isfinite(np.triu(_from_dev(b, n))).all()
    assert e1 < 1e-12 * n * np.linalg.norm(B)
    assert e2 < 1e-12 * n * np.abs(Uref).max()


@pytest.mark.gpu
def test_cholesky_stage_breakdown(tri_nb):
    """an indefinite B, and a B whose first non-positive pivot lies in the LAST diagonal block: EIGX_ERR_NOT_SPD"""
    from eigenexa_amd import layout

    Bi = layout.random_symmetric(50, seed=4) - 1.0
    b = _to_dev(_upper_with_nan(Bi), 52)
    assert tri_nb.eigx_chol_dev(50, b.data_ptr(), 52) == -7
    B = np.array(_pencil(130)[1])
    B[129, 129] = -1.0
    b = _to_dev(_upper_with_nan(B), 132)
    assert tri_nb.eigx_chol_dev(130, b.data_ptr(), 132) == -7
    b = _to_dev(_upper_with_nan(_pencil(130)[1]), 132)
    assert tri_nb.eigx_chol_dev(130, b.data_ptr(), 132) == 0      # the flag does not stick


@pytest.mark.gpu
@pytest.mark.parametrize("n", STAGE_N)
def test_triangular_solve_stage(tri_nb, n):
    """eigx_trsm_upper_dev, op = none / transpose, nrhs = 1, 7, 64, n; below the diagonal u_dev holds NaN"""
    U = _factor(n)
    ld = n + 2
    u = _to_dev(_upper_with_nan(U), ld)
    rng = np.random.default_rng(5 + n)
    for nrhs in sorted({1, 7, 64, n}):
        R = rng.standard_normal((n, nrhs))
        for trans in ("N", "T"):
            x = _to_dev(R, ld)
            assert tri_nb.eigx_trsm_upper_dev(trans.encode(), n, nrhs, u.data_ptr(), ld, x.data_ptr(), ld) == 0
            X = _from_dev(x, n)
            assert np.isfinite(X).all()
            err = np.linalg.norm((U if trans == "N" else U.T) @ X - R)
            gate = 1e-12 * n * np.linalg.norm(U) * np.linalg.norm(X)
            print(f"  n={n} nrhs={nrhs} op={trans}: ||op(U) X - R|| = {err:.2e} (gate {gate:.2e})")
            assert err < gate
    assert tri_nb.eigx_trsm_upper_dev(b"X", n, 1, u.data_ptr(), ld, u.data_ptr(), ld) == -2


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 65, 517, 1100])
def test_reduction_stage(tri_nb, n):
    """eigx_gev_reduce_dev: ||U^T C U - A||_F < 1e-12 n ||A||_F with C symmetrised from its upper triangle"""
    A = _pencil(n)[0]
    U = _factor(n)
    ld = n + 2
    a = _to_dev(_upper_with_nan(A), ld)
    u = _to_dev(_upper_with_nan(U), ld)
    assert tri_nb.eigx_gev_reduce_dev(n, a.data_ptr(), ld, u.data_ptr(), ld) == 0
    Cu = np.triu(_from_dev(a, n))
    assert np.isfinite(Cu).all()
    Cm = Cu + np.triu(Cu, 1).T
    err = np.linalg.norm(U.T @ Cm @ U - A)
    print(f"  n={n}: ||U^T C U - A|| = {err:.2e} (gate {1e-12 * n * np.linalg.norm(A):.2e})")
    assert err < 1e-12 * n * np.linalg.norm(A)


# ------------------------------------------------------------------------------------------------ whole solves, host API
def _solve_host(A, B, il, iu, mode="A", z_none=False):
    import eigenexa_amd as ee
    from eigenexa_amd import api

    n = A.shape[0]
    m = iu - il + 1
    a = np.asfortranarray(_upper_with_nan(A))
    b = np.asfortranarray(_upper_with_nan(B))
    z = None if z_none else np.full((n, m + 1), 7.0, order="F")   # one guard column
    w = np.full(m + 1, 7.0)
    ee.KMATH_EIGEN_GEV_RANGE(n, il, iu, a, n, b, n, w, z, n, mode=mode)
    assert api.last_status() == 0
    assert w[m] == 7.0
    if z is not None:
        assert (z[:, m] == 7.0).all()
        if mode == "N":
            assert (z == 7.0).all()
    return w[:m], (None if z is None else z[:, :m]), b


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 5, 130, 517])
def test_whole_solve_matches_scipy(all_sizes, n):
    """host API against scipy.linalg.eigh(A, B) on the windows of test_range.py with m = min(n, 24), key 17 = 100"""
    import eigenexa_amd as ee

    A, B = _pencil(n)
    wref = _reference(n)
    scale = max(1.0, np.abs(wref).max())
    m = min(n, 24)
    for il, iu in sorted(set(_windows(n, m))):
        w, Z, b = _solve_host(A, B, il, iu)
        _gates(A, B, w, Z, wref[il - 1:iu], scale, f"n={n} [{il}, {iu}]")
        info = ee.range_info()
        assert info.m == iu - il + 1
        if iu - il + 1 < n:
            assert info.path == 1
        U = np.triu(b)
        assert np.linalg.norm(U.T @ U - B) < 1e-12 * n * np.linalg.norm(B)   # b holds U with B = U^T U
    il, iu = 1, m
    wa, _, _ = _solve_host(A, B, il, iu)
    wn, _, _ = _solve_host(A, B, il, iu, mode="N")
    w0, _, _ = _solve_host(A, B, il, iu, mode="N", z_none=True)
    assert np.abs(wn - wa).max() < 1e-12 * scale and (w0 == wn).all()


@pytest.mark.gpu
def test_whole_solve_default_keys(gpu_lib):
    """default keys at n = 517: the size rule sends the window through the full divide and conquer (path 3)"""
    import eigenexa_amd as ee

    n = 517
    A, B = _pencil(n)
    wref = _reference(n)
    scale = max(1.0, np.abs(wref).max())
    for il, iu in [(1, 24), (200, 260), (1, n)]:
        w, Z, _ = _solve_host(A, B, il, iu)
        assert ee.range_info().path == 3
        _gates(A, B, w, Z, wref[il - 1:iu], scale, f"n={n} [{il}, {iu}] default keys")


@pytest.mark.gpu
@pytest.mark.parametrize("window", [(1, 52), (1, 517)])
def test_ill_conditioned_b(all_sizes, window):
    """B = Q diag(logspace(0, -4, n)) Q^T, cond 1e4: the same gates"""
    n = 517
    A, B = _pencil(n, "cond1e4")
    wref = _reference(n, "cond1e4")
    scale = max(1.0, np.abs(wref).max())
    il, iu = window
    w, Z, _ = _solve_host(A, B, il, iu)
    _gates(A, B, w, Z, wref[il - 1:iu], scale, f"cond 1e4 n={n} [{il}, {iu}]")


@pytest.mark.gpu
def test_agrees_with_kmath_eigen_gev(gpu_lib):
    """the same pencil through KMATH_EIGEN_GEV (two eigen_s solves, three products): eigenvalues to 1e-12 scale, the
    B-orthogonal projector onto the lowest 52 vectors to 1e-10 n (two different methods are compared)"""
    import eigenexa_amd as ee
    from eigenexa_amd import api

    n = 517
    A, B = _pencil(n)
    w1, Z1, _ = _solve_host(A, B, 1, n)
    a = np.asfortranarray(np.triu(A))
    b = np.asfortranarray(np.triu(B))
    Z2 = np.zeros((n, n), order="F")
    w2 = np.zeros(n)
    ee.KMATH_EIGEN_GEV(n, a, n, b, n, w2, Z2, n)
    assert api.last_status() == 0
    scale = max(1.0, np.abs(_reference(n)).max())
    P1 = Z1[:, :52] @ Z1[:, :52].T @ B
    P2 = Z2[:, :52] @ Z2[:, :52].T @ B
    dp = np.linalg.norm(P1 - P2)
    print(f"  |w - w_gev| = {np.abs(w1 - w2).max():.2e} (gate {1e-12 * scale:.2e}), projector difference = {dp:.2e} "
          f"(gate {1e-10 * n:.2e})")
    assert np.abs(w1 - w2).max() < 1e-12 * scale
    assert dp < 1e-10 * n


# ------------------------------------------------------------------------------------------------ device API
@pytest.mark.gpu
def test_device_api(gpu_lib):
    """torch tensors, n = 1200 with ld = n + 2, windows [1, 120] and [1, n]; gates as in
    test_gev_device_api_and_indefinite_b; a repeat call is bit-identical; an odd leading dimension is refused"""
    import torch
    import eigenexa_amd as ee
    from eigenexa_amd import api

    n = 1200
    A, B = _pencil(n)
    ld = n + 2
    results = []
    for il, iu in [(1, 120), (1, n)]:
        m = iu - il + 1
        for rep in range(2):
            a = _to_dev(_upper_with_nan(A), ld)
            b = _to_dev(_upper_with_nan(B), ld)
            z = torch.zeros(m, ld, dtype=torch.float64, device=_dev())
            w = torch.zeros(m, dtype=torch.float64, device=_dev())
            ee.KMATH_EIGEN_GEV_RANGE(n, il, iu, a, ld, b, ld, w, z, ld)
            assert api.last_status() == 0
            results.append((w.cpu().numpy(), _from_dev(z, n)))
        (wa, Za), (wb, Zb) = results[-2:]
        assert (wa == wb).all() and (Za == Zb).all()
        scale = max(1.0, np.abs(wa).max())
        res = np.linalg.norm(A @ Za - B @ Za * wa)
        orth = np.linalg.norm(Za.T @ B @ Za - np.eye(m))
        print(f"  n={n} [{il}, {iu}]: ||AZ - BZW|| = {res:.2e} (gate {1e-12 * scale * n:.2e}), ||Z^T B Z - I|| = {orth:.2e}")
        assert res < 1e-12 * scale * n and orth < 1e-12 * n
        assert (np.diff(wa) >= 0).all()
    wfull = results[-1][0]
    assert np.abs(results[0][0] - wfull[:120]).max() < 1e-12 * max(1.0, np.abs(wfull).max())
    ldo = n + 1
    a = torch.zeros(n, ldo, dtype=torch.float64, device=_dev())
    w = torch.zeros(n, dtype=torch.float64, device=_dev())
    for lds in [(ldo, ld, ld), (ld, ldo, ld), (ld, ld, ldo)]:
        assert gpu_lib.eigx_gev_range_dev(n, 1, 5, a.data_ptr(), lds[0], a.data_ptr(), lds[1], w.data_ptr(), a.data_ptr(),
                                          lds[2], b"A") == -2


@pytest.mark.gpu
def test_gates_at_n4096(gpu_lib):
    """N = 4096, matrices made on the GPU and the three gates computed there (as tests/test_hgev.py does); default keys;
    window [1, 410] and the full one; eigenvalues of the window against those of the full call"""
    import torch
    import eigenexa_amd as ee
    from eigenexa_amd import api

    n = 4096
    dev = _dev()
    g = torch.Generator(device=dev)
    g.manual_seed(4321)
    S = torch.randn(n, n, dtype=torch.float64, device=dev, generator=g)
    A = (S + S.T) / 2
    X = torch.randn(n, n, dtype=torch.float64, device=dev, generator=g)
    B = X @ X.T / n + torch.eye(n, dtype=torch.float64, device=dev)
    B = (B + B.T) / 2
    del S, X
    upper = torch.triu(torch.ones(n, n, dtype=torch.bool, device=dev))
    nan = torch.full((n, n), float("nan"), dtype=torch.float64, device=dev)
    ws = {}
    for il, iu in [(1, n), (1, 410)]:
        m = iu - il + 1
        a = torch.where(upper, A, nan).T.contiguous()
        b = torch.where(upper, B, nan).T.contiguous()
        z = torch.zeros(m, n, dtype=torch.float64, device=dev)
        w = torch.zeros(m, dtype=torch.float64, device=dev)
        ee.KMATH_EIGEN_GEV_RANGE(n, il, iu, a, n, b, n, w, z, n)
        assert api.last_status() == 0
        Z = z.T
        ws[m] = w
        scale = max(1.0, ws[n].abs().max().item())
        res = torch.linalg.norm(A @ Z - (B @ Z) * w[None, :]).item()
        orth = torch.linalg.norm(Z.T @ B @ Z - torch.eye(m, dtype=torch.float64, device=dev)).item()
        print(f"  n={n} [{il}, {iu}]: ||AZ - BZW|| = {res:.2e} (gate {1e-12 * scale * n:.2e}), ||Z^T B Z - I|| = {orth:.2e} "
              f"(gate {1e-12 * n:.2e})")
        assert res < 1e-12 * scale * n and orth < 1e-12 * n
        assert bool((w[1:] >= w[:-1]).all())
        del a, b, z, Z
    assert (ws[410] - ws[n][:410]).abs().max().item() < 1e-12 * scale


# ------------------------------------------------------------------------------------------------ statuses
@pytest.mark.gpu
def test_statuses(gpu_lib):
    """NaN in the significant triangle of a or of b: -5 and w(1:m) = NaN; bad windows and modes: -2; B indefinite: -7"""
    import eigenexa_amd as ee
    from eigenexa_amd import api, layout

    n = 50
    A, B = _pencil(n)
    z = np.zeros((n, n), order="F")
    for which in ("a", "b"):
        a = np.asfortranarray(np.triu(A))
        b = np.asfortranarray(np.triu(B))
        (a if which == "a" else b)[3, 7] = np.nan
        w = np.full(9, 7.0)
        ee.KMATH_EIGEN_GEV_RANGE(n, 2, 9, a, n, b, n, w, z, n)
        assert api.last_status() == -5
        assert np.isnan(w[:8]).all() and w[8] == 7.0
    a = np.asfortranarray(np.triu(A))
    b = np.asfortranarray(np.triu(B))
    w = np.zeros(n)
    pa, pb, pw, pz = a.ctypes.data, b.ctypes.data, w.ctypes.data, z.ctypes.data
    fn = gpu_lib.eigx_gev_range
    assert fn(n, 0, 5, pa, n, pb, n, pw, pz, n, b"A") == -2
    assert fn(n, 3, n + 1, pa, n, pb, n, pw, pz, n, b"A") == -2
    assert fn(n, 6, 5, pa, n, pb, n, pw, pz, n, b"A") == -2
    assert fn(n, 1, 5, pa, n, pb, n, pw, pz, n, b"X") == -2
    assert fn(n, 1, 5, pa, n, pb, n, pw, None, n, b"A") == -2
    assert fn(n, 1, 5, pa, n, None, n, pw, pz, n, b"A") == -2
    assert fn(n, 1, 5, pa, n, pb, n - 1, pw, pz, n, b"A") == -2
    assert fn(0, 1, 1, pa, n, pb, n, pw, pz, n, b"A") == -2
    assert (a == np.triu(A)).all() and (b == np.triu(B)).all()     # nothing was touched
    Bi = np.asfortranarray(layout.random_symmetric(n, seed=4) - 1.0)
    ee.KMATH_EIGEN_GEV_RANGE(n, 1, 5, a, n, Bi, n, w, z, n)
    assert api.last_status() == -7
    for key, bad in [(20, 0), (20, 32), (20, 96), (20, 1088), (20, -64)]:
        assert gpu_lib.eigx_tune(key, bad) == -1
    old = gpu_lib.eigx_tune(20, 192)
    assert old % 64 == 0 and gpu_lib.eigx_tune(20, old) == 192


def _run_worker(*args, timeout=300):
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "gev_range_worker.py"), *args],
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
    """a fresh process: after one eigx_gev_range_dev at n = 1024, window [1, 64], the "gevr." buffers hold at most
    2 n^2 doubles, the n x NB inverses (NB <= 1024) with their assembly workspace, and 1 MiB"""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = 1024
    m = re.search(r"MEMORY gevr=(\d+) held=(\d+)", _run_worker("memory", str(n), "64"))
    assert m
    gevr = int(m.group(1))
    print(f"  n={n}: gevr.* {gevr} B, bound {(2 * n * n + 2 * 1024 * n) * 8 + 2 ** 20} B")
    assert 0 < gevr <= (2 * n * n + 2 * 1024 * n) * 8 + 2 ** 20


@pytest.mark.gpu
def test_refuses_several_ranks():
    """two ranks on the one card: both return EIGX_ERR_BAD_ARG and exit cleanly"""
    import socket

    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = os.path.join(os.path.dirname(__file__), "gev_range_worker.py")
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


# ------------------------------------------------------------------------------------------------ Fortran
@pytest.mark.gpu
def test_fortran_gev_range_caller(gpu_lib, tmp_path):
    """a Fortran program calls KMATH_EIGEN_GEV_RANGE on a pencil with Frank's spectrum, n = 200, window [3, 40]"""
    if not os.path.exists(FLANG):
        pytest.skip("no flang")
    import json

    GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "known_answers.json")))
    lib = os.path.join(ROOT, "eigenexa_amd", "lib")
    mod = os.path.join(ROOT, "eigenexa_amd", "fortran", "eigen_libs_mod.F90")
    src = os.path.join(ROOT, "tests", "fortran", "gev_range_caller.F90")
    subprocess.check_call([FLANG, "-cpp", "-O2", "-c", mod, "-o", "eigen_libs_mod.o"], cwd=tmp_path)
    subprocess.check_call([FLANG, "-cpp", "-O2", "-c", src, "-o", "gev_range_caller.o"], cwd=tmp_path)
    subprocess.check_call([FLANG, "-o", "gev_range_caller", "gev_range_caller.o", "eigen_libs_mod.o", f"-L{lib}",
                           "-leigenexa_amd", f"-Wl,-rpath,{lib}"], cwd=tmp_path)
    out = subprocess.run([str(tmp_path / "gev_range_caller")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)

    def val(label):
        m = re.search(label + r"\s*=\s*([0-9.eEdD+-]+)", out.stdout)
        assert m, out.stdout
        return float(m.group(1).replace("D", "E").replace("d", "e"))

    n = 200
    scale = max(1.0, val(r"max \|w\|"))
    assert val("max rel eigenvalue error") < GOLD["gates"]["frank_rel_err"]
    assert val("residual norm") < 1e-12 * scale * n
    assert val("B-orthogonality norm") < 1e-12 * n
    assert val("mode N difference") < 1e-12 * scale


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", GEVR_SYMBOLS)
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
    if name.startswith("eigx_gev_range"):
        assert [p.split()[-1].lstrip("*").replace("_dev", "") for p in params] == ["n", "il", "iu", "a", "lda", "b", "ldb", "w", "z",
                                                                                   "ldz", "mode"]


def test_library_exports_the_symbols_and_key_20():
    """the built library has the five entry points; eigx_tune key 20 takes multiples of 64 from 64 to 1024 (no GPU needed)"""
    from eigenexa_amd import _lib

    lib = _lib.load()
    for name in GEVR_SYMBOLS:
        assert hasattr(lib, name)
    default = lib.eigx_tune(20, 128)
    assert default in (128, 256, 512)
    for bad in (0, 63, 65, 96, 1088, -128):
        assert lib.eigx_tune(20, bad) == -1
    assert lib.eigx_tune(20, 1024) == 128
    assert lib.eigx_tune(20, default) == 1024
    assert lib.eigx_tune(20, default) == default


def test_python_wrapper_is_exported_and_rejects_bad_windows_before_the_library(monkeypatch, capsys):
    """il < 1, iu > n, il > iu, n <= 0, a mode outside A / N, a missing z with mode A: status -2 and a warning, without
    loading the library"""
    import eigenexa_amd as ee
    from eigenexa_amd import _lib, api

    assert "KMATH_EIGEN_GEV_RANGE" in dir(ee)

    def boom():
        raise AssertionError("the library must not be touched")

    monkeypatch.setattr(_lib, "load", boom)
    a = np.zeros((10, 10), order="F")
    b = np.zeros((10, 10), order="F")
    z = np.zeros((10, 10), order="F")
    w = np.zeros(10)
    for n, il, iu, zz, mode in [(10, 0, 3, z, "A"), (10, 2, 11, z, "A"), (10, 5, 4, z, "A"), (0, 1, 1, z, "A"),
                                (-1, 1, 1, z, "A"), (10, 1, 3, z, "X"), (10, 1, 3, z, "S"), (10, 1, 3, None, "A")]:
        api._state["last_status"] = 0
        ee.KMATH_EIGEN_GEV_RANGE(n, il, iu, a, 10, b, 10, w, zz, 10, mode=mode)
        assert api.last_status() == -2
    assert "invalid window" in capsys.readouterr().err


def test_fortran_module_declares_the_subroutine():
    src = open(os.path.join(ROOT, "eigenexa_amd", "fortran", "eigen_libs_mod.F90")).read()
    assert 'bind(C, name="eigx_gev_range")' in src
    assert re.search(r"^subroutine KMATH_EIGEN_GEV_RANGE\(n, il, iu, a, lda, b, ldb, w, z, ldz, mode\)", src, flags=re.M)
    assert re.search(r"character\(\*\), intent\(in\), optional :: mode", src.split("subroutine KMATH_EIGEN_GEV_RANGE")[1])
