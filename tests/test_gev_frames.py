"""The contract that the four generalised solvers (KMATH_EIGEN_GEV, KMATH_EIGEN_GEV_RANGE and their complex siblings HGEV,
HGEV_RANGE) share through GevFrame and HostStage (csrc/eigx_context.h), at n = 5 and 65:
  * device drivers: after an EIGX_OK call the stage seconds timers[1..4] are >= 0 and add up to timers[0] (1e-6 s);
  * host forms: what comes back, and when (eigx_gev returns w only on EIGX_OK, eigx_hgev always, the two range
    forms the entries they wrote on EIGX_OK or EIGX_ERR_NONFINITE; a is returned by the full solvers only, b = U and the m
    columns of z by the range forms on EIGX_OK);
  * all eight entries return EIGX_ERR_NOT_INITIALIZED before they look at any argument (a fresh process: this file run
    as a script).
Nothing here depends on how the drivers are written: the file passes unchanged against the library before GevFrame."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

SIZES = [5, 65]
SENT = 12345.678
OK, NOT_INIT, NONFINITE = 0, -1, -5
ENTRIES = ["eigx_gev", "eigx_gev_dev", "eigx_gev_range", "eigx_gev_range_dev", "eigx_hgev", "eigx_hgev_dev", "eigx_hgev_range",
           "eigx_hgev_range_dev"]


@functools.lru_cache(maxsize=None)
def _pencil(n, cplx):
    """seeded A (symmetric / Hermitian) and B (positive definite, spectrum within about [1, 5]); read-only"""
    g = np.random.default_rng(7000 + n)
    S = g.standard_normal((n, n)) + (1j * g.standard_normal((n, n)) if cplx else 0.0)
    X = g.standard_normal((n, n)) + (1j * g.standard_normal((n, n)) if cplx else 0.0)
    A = (S + S.conj().T) / 2
    B = X @ X.conj().T / n + np.eye(n)
    B = (B + B.conj().T) / 2
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


def _window(n):
    return (2, 4) if n == 5 else (n // 3, n // 3 + 9)


def _to_dev(M, ld):
    """column-major image of M with leading dimension ld: tensor (cols, ld), t[j, i] = M(i, j)"""
    import torch

    dev = torch.device("cuda:0")
    t = torch.zeros(M.shape[1], ld, dtype=torch.complex128 if np.iscomplexobj(M) else torch.float64, device=dev)
    t[:, :M.shape[0]] = torch.from_numpy(np.ascontiguousarray(M.T)).to(dev)
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("entry", [e for e in ENTRIES if e.endswith("_dev")])
def test_stage_timers_add_up(gpu_lib, entry, n):
    import torch

    cplx = "hgev" in entry
    A, B = _pencil(n, cplx)
    ld = n + 1   # even, as the real drivers require
    a, b = _to_dev(A, ld), _to_dev(B, ld)
    z = torch.zeros(n, ld, dtype=a.dtype, device=a.device)
    w = torch.zeros(n, dtype=torch.float64, device=a.device)
    fn = getattr(gpu_lib, entry)
    if "range" in entry:
        il, iu = _window(n)
        rc = fn(n, il, iu, a.data_ptr(), ld, b.data_ptr(), ld, w.data_ptr(), z.data_ptr(), ld, b"A")
    else:
        rc = fn(n, a.data_ptr(), ld, b.data_ptr(), ld, w.data_ptr(), z.data_ptr(), ld)
    torch.cuda.synchronize()
    assert rc == OK
    t = np.full(16, -1.0)
    assert gpu_lib.eigx_get_timers(t.ctypes.data_as(C.POINTER(C.c_double))) == OK
    print(f"  {entry} n={n}: timers[0..4] = {t[:5]}")
    assert (t[1:5] >= 0.0).all()
    assert abs(t[1:5].sum() - t[0]) < 1e-6


def _host_call(lib, entry, n, A, B, w, z):
    """one host call on Fortran-ordered copies of A and B; returns rc and the arrays as the call left them"""
    a, b = np.asfortranarray(A.copy()), np.asfortranarray(B.copy())
    if "range" in entry:
        il, iu = _window(n)
        rc = getattr(lib, entry)(n, il, iu, a.ctypes.data, n, b.ctypes.data, n, w.ctypes.data, z.ctypes.data, n, b"A")
    else:
        rc = getattr(lib, entry)(n, a.ctypes.data, n, b.ctypes.data, n, w.ctypes.data, z.ctypes.data, n)
    return rc, a, b


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("entry", [e for e in ENTRIES if not e.endswith("_dev")])
def test_host_forms_return_what_the_table_says(gpu_lib, entry, n):
    cplx = "hgev" in entry
    ranged = "range" in entry
    A, B = _pencil(n, cplx)
    il, iu = _window(n)
    m = iu - il + 1 if ranged else n
    zcols = m + 1 if ranged else n          # one column more than a range call may write
    dt = np.complex128 if cplx else np.float64

    # ---- NaN in A's upper triangle, w and z from the sentinel
    bad = A.copy()
    bad[1, 3] = np.nan
    w = np.full(n + 2, SENT)
    z = np.full((n, zcols), SENT, dtype=dt, order="F")
    rc, a, b = _host_call(gpu_lib, entry, n, bad, B, w, z)
    print(f"  {entry} n={n} NaN in A: rc {rc}, NaN entries of w {np.flatnonzero(np.isnan(w)).tolist()}")
    assert rc == NONFINITE
    written = 0 if entry == "eigx_gev" else m      # eigx_gev returns w on EIGX_OK only
    assert np.isnan(w[:written]).all() and (w[written:] == SENT).all()
    assert (z == SENT).all()
    assert np.array_equal(a, np.asfortranarray(bad), equal_nan=True) and np.array_equal(b, B)   # neither comes back

    # ---- a good call
    w = np.full(n + 2, SENT)
    z = np.full((n, zcols), SENT, dtype=dt, order="F")
    rc, a, b = _host_call(gpu_lib, entry, n, A, B, w, z)
    assert rc == OK
    assert np.isfinite(w[:m]).all() and (np.diff(w[:m]) >= 0).all() and (w[m:] == SENT).all()
    assert np.isfinite(z[:, :m]).all() and not (z[:, :m] == SENT).any() and (z[:, m:] == SENT).all()
    Z = z[:, :m]
    res = np.linalg.norm(A @ Z - B @ Z * w[:m])
    scale = max(1.0, np.abs(w[:m]).max())
    print(f"  {entry} n={n}: ||A Z - B Z W||_F = {res:.2e} (gate {1e-12 * scale * n:.2e})")
    assert res < 1e-12 * scale * n                 # the gate of tests/test_gev_range.py and tests/test_hgev.py
    if ranged:
        assert np.array_equal(a, A)                # a does not come back
        U = np.triu(b)                             # b = U, B = U^H U
        assert np.linalg.norm(U.conj().T @ U - B) < 1e-12 * n * np.linalg.norm(B)
    else:
        assert not np.array_equal(a, A) and not np.array_equal(b, B)   # a = Y and b = the factor come back
        assert np.linalg.norm(b @ a - Z) < 1e-12 * n * np.linalg.norm(b)   # Z = factor times Y


def _uninitialised():
    """(child process) every entry, with arguments that are all invalid, before eigen_init"""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from eigenexa_amd import _lib

    lib = _lib.load()
    for entry in ENTRIES:
        fn = getattr(lib, entry)
        rc = fn(0, 0, -1, None, 0, None, 0, None, None, 0, b"?") if "range" in entry else fn(0, None, 0, None, 0, None, None, 0)
        assert rc == NOT_INIT, (entry, rc)
    print("OK uninit", flush=True)


@pytest.mark.gpu
def test_not_initialised_comes_before_any_argument():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "uninit"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK uninit" in r.stdout, r.stdout + r.stderr


if __name__ == "__main__" and sys.argv[1:] == ["uninit"]:
    _uninitialised()
