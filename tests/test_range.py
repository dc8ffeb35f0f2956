"""Index-range eigensolves (eigen_sx_range / eigen_s_range, an EXTENSION: the reference has no index-range interface):
Sturm multi-section on an index window, inverse iteration with one eigenvector per GPU thread, CholQR2 + Rayleigh-Ritz,
acceptance test with fallback to the full divide and conquer.  GPU tests are marked; the CPU tests at the end check the
ctypes table and the Python wrappers' argument checks."""
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
EPS = np.finfo(np.float64).eps
FLANG = os.environ.get("FC", "/opt/rocm/lib/llvm/bin/flang")
RANGE_SYMBOLS = ["eigx_sx_range", "eigx_s_range", "eigx_sx_range_dev", "eigx_s_range_dev"]


def _dev():
    import torch

    return torch.device("cuda:0")


def _band_matrix(d, e, band):
    n = len(d)
    T = np.diag(d)
    for b in range(1, min(band, n - 1) + 1):
        T += np.diag(e[b - 1, b:n], b) + np.diag(e[b - 1, b:n], -b)
    return T


@pytest.fixture
def all_sizes(gpu_lib):
    """size rule off (eigx_tune key 17 = 100 %): every window takes the subset path unless its acceptance test refuses"""
    old = gpu_lib.eigx_tune(17, 100)
    yield gpu_lib
    gpu_lib.eigx_tune(17, old)


def _windows(n, m):
    mid = max(1, (n - m) // 2)
    return [(1, m), (n - m + 1, n), (mid, mid + m - 1), (n // 3 + 1, n // 3 + 1), (1, n)]


def _solve_range(A, route, il, iu, mode="A"):
    import eigenexa_amd as ee
    from eigenexa_amd import api

    n = A.shape[0]
    m = iu - il + 1
    a = np.asfortranarray(np.triu(A))
    z = np.full((n, m + 1), 7.0, order="F")   # one guard column: entries beyond m are not touched
    w = np.full(m + 1, 7.0)
    (ee.eigen_sx_range if route == "sx" else ee.eigen_s_range)(n, il, iu, a, n, w, z, n, mode=mode)
    assert api.last_status() == 0
    assert w[m] == 7.0 and (z[:, m] == 7.0).all()
    return w[:m], z[:, :m], a


def _solve_full(A, route):
    import eigenexa_amd as ee
    from eigenexa_amd import api

    n = A.shape[0]
    a = np.asfortranarray(np.triu(A))
    z = np.zeros((n, n), order="F")
    w = np.zeros(n)
    (ee.eigen_sx if route == "sx" else ee.eigen_s)(n, n, a, n, w, z, n)
    assert api.last_status() == 0
    return w, z


def _check_window(A, route, il, iu, wf, Zf):
    """eigenvalues against the slice of the full solve, the two gates on the m columns against the dense A, and the span
    against the full solve's.  Returns the indices (0-based, inside the window) of the columns left out of the span check:
    those whose eigenvalue is not separated from the window's outside neighbours by more than 1e-6 ||A||.
    Span bound: both solves pass the residual gate, ||A Z - Z W||_F <= GATE_RES n eps ||A||_F, so each computed vector lies
    within residual / gap of the exact invariant subspace (Davis-Kahan), and both pass the orthogonality gate,
    ||Z^T Z - I||_F <= GATE_ORTH n eps, which is what is left when the gap is infinite (the window [1, n]: the projector is
    the identity up to that); two solves: twice the sum."""
    from eigenexa_amd import layout

    n = A.shape[0]
    m = iu - il + 1
    w, Z, _ = _solve_range(A, route, il, iu)
    werr = np.abs(w - wf[il - 1:iu]).max()
    res, orth = layout.accuracy_metrics(A, w, Z)
    anorm = np.linalg.norm(A, 2)
    gap = np.full(m, np.inf)
    if il > 1:
        gap = np.minimum(gap, w - wf[il - 2])
    if iu < n:
        gap = np.minimum(gap, wf[iu] - w)
    keep = gap > 1e-6 * anorm
    Zw = Zf[:, il - 1:iu]
    dev = np.linalg.norm(Zw @ (Zw.T @ Z) - Z, axis=0)
    bound = 2.0 * (GATE_RES * n * EPS * np.linalg.norm(A) / np.maximum(gap, 1e-300) + GATE_ORTH * n * EPS)
    worst = (dev[keep] / bound[keep]).max() if keep.any() else 0.0
    left_out = [int(k) for k in np.nonzero(~keep)[0]]
    print(f"  window [{il}, {iu}] n={n} {route}: |w - w_full| = {werr:.2e}, residual {res:.3e}, orthogonality {orth:.3e}, "
          f"span deviation / bound (worst) = {worst:.2e}, left out of the span check: {left_out}")
    assert werr < 1e-12 * max(1.0, np.abs(wf).max())
    assert res < GATE_RES and orth < GATE_ORTH
    assert (dev[keep] <= bound[keep]).all()
    return left_out


def _only_boundary_runs(left_out, m):
    """the left-out columns form a run from the window's first column and / or a run up to its last one"""
    s = set(left_out)
    lo = 0
    while lo in s:
        lo += 1
    hi = m - 1
    while hi in s:
        hi -= 1
    return s <= set(range(0, lo)) | set(range(hi + 1, m))


# ------------------------------------------------------------------------------------------------ stage test
@pytest.mark.gpu
@pytest.mark.parametrize("band", [1, 2])
@pytest.mark.parametrize("n", [97, 400, 1500])
def test_band_stage_window(gpu_lib, band, n):
    """eigx_band_reduce_dev, then eigx_band_bisect_range_dev + eigx_band_eigvec_dev on a low, a high and an interior window
    of the band matrix: eigenvalues against LAPACK at the tolerance of test_band_bisect_matches_oracle, the two gates
    against the band matrix"""
    import torch
    import eigenexa_amd as ee
    from eigenexa_amd import layout

    A = layout.random_symmetric(n, seed=100 + n + band)
    lda = n + (n & 1)
    a = torch.zeros(n, lda, dtype=torch.float64, device=_dev())
    a[:, :n] = torch.from_numpy(np.ascontiguousarray(A.T)).to(_dev())
    d = torch.zeros(n, dtype=torch.float64, device=_dev())
    e = torch.zeros(2 * n, dtype=torch.float64, device=_dev())
    assert gpu_lib.eigx_band_reduce_dev(n, a.data_ptr(), lda, d.data_ptr(), e.data_ptr(), n, 48, band) == 0
    dh, eh = d.cpu().numpy(), e.cpu().numpy().reshape(2, n)
    T = _band_matrix(dh, eh, band)
    wr = np.linalg.eigvalsh(T)
    m = max(1, n // 8)
    for il, iu in [(1, m), (n - m + 1, n), (n // 2 - m, n // 2 + m)]:
        mm = iu - il + 1
        ws = torch.zeros(mm, dtype=torch.float64, device=_dev())
        assert gpu_lib.eigx_band_bisect_range_dev(n, il, iu, d.data_ptr(), e.data_ptr(), n, band, ws.data_ptr()) == 0
        wsel = ws.cpu().numpy()
        assert (np.diff(wsel) >= 0).all()
        assert np.abs(wsel - wr[il - 1:iu]).max() < 1e-13 * max(1.0, np.abs(wr).max())
        wo = torch.zeros(mm, dtype=torch.float64, device=_dev())
        ldz = n + (n & 1)
        z = torch.zeros(mm, ldz, dtype=torch.float64, device=_dev())
        before = ee.range_info()
        rc = gpu_lib.eigx_band_eigvec_dev(n, mm, d.data_ptr(), e.data_ptr(), n, band, ws.data_ptr(), wo.data_ptr(),
                                          z.data_ptr(), ldz)
        assert rc == 0
        assert ee.range_info() == before   # the record of the last range SOLVE is not the stage entries' to write
        w = wo.cpu().numpy()
        Z = z[:, :n].T.cpu().numpy()
        res, orth = layout.accuracy_metrics(T, w, Z)
        print(f"  band {band} n={n} [{il}, {iu}]: |w - lapack| = {np.abs(w - wr[il - 1:iu]).max():.2e}, residual {res:.3e}, "
              f"orthogonality {orth:.3e}")
        assert np.abs(w - wr[il - 1:iu]).max() < 1e-13 * max(1.0, np.abs(wr).max())
        assert res < GATE_RES and orth < GATE_ORTH


# ------------------------------------------------------------------------------------------------ whole solves
@pytest.mark.gpu
@pytest.mark.parametrize("route", ["sx", "s"])
@pytest.mark.parametrize("n,seed", [(333, 5), (700, 6)])
def test_range_random_symmetric(all_sizes, route, n, seed):
    """seeded random matrices: every window against the full solve; the spectrum of these seeds has no pair closer than
    1e-6 ||A|| (asserted below with LAPACK on the CPU), so no column is left out of the span check"""
    import eigenexa_amd as ee
    from eigenexa_amd import layout

    A = layout.random_symmetric(n, seed=seed)
    wl = np.linalg.eigvalsh(A)
    assert np.diff(wl).min() > 1e-6 * np.abs(wl).max()
    wf, Zf = _solve_full(A, route)
    m = n // 5
    for il, iu in _windows(n, m):
        left = _check_window(A, route, il, iu, wf, Zf)
        assert len(left) == 0
        info = ee.range_info()
        assert info.m == iu - il + 1
        if iu - il + 1 <= n // 4:
            assert info.path == 1
    # eigenvalues only: z untouched (may be None)
    w, _, _ = _solve_range(A, route, 3, 50, mode="N")
    assert np.abs(w - wf[2:50]).max() < 1e-12 * max(1.0, np.abs(wf).max())
    a = np.asfortranarray(np.triu(A))
    w2 = np.zeros(48)
    (ee.eigen_sx_range if route == "sx" else ee.eigen_s_range)(n, 3, 50, a, n, w2, None, n, mode="N")
    assert (w2 == w).all()


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["sx", "s"])
@pytest.mark.parametrize("n", [200, 1000])
def test_range_frank_known_answer(all_sizes, route, n):
    """the Frank matrix (benchmark/mat_set.f:638-647): window eigenvalues against the closed form, as test_frank_known_answer.
    Span check: ||A|| is about 4 n^2 / pi^2 while the lower three quarters of the spectrum lie in [0.25, 1.8], so at the
    1e-6 ||A|| separation rule a low or interior window at n = 1000 is one cluster with its outside neighbours and every
    column is left out (n = 200: the nine columns next to the outside neighbour); the left-out columns must form runs from
    the window's ends.  The upper end of the spectrum is well separated: in the top window only columns next to its lower
    outside neighbour are left out (26 of 250 at n = 1000)."""
    import eigenexa_amd as ee
    from eigenexa_amd import layout

    A = layout.frank(n)
    lam = layout.frank_eigenvalues(n)
    wf, Zf = _solve_full(A, route)
    m = n // 4
    for il, iu in _windows(n, m):
        w, Z, a = _solve_range(A, route, il, iu)
        assert np.abs((w - lam[il - 1:iu]) / lam[il - 1:iu]).max() < GOLD["gates"]["frank_rel_err"]
        if iu - il + 1 <= n // 4:
            assert ee.range_info().path == 1
        assert a[0, 0] > 0 and a[1, 0] > 0 and a[2, 0] == -1.0   # a(1:3,1) = flops, seconds, -1
        left = _check_window(A, route, il, iu, wf, Zf)
        assert _only_boundary_runs(left, iu - il + 1)
        if il > n // 2:
            assert all(k < (iu - il + 1) // 4 for k in left)   # only next to the lower outside neighbour


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["sx", "s"])
@pytest.mark.parametrize("mtype", [1, 3, 4, 5, 6, 7, 8, 9])
def test_range_reference_matrix_families(all_sizes, route, mtype):
    """matrix types of the reference's benchmark driver (benchmark/mat_set.f:566-595) at n = 333, type 6 (six distinct
    eigenvalues: a window lies inside or across clusters of multiplicity 55) included.  Columns of a cluster that the
    window cuts cannot be compared with the full solve's span: they are the runs at the window's two ends."""
    import eigenexa_amd as ee
    from eigenexa_amd import layout

    n = 333
    A, _ = layout.reference_matrix(n, mtype)
    wf, Zf = _solve_full(A, route)
    for il, iu in _windows(n, 80):
        left = _check_window(A, route, il, iu, wf, Zf)
        info = ee.range_info()
        print(f"  type {mtype}: path {info.path}, cond(L) {info.cond:.3g}")
        if mtype == 6 and iu - il + 1 <= n // 4:
            assert info.path == 1
        assert _only_boundary_runs(left, iu - il + 1)


# ------------------------------------------------------------------------------------------------ which code ran
@pytest.mark.gpu
def test_size_rule_and_forced_fallback(gpu_lib):
    """path 3 when key 17 is below the window, path 2 when the acceptance bound is forced low on the type-6 matrix (key 19 = 0:
    cond(L) <= 1 is asked for); the gates hold on every path"""
    import eigenexa_amd as ee
    from eigenexa_amd import layout

    n = 333
    A, _ = layout.reference_matrix(n, 6)
    wf, Zf = _solve_full(A, "sx")
    # the default size rule is automatic (-1) and does not take the subset path at this n
    _check_window(A, "sx", 1, 10, wf, Zf)
    assert ee.range_info().path == 3
    old17 = gpu_lib.eigx_tune(17, 100)
    assert old17 == -1
    try:
        for il, iu in [(1, 60), (100, 170)]:
            gpu_lib.eigx_tune(17, 100)
            _check_window(A, "sx", il, iu, wf, Zf)
            assert ee.range_info().path == 1 and ee.range_info().cond >= 1.0
            gpu_lib.eigx_tune(17, 5)     # 100 m > 5 n
            _check_window(A, "sx", il, iu, wf, Zf)
            assert ee.range_info().path == 3
            gpu_lib.eigx_tune(17, 100)
            old19 = gpu_lib.eigx_tune(19, 0)
            try:
                _check_window(A, "s", il, iu, wf, Zf)
                assert ee.range_info().path == 2 and ee.range_info().cond > 1.0
            finally:
                gpu_lib.eigx_tune(19, old19)
            assert old19 == 6
    finally:
        gpu_lib.eigx_tune(17, old17)


@pytest.mark.gpu
def test_opt_in_route_of_eigen_sx(gpu_lib):
    """eigx_tune(18, 1): eigen_sx(n, 40, ...) takes the range path; with key 18 back at 0 the call is bit-identical to one made
    before the key was touched and leaves range_info alone"""
    import eigenexa_amd as ee
    from eigenexa_amd import api, layout

    n = 400
    A = layout.random_symmetric(n, seed=9)
    wr = np.linalg.eigvalsh(A)

    def run():
        a = np.asfortranarray(A.copy())
        z = np.zeros((n, n), order="F")
        w = np.zeros(n)
        ee.eigen_sx(n, 40, a, n, w, z, n)
        assert api.last_status() == 0
        return w, z

    w0, z0 = run()
    old17 = gpu_lib.eigx_tune(17, 100)
    assert gpu_lib.eigx_tune(18, 1) == 0
    try:
        w1, z1 = run()
        info = ee.range_info()
    finally:
        assert gpu_lib.eigx_tune(18, 0) == 1
        gpu_lib.eigx_tune(17, old17)
    assert info.path == 1 and info.m == 40
    Z = z1[:, :40]
    assert np.linalg.norm(A @ Z - Z * w1[:40]) / (n * EPS * np.linalg.norm(A)) < GATE_RES
    assert np.linalg.norm(Z.T @ Z - np.eye(40)) / (n * EPS) < GATE_ORTH
    assert np.abs(w1 - wr).max() < 1e-12 * np.abs(wr).max()     # w holds all n eigenvalues, as the reference's does
    _solve_range(A, "s", 5, 9)
    before = ee.range_info()
    w2, z2 = run()
    assert (w2 == w0).all() and (z2 == z0).all()
    assert ee.range_info() == before and before.m == 5


# ------------------------------------------------------------------------------------------------ memory / ranks
@pytest.mark.gpu
def test_range_memory_scales_with_the_window():
    """a fresh process: after one eigx_sx_range_dev at n = 4096, m = 128 on the subset path the "dc." workspace is what the
    128 x 128 Rayleigh-Ritz solve needs, far below the 2 n^2 of the outer D&C, and the whole pool stays inside
    eigx_memory_internal(n)"""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "range_worker.py"), "memory", "4096", "128"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"MEMORY path=(\d+) dc=(\d+) held=(\d+) internal=(\d+)", r.stdout)
    assert m, r.stdout + r.stderr
    path, dc, held, internal = (int(v) for v in m.groups())
    print(f"  n=4096 m=128: dc.* {dc} B, held {held} B, eigx_memory_internal {internal} B")
    assert path == 1
    assert dc < 4096 * 4096 * 8
    assert held <= internal


@pytest.mark.gpu
def test_range_refuses_several_ranks():
    """two ranks on the one card: the range entries return EIGX_ERR_BAD_ARG on both and the processes exit cleanly"""
    import socket

    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = os.path.join(os.path.dirname(__file__), "range_worker.py")
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


# ------------------------------------------------------------------------------------------------ errors
@pytest.mark.gpu
def test_range_errors(gpu_lib):
    """bad windows, sizes and modes are EIGX_ERR_BAD_ARG (-2) at the C-ABI; a NaN in the upper triangle is
    EIGX_ERR_NONFINITE (-5) with w(1:m) = NaN, as for eigen_sx"""
    import eigenexa_amd as ee
    from eigenexa_amd import api, layout

    n = 50
    A = layout.random_symmetric(n)
    a = np.asfortranarray(A.copy())
    z = np.zeros((n, n), order="F")
    w = np.zeros(n)
    pa, pw, pz = a.ctypes.data, w.ctypes.data, z.ctypes.data
    for fn in (gpu_lib.eigx_sx_range, gpu_lib.eigx_s_range):
        assert fn(n, 0, 5, pa, n, pw, pz, n, 48, 128, b"A") == -2
        assert fn(n, 3, n + 1, pa, n, pw, pz, n, 48, 128, b"A") == -2
        assert fn(n, 6, 5, pa, n, pw, pz, n, 48, 128, b"A") == -2
        assert fn(0, 1, 1, pa, n, pw, pz, n, 48, 128, b"A") == -2
        assert fn(-3, 1, 1, pa, n, pw, pz, n, 48, 128, b"A") == -2
        assert fn(n, 1, 5, pa, n, pw, pz, n, 48, 128, b"X") == -2
        assert fn(n, 1, 5, pa, n, pw, pz, n, 48, 128, b"S") == -2
        assert fn(n, 1, 5, pa, n, pw, None, n, 48, 128, b"A") == -2
        assert fn(n, 1, 5, pa, n - 1, pw, pz, n, 48, 128, b"A") == -2
    assert (a == A).all()     # nothing was touched
    B = A.copy()
    B[3, 7] = np.nan
    B[20, 11] = np.inf        # lower triangle: never read
    for route in ("sx", "s"):
        a = np.asfortranarray(B.copy())
        w = np.full(9, 7.0)
        (ee.eigen_sx_range if route == "sx" else ee.eigen_s_range)(n, 2, 9, a, n, w, z, n)
        assert api.last_status() == -5
        assert np.isnan(w[:8]).all() and w[8] == 7.0
    a = np.asfortranarray(np.tril(np.full((n, n), np.nan), -1) + np.triu(A))
    w = np.zeros(5)
    ee.eigen_sx_range(n, 1, 5, a, n, w, z, n)
    assert api.last_status() == 0 and np.abs(w - np.linalg.eigvalsh(A)[:5]).max() < 1e-12 * np.abs(A).sum(axis=1).max()


@pytest.mark.gpu
def test_range_scaling_extremes(all_sizes):
    """the factors of test_scaling_extremes through the range entries: rescaled inside, w unscaled"""
    import eigenexa_amd as ee
    from eigenexa_amd import layout

    n = 120
    A0 = layout.random_symmetric(n, seed=4)
    wr = np.linalg.eigvalsh(A0)
    for f in (1e-200, 1e200, 1e80, 1e-120):
        for route, (il, iu) in (("sx", (1, 20)), ("s", (90, 120))):
            w, Z, _ = _solve_range(A0 * f, route, il, iu)
            assert ee.range_info().path == 1
            assert np.abs(w / f - wr[il - 1:iu]).max() < 1e-12 * np.abs(wr).max()
            res, orth = layout.accuracy_metrics(A0, w / f, Z)
            assert res < GATE_RES and orth < GATE_ORTH


# ------------------------------------------------------------------------------------------------ device API
@pytest.mark.gpu
@pytest.mark.parametrize("route", ["sx", "s"])
@pytest.mark.parametrize("odd", [False, True])
def test_range_device_api(all_sizes, route, odd):
    """torch tensors on the GPU; lda from eigen_get_matdims or n + 1 (odd: served from a padded copy); the matrix is filled by
    an asynchronous copy on the default stream and the call follows at once"""
    import torch
    import eigenexa_amd as ee
    from eigenexa_amd import api, layout

    n = 1500
    il, iu = n - 199, n
    m = iu - il + 1
    for rep in range(2):
        A = layout.random_symmetric_torch(n, _dev(), seed=31 + rep)
        nx, ny = ee.eigen_get_matdims(n)
        lda = n + 1 if odd else nx
        assert (lda & 1) == (1 if odd else 0)
        a = torch.zeros(n, lda, dtype=torch.float64, device=_dev())
        a[:, :n] = A.T
        z = torch.zeros(m, lda, dtype=torch.float64, device=_dev())
        w = torch.zeros(m, dtype=torch.float64, device=_dev())
        if rep == 0:
            (ee.eigen_sx_range if route == "sx" else ee.eigen_s_range)(n, il, iu, a, lda, w, z, lda)
            assert api.last_status() == 0
        else:
            fn = all_sizes.eigx_sx_range_dev if route == "sx" else all_sizes.eigx_s_range_dev
            # (no torch.cuda.synchronize() here on purpose)
            assert fn(n, il, iu, a.data_ptr(), lda, w.data_ptr(), z.data_ptr(), lda, 128, 128, b"A") == 0
        assert ee.range_info().path == 1
        Z = z[:, :n].T
        anorm = torch.linalg.norm(A).item()
        res = torch.linalg.norm(A @ Z - Z * w[None, :]).item() / (n * EPS * anorm)
        orth = torch.linalg.norm(Z.T @ Z - torch.eye(m, dtype=torch.float64, device=_dev())).item() / (n * EPS)
        wl = torch.linalg.eigvalsh(A)[il - 1:iu]
        print(f"  {route} lda={lda}: residual {res:.3e}, orthogonality {orth:.3e}")
        assert res < GATE_RES and orth < GATE_ORTH
        assert (w - wl).abs().max().item() < 1e-12 * wl.abs().max().item()
        st = a[0, :3].cpu().numpy()
        assert st[0] > 0 and st[1] > 0 and st[2] == -1.0
        del A, a, z, w, Z


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["sx", "s"])
def test_range_n8192_windows(all_sizes, route):
    """n = 8192 random, windows [1, 512] and [n - 511, n] on the device API; the gates are computed on the GPU"""
    import torch
    import eigenexa_amd as ee
    from eigenexa_amd import layout

    n, m = 8192, 512
    nx, ny = ee.eigen_get_matdims(n)
    for il, iu in [(1, m), (n - m + 1, n)]:
        A = layout.random_symmetric_torch(n, _dev())
        a = torch.zeros(n, nx, dtype=torch.float64, device=_dev())
        a[:, :n] = A.T
        z = torch.zeros(m, nx, dtype=torch.float64, device=_dev())
        w = torch.zeros(m, dtype=torch.float64, device=_dev())
        fn = all_sizes.eigx_sx_range_dev if route == "sx" else all_sizes.eigx_s_range_dev
        assert fn(n, il, iu, a.data_ptr(), nx, w.data_ptr(), z.data_ptr(), nx, 128, 128, b"A") == 0
        info = ee.range_info()
        Z = z[:, :n].T
        anorm = torch.linalg.norm(A).item()
        res = torch.linalg.norm(A @ Z - Z * w[None, :]).item() / (n * EPS * anorm)
        orth = torch.linalg.norm(Z.T @ Z - torch.eye(m, dtype=torch.float64, device=_dev())).item() / (n * EPS)
        print(f"  {route} n={n} [{il}, {iu}]: path {info.path}, cond(L) {info.cond:.3g}, residual {res:.3e}, orthogonality {orth:.3e}")
        assert info.path == 1 and info.m == m
        assert res < GATE_RES and orth < GATE_ORTH
        assert (w[1:] >= w[:-1]).all()
        del A, a, z, w, Z


# ------------------------------------------------------------------------------------------------ Fortran
@pytest.mark.gpu
def test_fortran_range_caller(gpu_lib, tmp_path):
    """a Fortran program calls eigen_sx_range / eigen_s_range of module eigen_libs_mod on the Frank matrix"""
    if not os.path.exists(FLANG):
        pytest.skip("no flang")
    lib = os.path.join(ROOT, "eigenexa_amd", "lib")
    mod = os.path.join(ROOT, "eigenexa_amd", "fortran", "eigen_libs_mod.F90")
    src = os.path.join(ROOT, "tests", "fortran", "range_caller.F90")
    subprocess.check_call([FLANG, "-cpp", "-O2", "-c", mod, "-o", "eigen_libs_mod.o"], cwd=tmp_path)
    subprocess.check_call([FLANG, "-cpp", "-O2", "-c", src, "-o", "range_caller.o"], cwd=tmp_path)
    subprocess.check_call([FLANG, "-o", "range_caller", "range_caller.o", "eigen_libs_mod.o", f"-L{lib}", "-leigenexa_amd",
                           f"-Wl,-rpath,{lib}"], cwd=tmp_path)
    out = subprocess.run([str(tmp_path / "range_caller")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    num = r"\s*=\s*([0-9.eEdD+-]+)"
    m = re.search(r"max rel eigenvalue error" + num, out.stdout)
    r = re.search(r"max residual norm" + num, out.stdout)
    assert m and r, out.stdout
    assert float(m.group(1).replace("D", "E").replace("d", "e")) < GOLD["gates"]["frank_rel_err"]
    # per column ||A z - w z|| <= the residual gate on the whole block: GATE_RES n eps ||A||_F, ||Frank(300)||_F < 300^2
    assert float(r.group(1).replace("D", "E").replace("d", "e")) < GATE_RES * 300 * EPS * 300.0 ** 2


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", RANGE_SYMBOLS + ["eigx_band_bisect_range_dev", "eigx_band_eigvec_dev", "eigx_range_info",
                                  "eigx_range_timers"])
def test_header_prototypes_match_the_ctypes_table(name):
    from eigenexa_amd import _lib

    params = _prototype(name)
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is C.c_int and len(argtypes) == len(params)
    for p, t in zip(params, argtypes):
        if p.startswith("char "):
            assert t is C.c_char
        elif name in ("eigx_range_info", "eigx_range_timers"):
            assert t == (C.POINTER(C.c_int) if p.startswith("int*") else C.POINTER(C.c_double))
        elif "*" in p:
            assert t is C.c_void_p
        else:
            assert p.startswith("int ") and t is C.c_int
    if name in RANGE_SYMBOLS:
        assert [p.split()[-1] for p in params] == ["n", "il", "iu", "a", "lda", "w", "z", "ldz", "m_forward", "m_backward", "mode"]


def test_python_wrappers_reject_bad_windows_before_the_library(monkeypatch, capsys):
    """il < 1, iu > n, il > iu, n <= 0, a mode outside A / N, a missing z with mode A: status -2 and a warning, without
    loading the library"""
    import eigenexa_amd as ee
    from eigenexa_amd import _lib, api

    def boom():
        raise AssertionError("the library must not be touched")

    monkeypatch.setattr(_lib, "load", boom)
    a = np.zeros((10, 10), order="F")
    z = np.zeros((10, 10), order="F")
    w = np.zeros(10)
    for fn in (ee.eigen_sx_range, ee.eigen_s_range):
        for n, il, iu, zz, mode in [(10, 0, 3, z, "A"), (10, 2, 11, z, "A"), (10, 5, 4, z, "A"), (0, 1, 1, z, "A"),
                                    (-1, 1, 1, z, "A"), (10, 1, 3, z, "X"), (10, 1, 3, z, "S"), (10, 1, 3, None, "A")]:
            api._state["last_status"] = 0
            fn(n, il, iu, a, 10, w, zz, 10, mode=mode)
            assert api.last_status() == -2
    assert "invalid window" in capsys.readouterr().err
    assert {"eigen_sx_range", "eigen_s_range", "range_info"} <= set(dir(ee))


def test_fortran_module_binds_the_range_entries():
    src = open(os.path.join(ROOT, "eigenexa_amd", "fortran", "eigen_libs_mod.F90")).read()
    for name in ("eigx_sx_range", "eigx_s_range"):
        assert f'bind(C, name="{name}")' in src
    assert "public :: eigen_sx_range, eigen_s_range" in src


def test_range_tune_keys_refuse_values_outside_their_range():
    """keys 17 - 19 (no GPU needed): defaults -1 (automatic size rule) / 0 / 6; key 17 takes 0 .. 100 or a negative value
    (automatic), key 18 only 0 / 1, key 19 0 .. 16; anything else is refused with -1 and changes nothing"""
    from eigenexa_amd import _lib

    lib = _lib.load()
    for key, default, good, bad in [(17, -1, 25, 101), (18, 0, 1, 2), (19, 6, 3, 17)]:
        assert lib.eigx_tune(key, good) == default
        assert lib.eigx_tune(key, bad) == -1
        assert lib.eigx_tune(key, default) == good      # the refused value changed nothing
        assert lib.eigx_tune(key, default) == default
    assert lib.eigx_tune(18, -1) == -1 and lib.eigx_tune(19, -1) == -1
    assert lib.eigx_tune(17, -7) == -1 and lib.eigx_tune(17, -1) == -1   # any negative value means automatic
    assert lib.eigx_tune(18, 0) == 0 and lib.eigx_tune(19, 6) == 6
