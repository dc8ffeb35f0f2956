"""KMATH_EIGEN_HGEV -- an extension (the reference has no complex generalised solver): the complex Hermitian-definite
problem A x = lambda B x by the method of KMATH_EIGEN_GEV over complex numbers.  GPU tests against scipy and the known
Frank spectrum, consistency with KMATH_EIGEN_GEV and eigen_h, the multi-rank path, and CPU checks of the public surface."""
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
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "known_answers.json")))
FLANG = os.environ.get("FC", "/opt/rocm/lib/llvm/bin/flang")


def _nan_lower(M):
    """the upper triangle of M, NaN strictly below it and in Im of the diagonal (neither may matter)"""
    n = M.shape[0]
    out = np.where(np.triu(np.ones((n, n), dtype=bool)), M, np.nan + 1j * np.nan)
    d = np.empty(n, dtype=np.complex128)
    d.real, d.imag = M.real.diagonal(), np.nan
    out[np.diag_indices(n)] = d
    return np.asfortranarray(out)


def _hgev_host(A, B):
    import eigenexa_amd as ee
    from eigenexa_amd import api

    n = A.shape[0]
    a, b = _nan_lower(A), _nan_lower(B)
    z = np.zeros((n, n), dtype=np.complex128, order="F")
    w = np.zeros(n)
    ee.KMATH_EIGEN_HGEV(n, a, n, b, n, w, z, n)
    return api.last_status(), w, z, a, b


def _frank_pencil(n, unitary_q=True, seed=5):
    """A = G M G^H, B = G G^H with M = S^H K S (K Frank, S unit phases), G = Q D^1/2: spectrum = Frank's"""
    from eigenexa_amd import layout

    rng = np.random.default_rng(seed)
    s = np.exp(1j * rng.uniform(0, 2 * np.pi, n))
    M = s.conj()[:, None] * layout.frank(n) * s[None, :]
    if unitary_q:
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    else:
        Q = np.eye(n)
    G = Q * np.sqrt(rng.uniform(1.0, 10.0, n))[None, :]
    A = G @ M @ G.conj().T
    B = G @ G.conj().T
    return (A + A.conj().T) / 2, (B + B.conj().T) / 2


# ---------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 5, 130, 517])
def test_hgev_host_api_matches_scipy(gpu_lib, n):
    import scipy.linalg
    from eigenexa_amd import layout

    A = layout.random_hermitian(n, seed=3)
    B = layout.random_hpd(n, seed=n)
    rc, w, Z, a, b = _hgev_host(A, B)
    assert rc == 0
    wr = scipy.linalg.eigh(A, B, eigvals_only=True)
    scale = max(1.0, np.abs(wr).max())
    assert np.abs(w - wr).max() < 1e-12 * scale
    assert np.all(np.diff(w) >= 0)
    assert np.linalg.norm(A @ Z - B @ Z * w) < 1e-12 * scale * n
    assert np.linalg.norm(Z.conj().T @ B @ Z - np.eye(n)) < 1e-12 * n
    # on exit: b holds F (F^H B F = I), a holds the unitary Y, z = F Y
    F, Y = b, a
    assert np.linalg.norm(F.conj().T @ B @ F - np.eye(n)) < 1e-12 * n
    assert np.linalg.norm(Y.conj().T @ Y - np.eye(n)) < 1e-12 * n
    assert np.linalg.norm(F @ Y - Z) < 1e-12 * n * np.abs(F).max()


@pytest.mark.gpu
@pytest.mark.parametrize("n,unitary_q", [(64, True), (1000, True), (300, False)])
def test_hgev_frank_known_answer(gpu_lib, n, unitary_q):
    """the pencil reduces to M y = lambda y (y = G^H x); Q = I makes B diagonal, so eigen_h(B) deflates completely"""
    from eigenexa_amd import layout

    A, B = _frank_pencil(n, unitary_q)
    rc, w, Z, _, _ = _hgev_host(A, B)
    assert rc == 0
    lam = layout.frank_eigenvalues(n)
    assert np.abs((w - lam) / lam).max() < GOLD["gates"]["frank_rel_err"]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 300])
def test_hgev_real_input_agrees_with_kmath_eigen_gev(gpu_lib, n):
    import eigenexa_amd as ee
    from eigenexa_amd import api, layout

    A = layout.random_symmetric(n, seed=3)
    B = layout.random_hpd(n, seed=8, real=True)
    rc, w, _, _, _ = _hgev_host(A.astype(np.complex128), B.astype(np.complex128))
    assert rc == 0
    a, b = np.asfortranarray(np.triu(A)), np.asfortranarray(np.triu(B))
    wg, zg = np.zeros(n), np.zeros((n, n), order="F")
    ee.KMATH_EIGEN_GEV(n, a, n, b, n, wg, zg, n)
    assert api.last_status() == 0
    scale = max(1.0, np.abs(wg).max())
    assert np.abs(w - wg).max() < 1e-12 * scale


@pytest.mark.gpu
@pytest.mark.parametrize("n", [7, 260])
def test_hgev_identity_b_agrees_with_eigen_h(gpu_lib, n):
    import eigenexa_amd as ee
    from eigenexa_amd import api, layout

    A = layout.random_hermitian(n, seed=9)
    rc, w, _, _, _ = _hgev_host(A, np.eye(n, dtype=np.complex128))
    assert rc == 0
    ah = np.asfortranarray(A.copy())
    wh, zh = np.zeros(n), np.zeros((n, n), dtype=np.complex128, order="F")
    ee.eigen_h(n, n, ah, n, wh, zh, n)
    assert api.last_status() == 0
    scale = max(1.0, np.abs(wh).max())
    assert np.abs(w - wh).max() < 1e-12 * scale


def _dev_solve(n, ld, A, B):
    import torch
    import eigenexa_amd as ee
    from eigenexa_amd import api

    dev = torch.device("cuda:0")
    a = torch.zeros(n, ld, dtype=torch.complex128, device=dev)
    b = torch.zeros(n, ld, dtype=torch.complex128, device=dev)
    a[:, :n] = torch.from_numpy(_nan_lower(A).T.copy()).to(dev)
    b[:, :n] = torch.from_numpy(_nan_lower(B).T.copy()).to(dev)
    z = torch.zeros(n, ld, dtype=torch.complex128, device=dev)
    w = torch.zeros(n, dtype=torch.float64, device=dev)
    ee.KMATH_EIGEN_HGEV(n, a, ld, b, ld, w, z, ld)
    return api.last_status(), w, z


@pytest.mark.gpu
def test_hgev_device_api_odd_ld_timers_and_repro(gpu_lib):
    from eigenexa_amd import layout

    n, ld = 1200, 1201
    A = layout.random_hermitian(n, seed=5)
    B = layout.random_hpd(n, seed=6)
    rc, w, z = _dev_solve(n, ld, A, B)
    assert rc == 0
    t = (C.c_double * 16)()
    gpu_lib.eigx_get_timers(t)
    assert all(t[i] > 0 for i in range(5)), list(t)[:5]
    Z = z[:, :n].T.cpu().numpy()
    wg = w.cpu().numpy()
    scale = max(1.0, np.abs(wg).max())
    assert np.linalg.norm(A @ Z - B @ Z * wg) < 1e-12 * scale * n
    assert np.linalg.norm(Z.conj().T @ B @ Z - np.eye(n)) < 1e-12 * n
    # the reference's "Repro test" for eigen_h: the same input twice gives bit-identical results
    rc2, w2, z2 = _dev_solve(n, ld, A, B)
    assert rc2 == 0
    assert np.array_equal(w.cpu().numpy(), w2.cpu().numpy())
    assert np.array_equal(z[:, :n].cpu().numpy(), z2[:, :n].cpu().numpy())


@pytest.mark.gpu
def test_hgev_errors(gpu_lib, capfd):
    from eigenexa_amd import layout

    n = 50
    A = layout.random_hermitian(n, seed=3)
    # indefinite B: message and status, as KMATH_EIGEN_GEV
    B = layout.random_hpd(n, seed=7)
    Bi = B - (np.linalg.eigvalsh(B)[0] + 1.0) * np.eye(n)   # one eigenvalue -1, the rest either sign
    capfd.readouterr()
    rc, _, _, _, _ = _hgev_host(A, Bi)
    assert rc == -7
    assert "Matrix B is not positive definite!" in capfd.readouterr().err
    # NaN / Inf in a significant entry of a or b: EIGX_ERR_NONFINITE with w = NaN, as eigen_h
    for which, (i, j) in (("a", (3, 7)), ("b", (10, 10)), ("a", (0, 49))):
        A2, B2 = A.copy(), B.copy()
        (A2 if which == "a" else B2)[i, j] = np.nan if i != j else np.inf
        rc, w, _, _, _ = _hgev_host(A2, B2)
        assert rc == -5 and np.isnan(w).all(), (which, rc)
    # and a good call afterwards still works
    rc, _, _, _, _ = _hgev_host(A, B)
    assert rc == 0


@pytest.mark.gpu
def test_hgev_n4096_on_the_gpu(gpu_lib):
    """matrices made on the GPU; the gates of the host test with complex128 matmuls on the GPU"""
    import torch
    import eigenexa_amd as ee
    from eigenexa_amd import api

    n = 4096
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    S = torch.randn(n, n, dtype=torch.complex128, device=dev, generator=g)
    A = (S + S.conj().T) / 2
    X = torch.randn(n, n, dtype=torch.complex128, device=dev, generator=g)
    B = X @ X.conj().T / n + torch.eye(n, dtype=torch.complex128, device=dev)
    B = (B + B.conj().T) / 2
    # column-major images: a[j, i] = A(i, j); the lower triangles carry NaN
    upper = torch.triu(torch.ones(n, n, dtype=torch.bool, device=dev))
    nan = torch.full((n, n), complex(float("nan"), float("nan")), dtype=torch.complex128, device=dev)
    a = torch.where(upper, A, nan).T.contiguous()
    b = torch.where(upper, B, nan).T.contiguous()
    z = torch.zeros(n, n, dtype=torch.complex128, device=dev)
    w = torch.zeros(n, dtype=torch.float64, device=dev)
    ee.KMATH_EIGEN_HGEV(n, a, n, b, n, w, z, n)
    assert api.last_status() == 0
    Z = z.T
    wc = w.to(torch.complex128)
    scale = max(1.0, w.abs().max().item())
    assert torch.linalg.norm(A @ Z - (B @ Z) * wc[None, :]).item() < 1e-12 * scale * n
    assert torch.linalg.norm(Z.conj().T @ B @ Z - torch.eye(n, dtype=torch.complex128, device=dev)).item() < 1e-12 * n
    assert bool((w[1:] >= w[:-1]).all())


def _run_hgev_ranks(world, n, dims):
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = os.path.join(os.path.dirname(__file__), "mg_hgev_worker.py")
    env = dict(os.environ)
    env.setdefault("EIGX_SELFTEST_ROUNDS", "40")
    procs = [subprocess.Popen([sys.executable, script, str(r), str(world), str(port), str(n), dims or "-"],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env) for r in range(world)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=600)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"OK rank {r}/{world}" in o, o[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("world,n,dims", [(2, 150, ""), (4, 600, ""), (3, 97, "3x1"), (4, 203, "1x4"), (4, 3, ""),
                                          (3, 1, "")])
def test_multi_rank_kmath_eigen_hgev(world, n, dims):
    """the 2-D cyclic path: nothing gathered, w bit-identical on every rank, indefinite B refused on every rank"""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _run_hgev_ranks(world, n, dims)


@pytest.mark.gpu
def test_fortran_caller_known_answer(gpu_lib, tmp_path):
    """a Fortran program calls the external subroutine KMATH_EIGEN_HGEV on the Frank pencil with a diagonal B"""
    if not os.path.exists(FLANG):
        pytest.skip("no flang")
    lib = os.path.join(ROOT, "eigenexa_amd", "lib")
    mod = os.path.join(ROOT, "eigenexa_amd", "fortran", "eigen_libs_mod.F90")
    src = os.path.join(ROOT, "tests", "fortran", "hgev_caller.F90")
    subprocess.check_call([FLANG, "-cpp", "-O2", "-c", mod, "-o", "eigen_libs_mod.o"], cwd=tmp_path)
    subprocess.check_call([FLANG, "-cpp", "-O2", "-c", src, "-o", "hgev_caller.o"], cwd=tmp_path)
    subprocess.check_call([FLANG, "-o", "hgev_caller", "hgev_caller.o", "eigen_libs_mod.o", f"-L{lib}", "-leigenexa_amd",
                           f"-Wl,-rpath,{lib}"], cwd=tmp_path)
    out = subprocess.run([str(tmp_path / "hgev_caller")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"max rel eigenvalue error\s*=\s*([0-9.eEdD+-]+)", out.stdout)
    assert m, out.stdout
    assert float(m.group(1).replace("D", "E").replace("d", "e")) < GOLD["gates"]["frank_rel_err"]


# ---------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("name", ["eigx_hgev", "eigx_hgev_dev"])
def test_header_prototypes_match_the_ctypes_table(name):
    from eigenexa_amd import _lib

    params = _prototype(name)
    kinds = [C.c_void_p if "*" in p else C.c_int for p in params]
    assert all(p.startswith(("int ", "double*")) for p in params), params
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is C.c_int and list(argtypes) == kinds
    # the same argument list as eigx_gev[_dev]
    assert [re.sub(r"\s+\w+$", "", p) for p in params] == \
        [re.sub(r"\s+\w+$", "", p) for p in _prototype(name.replace("hgev", "gev"))]


def test_fortran_module_binds_kmath_eigen_hgev(tmp_path):
    src = open(os.path.join(ROOT, "eigenexa_amd", "fortran", "eigen_libs_mod.F90")).read()
    m = re.search(r"subroutine KMATH_EIGEN_HGEV\(n, a, lda, b, ldb, w, z, ldz\)(.*?)end subroutine KMATH_EIGEN_HGEV", src, re.S)
    assert m
    body = m.group(1)
    assert 'bind(C, name="eigx_hgev")' in body
    assert re.search(r"complex\(8\).*::\s*a\(lda, \*\), b\(ldb, \*\), z\(ldz, \*\)", body)
    if not os.path.exists(FLANG):
        pytest.skip("no flang")
    subprocess.check_call([FLANG, "-cpp", "-O2", "-c", os.path.join(ROOT, "eigenexa_amd", "fortran", "eigen_libs_mod.F90"),
                           "-o", str(tmp_path / "m.o")], cwd=tmp_path)


def test_not_initialised_returns_minus_one():
    """before eigen_init: status -1 from the C entry points and the Python wrapper (no GPU is touched)"""
    code = (
        "import ctypes, numpy as np\n"
        "import eigenexa_amd as ee\n"
        "from eigenexa_amd import _lib, api\n"
        "lib = _lib.load()\n"
        "assert lib.eigx_hgev(4, None, 4, None, 4, None, None, 4) == -1\n"
        "assert lib.eigx_hgev_dev(4, None, 4, None, 4, None, None, 4) == -1\n"
        "a = np.eye(4, dtype=np.complex128, order='F'); b = a.copy(); z = a.copy(); w = np.zeros(4)\n"
        "ee.KMATH_EIGEN_HGEV(4, a, 4, b, 4, w, z, 4)\n"
        "assert api.last_status() == -1\n"
        "print('OK')\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr


def test_python_api_exports_kmath_eigen_hgev():
    import eigenexa_amd as ee

    assert callable(ee.KMATH_EIGEN_HGEV)
    assert "not in the reference" in ee.KMATH_EIGEN_HGEV.__doc__
