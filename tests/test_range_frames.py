"""The contract that the range solves of the five families share (csrc/range.hip: the window stage of the device drivers and
the one host form), through the ten host entries eigx_{sx,s,h,gev,hgev}_range[_v] at n = 5 and 65, windows (2, 4) and
(n/3, n/3 + 9), value bounds midway between numpy's eigenvalues.  Every call starts from sentinel-filled w and z and fresh
copies of A and B, and what it left is compared exactly with the sentinel and the inputs:

  call                      status  w                 z            a                       b      *m, *il
  good, mode 'A'            OK      w(1:m)            z(:, 1:m)    statistics (*)          U      m, il
  mode 'N'                  OK      w(1:m)            -            statistics              U      m, il
  NaN in A                  -5      w(1:wcap) = NaN   -            -                       -      0, untouched
  empty window (by value)   OK      -                 -            statistics              U      0, count(vl) + 1
  mmax too small (value)    -9      -                 -            -                       -      m, il
  mode 'C' (by value)       OK      -                 -            statistics              U      m, il
  (*) a(1:3,1) for sx / s (a(3,1) = -1 on one GPU), a(1:2,1) for h, nothing for gev / hgev; wcap = m by index, mmax by value

Then per family: the value call and the index call of the window it returned give bit-identical w and z; one device call at
n = 65 with il > 1 and eigx_tune key 17 = 0, which cuts the window out of the full divide and conquer (path 3); and all twenty
entries return EIGX_ERR_NOT_INITIALIZED before they look at any argument (a fresh process: this file run as a script).
Nothing here depends on how the drivers are written: the file passes unchanged against the library before range.hip.
Last the windowed batched entries eigx_{s,h,gev,hgev}_batch_range_dev (csrc/batch_frame.hip: one frame for the four families):
what each of the three routes leaves after a batch with one failed matrix."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

SIZES = [5, 65]
FAMILIES = ["sx", "s", "h", "gev", "hgev"]
SENT = 12345.678
MARK = -77                      # what *m and *il start from
OK, NOT_INIT, NONFINITE, WINDOW = 0, -1, -5, -9
STAT_ROWS = {"sx": 3, "s": 3, "h": 2, "gev": 0, "hgev": 0}
EPS = np.finfo(np.float64).eps


@functools.lru_cache(maxsize=None)
def _problem(fam, n):
    """seeded A (symmetric / Hermitian), B (positive definite, spectrum within about [1, 5]; None for the standard families)
    and the ascending eigenvalues by numpy; read-only"""
    cplx, pencil = fam in ("h", "hgev"), fam in ("gev", "hgev")
    g = np.random.default_rng(7100 + n)
    S = g.standard_normal((n, n)) + (1j * g.standard_normal((n, n)) if cplx else 0.0)
    X = g.standard_normal((n, n)) + (1j * g.standard_normal((n, n)) if cplx else 0.0)
    A = (S + S.conj().T) / 2
    A.setflags(write=False)
    if not pencil:
        return A, None, np.linalg.eigvalsh(A)
    B = X @ X.conj().T / n + np.eye(n)
    B = (B + B.conj().T) / 2
    B.setflags(write=False)
    L = np.linalg.cholesky(B)
    Cm = np.linalg.solve(L, np.linalg.solve(L, A).conj().T).conj().T
    return A, B, np.linalg.eigvalsh((Cm + Cm.conj().T) / 2)


def _window(n):
    return (2, 4) if n == 5 else (n // 3, n // 3 + 9)


def _mid(lam, k):
    """between the eigenvalues k and k + 1 (1-based, 1 <= k < n)"""
    return 0.5 * (lam[k - 1] + lam[k])


def _call(lib, fam, n, A, B, win, mode, w, z, dev=False, ld=None):
    """One call of eigx_<fam>_range[_v][_dev]: win = (il, iu) or (vl, vu, mmax).  Host form: Fortran-ordered copies of A and B,
    w and z numpy arrays; device form: tensors with the leading dimension ld.  Returns rc, a, b as left, *m, *il."""
    ld = ld or n
    if dev:
        a, b = _to_dev(A, ld), None if B is None else _to_dev(B, ld)
        ptr = lambda t: t.data_ptr()
    else:
        a, b = np.asfortranarray(A.copy()), None if B is None else np.asfortranarray(B.copy())
        ptr = lambda t: t.ctypes.data
    m, il = C.c_int(MARK), C.c_int(MARK)
    by_value = len(win) == 3
    fn = getattr(lib, f"eigx_{fam}_range" + ("_v" if by_value else "") + ("_dev" if dev else ""))
    head = (n, float(win[0]), float(win[1]), win[2], C.byref(m), C.byref(il)) if by_value else (n, win[0], win[1])
    mats = (ptr(a), ld) + (() if B is None else (ptr(b), ld))
    tail = (ptr(w), ptr(z), ld) + ((0, 0) if B is None else ())     # the standard families take m_forward, m_backward
    rc = fn(*head, *mats, *tail, mode)
    if dev:
        import torch

        torch.cuda.synchronize()
    return rc, a, b, m.value, il.value


def _to_dev(M, ld):
    """column-major image of M with leading dimension ld: tensor (cols, ld), t[j, i] = M(i, j)"""
    import torch

    dev = torch.device("cuda:0")
    t = torch.zeros(M.shape[1], ld, dtype=torch.complex128 if np.iscomplexobj(M) else torch.float64, device=dev)
    t[:, :M.shape[0]] = torch.from_numpy(np.ascontiguousarray(M.T)).to(dev)
    return t


def _fresh(n, zcols, dt):
    return np.full(n + 2, SENT), np.full((n, zcols), SENT, dtype=dt, order="F")


def _check_a_b(fam, n, a, b, A_in, B, returned):
    """returned: the call was EIGX_OK -- a differs from what went in exactly in its statistics, b holds U; else both are as passed"""
    rows = min(n, STAT_ROWS[fam]) if returned else 0
    rest = np.ones((n, n), dtype=bool)
    rest[:rows, 0] = False
    assert np.array_equal(a[rest], np.asfortranarray(A_in)[rest], equal_nan=True)
    if rows:
        st = a[:rows, 0]
        assert np.isfinite(st).all() and (st != A_in[:rows, 0]).all() and (np.imag(st) == 0).all()
        assert st[1].real > 0                       # seconds
        if rows == 3:
            assert st[2] == -1.0                    # no communication on one GPU
    if B is not None and returned:
        U = np.triu(b)
        assert np.linalg.norm(U.conj().T @ U - B) < 1e-12 * n * np.linalg.norm(B)
    elif B is not None:
        assert np.array_equal(b, B)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("by_value", [False, True], ids=["index", "value"])
@pytest.mark.parametrize("fam", FAMILIES)
def test_host_forms_return_what_the_table_says(gpu_lib, fam, by_value, n):
    A, B, lam = _problem(fam, n)
    il, iu = _window(n)
    m = iu - il + 1
    cap = m + 1 if by_value else m                 # by value: room for one eigenpair more than the window holds
    vl, vu = _mid(lam, il - 1), _mid(lam, iu)
    win = (vl, vu, cap) if by_value else (il, iu)
    dt = A.dtype
    window_out = (m, il) if by_value else (MARK, MARK)
    tag = f"eigx_{fam}_range{'_v' if by_value else ''} n={n}"

    # ---- a good call, mode 'A'
    w, z = _fresh(n, cap + 1, dt)
    rc, a, b, mo, ilo = _call(gpu_lib, fam, n, A, B, win, b"A", w, z)
    assert rc == OK and (mo, ilo) == window_out
    assert np.isfinite(w[:m]).all() and (np.diff(w[:m]) >= 0).all() and (w[m:] == SENT).all()
    assert np.isfinite(z[:, :m]).all() and not (z[:, :m] == SENT).any() and (z[:, m:] == SENT).all()
    Z = z[:, :m]
    res = np.linalg.norm(A @ Z - (Z if B is None else B @ Z) * w[:m])
    scale = max(1.0, np.abs(w[:m]).max())
    print(f"  {tag}: ||A Z - B Z W||_F = {res:.2e} (gate {1e-12 * scale * n:.2e}), max |w - numpy| = "
          f"{np.abs(w[:m] - lam[il - 1:iu]).max():.2e}")
    assert res < 1e-12 * scale * n                 # the gate of tests/test_gev_frames.py
    _check_a_b(fam, n, a, b, A, B, True)
    w_good = w.copy()

    # ---- mode 'N': the same eigenvalues' worth of w, z not touched
    w, z = _fresh(n, cap + 1, dt)
    rc, a, b, mo, ilo = _call(gpu_lib, fam, n, A, B, win, b"N", w, z)
    assert rc == OK and (mo, ilo) == window_out
    assert np.isfinite(w[:m]).all() and (np.diff(w[:m]) >= 0).all() and (w[m:] == SENT).all() and (z == SENT).all()
    assert np.abs(w[:m] - w_good[:m]).max() < 1e-12 * scale * n
    _check_a_b(fam, n, a, b, A, B, True)

    # ---- NaN in A's upper triangle: w(1:wcap) = NaN and *m = 0, nothing else
    bad = A.copy()
    bad[1, 3] = np.nan
    w, z = _fresh(n, cap + 1, dt)
    rc, a, b, mo, ilo = _call(gpu_lib, fam, n, bad, B, win, b"A", w, z)
    print(f"  {tag} NaN in A: rc {rc}, NaN entries of w {np.flatnonzero(np.isnan(w)).tolist()}")
    assert rc == NONFINITE and (mo, ilo) == ((0, MARK) if by_value else (MARK, MARK))
    assert np.isnan(w[:cap]).all() and (w[cap:] == SENT).all() and (z == SENT).all()
    _check_a_b(fam, n, a, b, bad, B, False)
    if not by_value:
        return

    # ---- an empty window inside the gap above eigenvalue il - 1
    gap = lam[il - 1] - lam[il - 2]
    w, z = _fresh(n, cap + 1, dt)
    rc, a, b, mo, ilo = _call(gpu_lib, fam, n, A, B, (lam[il - 2] + 0.25 * gap, lam[il - 2] + 0.75 * gap, cap), b"A", w, z)
    assert rc == OK and (mo, ilo) == (0, il)
    assert (w == SENT).all() and (z == SENT).all()
    _check_a_b(fam, n, a, b, A, B, True)

    # ---- mmax one too small: the window is reported, nothing is computed or returned
    w, z = _fresh(n, m, dt)
    rc, a, b, mo, ilo = _call(gpu_lib, fam, n, A, B, (vl, vu, m - 1), b"A", w, z)
    assert rc == WINDOW and (mo, ilo) == (m, il)
    assert (w == SENT).all() and (z == SENT).all()
    _check_a_b(fam, n, a, b, A, B, False)

    # ---- mode 'C': the count alone
    w, z = _fresh(n, 1, dt)
    rc, a, b, mo, ilo = _call(gpu_lib, fam, n, A, B, (vl, vu, 0), b"C", w, z)
    assert rc == OK and (mo, ilo) == (m, il)
    assert (w == SENT).all() and (z == SENT).all()
    _check_a_b(fam, n, a, b, A, B, True)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMILIES)
def test_value_call_is_the_index_call_of_its_window(gpu_lib, fam):
    n = 65
    A, B, lam = _problem(fam, n)
    il, iu = _window(n)
    m = iu - il + 1
    wv, zv = _fresh(n, m + 2, A.dtype)
    rc, _, _, mo, ilo = _call(gpu_lib, fam, n, A, B, (_mid(lam, il - 1), _mid(lam, iu), m + 1), b"A", wv, zv)
    assert rc == OK and (mo, ilo) == (m, il)
    wi, zi = _fresh(n, m + 2, A.dtype)
    rc, _, _, _, _ = _call(gpu_lib, fam, n, A, B, (ilo, ilo + mo - 1), b"A", wi, zi)
    assert rc == OK
    assert wv.tobytes() == wi.tobytes() and zv.tobytes() == zi.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMILIES)
def test_window_cut_out_of_the_full_divide_and_conquer(gpu_lib, fam):
    """device form, il > 1, key 17 = 0: the full D&C for the lowest iu pairs, the window copied (real) or offset (planes) out of
    it.  eigx_hgev_range_dev by index runs eigen_h itself, so the complex pencil goes by value (through herm_range_dev).
    Residual and orthogonality with the bounds of tests/range_worker.py: 768 and 8 in units of n eps."""
    import torch

    n = 65
    A, B, lam = _problem(fam, n)
    il, iu = _window(n)
    m = iu - il + 1
    win = (_mid(lam, il - 1), _mid(lam, iu), m) if fam == "hgev" else (il, iu)
    ld = n + 1                                    # even, as the real drivers require
    dev = torch.device("cuda:0")
    w = torch.full((m + 2,), SENT, dtype=torch.float64, device=dev)
    z = torch.full((m + 1, ld), SENT, dtype=torch.complex128 if np.iscomplexobj(A) else torch.float64, device=dev)
    old = gpu_lib.eigx_tune(17, 0)
    try:
        rc, _, _, _, _ = _call(gpu_lib, fam, n, A, B, win, b"A", w, z, dev=True, ld=ld)
        path, mm, cond = C.c_int(0), C.c_int(0), C.c_double(0.0)
        gpu_lib.eigx_range_info(C.byref(path), C.byref(mm), C.byref(cond))
    finally:
        gpu_lib.eigx_tune(17, old)
    assert rc == OK and (path.value, mm.value) == (3, m)
    wh, zh = w.cpu().numpy(), z.cpu().numpy()
    assert (wh[m:] == SENT).all() and (zh[m] == SENT).all() and (zh[:m, n:] == SENT).all()
    Z, wm = zh[:m, :n].T, wh[:m]
    BZ = Z if B is None else B @ Z
    res = np.linalg.norm(A @ Z - BZ * wm) / (n * EPS * np.linalg.norm(A))
    orth = np.linalg.norm(Z.conj().T @ BZ - np.eye(m)) / (n * EPS)
    print(f"  eigx_{fam}_range_dev n={n} {il}..{iu} path 3: residual {res:.2f} (768), orthogonality {orth:.2f} (8) n eps")
    assert res < 768 and orth < 8
    assert np.abs(wm - lam[il - 1:iu]).max() < 1e-12 * n * max(1.0, np.abs(lam).max())


BATCH_CUTOFF_KEY = {"s": 21, "h": 22, "gev": 23, "hgev": 24}
NOT_TOUCHED = -7.25


@pytest.mark.gpu
@pytest.mark.parametrize("route", [1, 2, 3])
@pytest.mark.parametrize("fam", ["s", "h", "gev", "hgev"])
def test_windowed_batch_frame_after_a_failed_matrix(gpu_lib, fam, route):
    """What the one windowed frame of the four batched families (csrc/batch_frame.hip: brange_frame_dev) leaves after a batch in
    which one matrix fails, on each of its three routes: eigx_<fam>_batch_range_dev on three matrices / pencils of order 5, the
    second with a NaN in A, window (2, 4), mode 'A'.  Route 1 (eigx_tune key 26 = 1: the window kernel), route 2 (key 26 = 2: the
    full batched solve and a gather), route 3 (the family's cutoff key lowered to 4: the range solver matrix by matrix).  The
    expected values are those of the four separate frames this one replaced, read off that library: the four families and the
    three routes agree in every one of them (errinfo = -1 on route 3 too, unlike the uniform batched frame: DESIGN section 8h)."""
    import torch

    n, nb, il, iu, ld = 5, 3, 2, 4, 6
    m = iu - il + 1
    dev = torch.device("cuda:0")
    A, B, _ = _problem(fam, n)
    cplx, pencil = np.iscomplexobj(A), B is not None
    dt = torch.complex128 if cplx else torch.float64

    def stack(M, nan_in_second):
        t = torch.zeros(nb, n, ld, dtype=dt, device=dev)          # t[k, j, i] = M_k(i, j)
        for k in range(nb):
            Mk = np.array(M) * (1.0 + 0.25 * k)
            if nan_in_second and k == 1:
                Mk[1, 3] = Mk[3, 1] = np.nan
            t[k, :, :n] = torch.from_numpy(np.ascontiguousarray(Mk.T)).to(dev)
        return t

    a = stack(A, True)
    b = stack(B, False) if pencil else None
    b_in = b.clone() if pencil else None
    w = torch.full((nb, m + 1), NOT_TOUCHED, dtype=torch.float64, device=dev)
    z = torch.full((nb, m, ld), NOT_TOUCHED, dtype=dt, device=dev)
    info = torch.full((nb,), 77, dtype=torch.int32, device=dev)
    key = BATCH_CUTOFF_KEY[fam] if route == 3 else 26
    old = gpu_lib.eigx_tune(key, 4 if route == 3 else route)
    assert old >= 0                               # the key took the value
    try:
        pens = (b.data_ptr(), ld, n * ld) if pencil else ()
        rc = getattr(gpu_lib, f"eigx_{fam}_batch_range_dev")(n, nb, il, iu, a.data_ptr(), ld, n * ld, *pens, w.data_ptr(), m + 1,
                                                            z.data_ptr(), ld, m * ld, b"A", info.data_ptr())
        torch.cuda.synchronize()
        err, r, mm, redone = C.c_int64(77), C.c_int(-1), C.c_int(-1), C.c_int(-1)
        gpu_lib.eigx_get_errinfo(C.byref(err))
        gpu_lib.eigx_batch_range_info(C.byref(r), C.byref(mm), C.byref(redone))
    finally:
        gpu_lib.eigx_tune(key, old)
    wh, zh, ih = w.cpu().numpy(), z.cpu().numpy(), info.cpu().numpy()
    print(f"  eigx_{fam}_batch_range_dev route {route}: rc {rc}, info {ih.tolist()}, errinfo {err.value}, "
          f"range_info {(r.value, mm.value, redone.value)}, w[1] {wh[1].tolist()}, z[1] untouched {bool((zh[1] == NOT_TOUCHED).all())}")
    assert rc == NONFINITE
    assert ih.tolist() == [OK, NONFINITE, OK]
    assert err.value == -1
    assert (r.value, mm.value, redone.value) == (route, m, 0)
    assert np.isnan(wh[1, :m]).all() and wh[1, m] == NOT_TOUCHED
    assert (zh[1] == NOT_TOUCHED).all()
    for k in (0, 2):                              # the others are solved all the same
        assert np.isfinite(wh[k, :m]).all() and (np.diff(wh[k, :m]) >= 0).all() and wh[k, m] == NOT_TOUCHED
        assert np.isfinite(zh[k, :, :n]).all() and (zh[k, :, n:] == NOT_TOUCHED).all()
    if pencil:
        assert torch.equal(b[1], b_in[1])
        assert not torch.equal(b[0], b_in[0])     # (U has taken B's place where the pencil was solved)


def _uninitialised():
    """(child process) every entry, with arguments that are all invalid, before eigen_init"""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from eigenexa_amd import _lib

    lib = _lib.load()
    for fam in FAMILIES:
        for suffix in ("", "_dev"):
            tail = (None, 0, None, 0, None, None, 0, b"?") if fam in ("gev", "hgev") else (None, 0, None, None, 0, 0, 0, b"?")
            rc = getattr(lib, f"eigx_{fam}_range{suffix}")(0, 0, -1, *tail)
            assert rc == NOT_INIT, (fam, suffix, rc)
            rc = getattr(lib, f"eigx_{fam}_range_v{suffix}")(0, 1.0, 0.0, -1, None, None, *tail)
            assert rc == NOT_INIT, (fam, suffix, "v", rc)
    print("OK uninit", flush=True)


@pytest.mark.gpu
def test_not_initialised_comes_before_any_argument():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "uninit"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK uninit" in r.stdout, r.stdout + r.stderr


if __name__ == "__main__" and sys.argv[1:] == ["uninit"]:
    _uninitialised()
