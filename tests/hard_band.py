"""Band matrices on which a divide-and-conquer eigensolver deflates, an extended-precision eigenvalue reference for them,
and column-wise / entry-wise error metrics (tests/test_dc_hard.py, tests/golden/make_dc_hard_bounds.py, tests/mg_worker.py).

Layout as in the other stage tests: d[n] is the diagonal, e[band, n] holds e[b-1, i] = T(i-b, i) (entries i < b unused, 0).
A plain module: no fixtures, no pytest settings."""
import json
import os

import numpy as np

LD = np.longdouble
# the reference has to be markedly more precise than the fp64 results it judges: x87 80-bit (eps 1.08e-19) or wider
assert np.finfo(LD).eps < 2e-19, "numpy.longdouble is no extended-precision type on this platform"
EPS = 2.0 ** -52

FAMILIES = ("wilkinson", "glued", "toeplitz", "equal_d_tiny_e", "split", "graded", "identity_plus", "clement",
            "half_identity")
SMALL_ONLY = ("zero", "diagonal")              # run at n = 33 only
SIZES = {1: (33, 65, 200, 1100), 2: (33, 65, 200, 600)}
BOUND_FACTOR = 16.0                            # test bound = BOUND_FACTOR x LAPACK's worst value over the case table
BOUNDS_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dc_hard_bounds.json")


def cases(max_n=None):
    """the case table: (band, n, family) for every family at every size, `zero` and `diagonal` at n = 33 only"""
    out = []
    for band in (1, 2):
        for n in SIZES[band]:
            if max_n is not None and n > max_n:
                continue
            for name in FAMILIES + (SMALL_ONLY if n == 33 else ()):
                out.append((band, n, name))
    return out


def families(n, band, seed=0):
    """{name: (d, e[band, n])}; the second band is used when band == 2, else dropped"""
    i = np.arange(n)
    fam = {}

    def rng_of(k):
        return np.random.default_rng([seed, n, band, k])

    def pack(d, e1, e2=None):
        e = np.zeros((band, n))
        if n > 1:
            e[0, 1:] = np.asarray(e1, dtype=np.float64)[1:]
        if band == 2 and e2 is not None and n > 2:
            e[1, 2:] = np.asarray(e2, dtype=np.float64)[2:]
        return np.asarray(d, dtype=np.float64).copy(), e

    r = rng_of(0)
    fam["wilkinson"] = pack(np.abs(i - (n - 1) / 2), np.ones(n), 1e-9 * r.standard_normal(n))
    e1 = np.ones(n)
    e1[21::21] = 1e-10
    fam["glued"] = pack(np.abs((i % 21) - 10.0), e1, np.zeros(n))
    fam["toeplitz"] = pack(np.full(n, 2.0), np.full(n, -1.0), np.full(n, 0.25))
    r = rng_of(3)
    fam["equal_d_tiny_e"] = pack(np.round(2 * r.standard_normal(n)) / 2, 1e-7 * r.standard_normal(n),
                                 1e-7 * r.standard_normal(n))
    r = rng_of(4)
    fam["split"] = pack(r.standard_normal(n), r.standard_normal(n) * (r.random(n) < 0.5),
                        r.standard_normal(n) * (r.random(n) < 0.3))
    g = 10.0 ** (-14.0 * i / max(n - 1, 1))
    fam["graded"] = pack(g, 0.3 * np.sqrt(np.r_[0.0, g[:-1]] * g), 0.1 * np.sqrt(np.r_[0.0, 0.0, g[:-2]] * g))
    fam["identity_plus"] = pack(np.ones(n), np.full(n, 1e-17), np.zeros(n))
    fam["clement"] = pack(np.zeros(n), np.sqrt(i * (n - i.astype(np.float64))), np.zeros(n))
    r = rng_of(8)
    h = n // 2
    d = r.standard_normal(n)
    e1 = r.standard_normal(n)
    d[h:] = 1.0
    e1[h:] = 0.0
    fam["half_identity"] = pack(d, e1, np.zeros(n))
    fam["zero"] = pack(np.zeros(n), np.zeros(n), np.zeros(n))
    fam["diagonal"] = pack(rng_of(10).standard_normal(n), np.zeros(n), np.zeros(n))
    return fam


def band_matrix(d, e, band, dtype=np.float64):
    n = len(d)
    T = np.diag(np.asarray(d, dtype=dtype))
    for b in range(1, min(band, n - 1) + 1):
        eb = np.asarray(e[b - 1, b:n], dtype=dtype)
        T += np.diag(eb, b) + np.diag(eb, -b)
    return T


def _bisect_tridiagonal(d, e):
    """all eigenvalues of the symmetric tridiagonal (d, e[i] = T(i-1, i)) in longdouble: Sturm counts for all n indices at
    once, 80 halvings of the Gershgorin interval"""
    n = len(d)
    d = np.asarray(d, dtype=LD)
    e2 = np.asarray(e, dtype=LD) ** 2
    ae = np.abs(np.asarray(e, dtype=LD))
    rad = np.zeros(n, dtype=LD)
    rad[1:] += ae[1:]
    rad[:-1] += ae[1:]
    glo, ghi = (d - rad).min(), (d + rad).max()
    pad = (ghi - glo) * LD(2.0) ** -40 + np.finfo(LD).tiny
    lo = np.full(n, glo - pad, dtype=LD)
    hi = np.full(n, ghi + pad, dtype=LD)
    k = np.arange(n)
    tiny = LD(np.finfo(LD).tiny) * LD(2.0) ** 64
    for _ in range(80):
        x = (lo + hi) / 2
        q = d[0] - x
        q = np.where(q == 0, -tiny, q)
        cnt = (q < 0).astype(np.int64)
        for i in range(1, n):
            q = (d[i] - x) - e2[i] / q
            q = np.where(q == 0, -tiny, q)
            cnt += q < 0
        up = cnt > k                      # more than k eigenvalues below x: lambda_k < x
        hi = np.where(up, x, hi)
        lo = np.where(up, lo, x)
    return (lo + hi) / 2


def _householder_tridiagonalise(T):
    """dense Householder tridiagonalisation in longdouble: returns (d, e) with e[i] = T'(i-1, i)"""
    A = np.array(T, dtype=LD)
    n = A.shape[0]
    for k in range(n - 2):
        x = A[k + 1:, k].copy()
        scale = np.abs(x).max()
        if scale == 0 or not np.any(x[1:] != 0):
            continue
        x /= scale
        alpha = -np.copysign(np.sqrt(x @ x), x[0])
        v = x
        v[0] -= alpha
        beta = 2 / (v @ v)
        B = A[k + 1:, k + 1:]
        p = beta * (B @ v)
        wv = p - (beta / 2) * (p @ v) * v
        B -= np.outer(v, wv) + np.outer(wv, v)
        A[k + 1, k] = A[k, k + 1] = alpha * scale
        A[k + 2:, k] = 0
        A[k, k + 2:] = 0
    e = np.zeros(n, dtype=LD)
    e[1:] = np.diagonal(A, 1)
    return np.diagonal(A).copy(), e


_cache = {}


def reference_eigenvalues(d, e, band, key=None):
    """ascending eigenvalues in numpy.longdouble.  Band 1: bisection on (d, e).  Band 2: Householder tridiagonalisation in
    longdouble first (a no-pivot LDL^T Sturm count on the pentadiagonal itself loses 1e8 eps on clustered input).
    key = (name, n, band) caches the result for the process."""
    if key is not None and key in _cache:
        return _cache[key]
    e = np.asarray(e)
    if band == 1 or len(d) < 3 or not np.any(e[1]):
        w = _bisect_tridiagonal(d, e[0])
    else:
        w = _bisect_tridiagonal(*_householder_tridiagonalise(band_matrix(d, e, band, LD)))
    w = np.sort(w)
    w.setflags(write=False)
    if key is not None:
        _cache[key] = w
    return w


def case(name, n, band, seed=0):
    """(d, e, w_ref) of one case of the table, the reference cached per (name, n, band)"""
    d, e = families(n, band, seed)[name]
    return d, e, reference_eigenvalues(d, e, band, key=(name, n, band, seed))


def metrics(d, e, band, w, Z, w_ref):
    """(E_w, E_r, E_o) in units of eps = 2^-52, column-wise and entry-wise maxima (no Frobenius norms):
    E_w = max_k |w_k - lambda_k| / (eps |T|_2), E_r = max_j |T z_j - w_j z_j|_2 / (eps |T|_2) with the banded product in
    longdouble, E_o = max |Z^T Z - I| / eps.  Z may hold the first m <= n columns only."""
    n = len(d)
    w = np.asarray(w, dtype=np.float64)
    Z = np.asarray(Z, dtype=np.float64)
    m = Z.shape[1]
    tnorm = float(np.abs(w_ref).max())
    tnorm = tnorm if tnorm > 0 else 1.0
    E_w = float(np.abs(w.astype(LD) - w_ref).max()) / (EPS * tnorm)
    Zl = Z.astype(LD)
    R = np.asarray(d, dtype=LD)[:, None] * Zl - Zl * w[:m].astype(LD)[None, :]
    for b in range(1, min(band, n - 1) + 1):
        eb = np.asarray(e[b - 1, b:n], dtype=LD)[:, None]
        R[b:] += eb * Zl[:-b]             # row i gets T(i, i-b) z[i-b]
        R[:-b] += eb * Zl[b:]             # row i-b gets T(i-b, i) z[i]
    E_r = float(np.sqrt((R * R).sum(axis=0)).max()) / (EPS * tnorm)
    E_o = float(np.abs(Z.T @ Z - np.eye(m)).max()) / EPS
    return E_w, E_r, E_o


def dense_metrics(A, w, Z):
    """E_r and E_o of a whole solve of the dense symmetric A (the product in longdouble, |A|_2 from LAPACK)"""
    w = np.asarray(w, dtype=np.float64)
    m = Z.shape[1]
    tnorm = float(np.abs(np.linalg.eigvalsh(A)).max()) or 1.0
    Zl = np.asarray(Z, dtype=LD)
    R = np.asarray(A, dtype=LD) @ Zl - Zl * w[:m].astype(LD)[None, :]
    E_r = float(np.sqrt((R * R).sum(axis=0)).max()) / (EPS * tnorm)
    E_o = float(np.abs(Z.T @ Z - np.eye(m)).max()) / EPS
    return E_r, E_o


def bounds():
    """the bounds in force: BOUND_FACTOR x LAPACK's worst value per metric, from the committed JSON"""
    worst = json.load(open(BOUNDS_JSON))["worst"]
    return tuple(BOUND_FACTOR * worst[k] for k in ("E_w", "E_r", "E_o"))
