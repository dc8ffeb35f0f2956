"""Small dense matrices and pencils on which a one-workgroup-per-matrix eigensolver can go wrong (graded and glued input,
multiplicities, near-identity, zero columns in the reduction, ill-conditioned B), extended-precision eigenvalue references for
them, and column-wise / entry-wise error metrics in units of eps = 2^-52 (tests/test_batch_accuracy.py,
tests/golden/make_batch_accuracy_bounds.py).

References: real dense -> hard_band's Householder tridiagonalisation and bisection in longdouble; Hermitian -> the same on the
real embedding [[Re, -Im], [Im, Re]] of order 2 n, every second eigenvalue; pencils -> C = L^-1 A L^-H with the Cholesky factor
and the two triangular solves in mpmath at 50 digits (longdouble loses eps_LD cond(B) there), C rounded to longdouble, then the
dense route.  References are computed in the process and cached: the B matrices go through LAPACK's QR and are not bit-
reproducible across machines.

The second half serves the dense generalised solvers (tests/test_dense_pencil_accuracy.py,
tests/golden/make_dense_pencil_bounds.py): longdouble substitution and reduction with a given float64 factor as the stage
references, E_f / E_t / E_c, the case table of the whole solves, an exactly scaled copy of a pencil, and their bounds.

The last part serves the dense standard drivers and their stages (tests/test_dense_driver_accuracy.py,
tests/golden/make_dense_driver_bounds.py): the case table with its panel widths, E_s / E_q of a reduction with its Q formed, the
back-transformation reflector by reflector in longdouble (E_b), an exactly scaled copy of a standard problem, and their bounds.

A plain module: no fixtures, no pytest settings."""
import functools
import json
import os

import numpy as np

import hard_band as hb
from hard_band import BOUND_FACTOR, EPS, LD

KINDS = ("s", "h", "gev", "hgev", "window")
FAMILIES = ("random", "graded", "graded_rev", "glued_tri", "glued_rot", "half_integer", "identity_plus", "rank_one", "clement",
            "blocks", "frank", "diagonal", "identity", "zero")
# every kernel instance (n-classes 32, 64, 96, 128) from both sides of an edge, both parities (the halves split the columns at
# (l + 2) / 2)
SIZES = {"s": (5, 32, 33, 64, 65, 96, 97, 128), "h": (5, 32, 33, 64, 65, 96), "gev": (5, 33, 64, 96), "hgev": (5, 33, 65),
         "window": (33, 96, 97, 128)}
PENCIL_A = ("random", "glued_rot")
PENCIL_C = (0, 1, 4, 8)                         # B = I (0) or Q diag(logspace(0, -c)) Q^H: cond_2(B) = 10^c
BOUNDS_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_accuracy_bounds.json")
METRICS = ("E_w", "E_r", "E_o")
PENCIL_METRICS = ("E_w", "E_r", "E_o", "E_f")
# the dense Cholesky-route and spectral-route solvers (tests/test_dense_pencil_accuracy.py): sizes of the stage cases and of the
# whole solves, and the record of what LAPACK reaches on them
DENSE_BOUNDS_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dense_pencil_bounds.json")
STAGE_SIZES = (1, 2, 63, 64, 65, 130, 200, 330)
STAGE_NRHS = 7                                  # the widest nrhs of the solve stage besides n
DENSE_SIZES = (65, 130)
STAGES = {"chol": ("E_f",), "trsm": ("E_t",), "reduce": ("E_c",)}


def window_width(n):
    """the widest window the window kernel serves in mode 'A' at this n"""
    return 16 if n <= 96 else 4


# ------------------------------------------------------------------------------------------------ matrices
def _from_upper(M):
    """the symmetric / Hermitian matrix that the upper triangle of M defines (of the diagonal the real parts): what a solver
    that reads the upper triangle sees"""
    U = np.triu(M, 1)
    return np.ascontiguousarray(U + U.conj().T + np.diag(np.diag(M).real))


def _rng(seed, n, k):
    return np.random.default_rng([seed, n, k])


def _normal(r, shape, cplx):
    return r.standard_normal(shape) + (1j * r.standard_normal(shape) if cplx else 0.0)


def _q(r, n, cplx):
    return np.linalg.qr(_normal(r, (n, n), cplx))[0]


def _sym(r, n, cplx):
    S = _normal(r, (n, n), cplx)
    return S + S.conj().T


def _phased(r, T, cplx):
    """D T D^H with unit phases D: a real matrix as a Hermitian one of the same spectrum"""
    if not cplx:
        return T
    ph = np.exp(1j * r.uniform(0.0, 2.0 * np.pi, T.shape[0]))
    return ph[:, None] * T * ph.conj()[None, :]


def _glued(n):
    """glued Wilkinson: blocks W21 (diagonal |i - 10|, off-diagonal 1) glued by 1e-10"""
    i = np.arange(n)
    e = np.ones(max(n - 1, 0))
    e[20::21] = 1e-10
    return np.diag(np.abs((i % 21) - 10.0)) + np.diag(e, 1) + np.diag(e, -1)


def half_integer_spectrum(n, seed=0):
    """the ascending diagonal of the half_integer family before rotation and perturbation: multiples of 1/2, most repeated"""
    return np.sort(np.round(2 * _rng(seed, n, 5).standard_normal(n)) / 2)


def matrix(family, n, cplx=False, seed=0):
    """one matrix of the table, float64 or complex128, exactly symmetric / Hermitian with a real diagonal"""
    k = FAMILIES.index(family)
    r = _rng(seed, n, k)
    i = np.arange(n)
    g = 10.0 ** (-14.0 * i / max(n - 1, 1))
    if family == "random":
        M = _sym(r, n, cplx)
    elif family in ("graded", "graded_rev"):      # graded by 1e-14 across rows and columns, the large entries at the top left
        M = g[:, None] * _sym(_rng(seed, n, 1), n, cplx) * g[None, :]
        M = M[::-1, ::-1] if family == "graded_rev" else M
    elif family == "glued_tri":
        M = _phased(r, _glued(n), cplx)
    elif family == "glued_rot":
        Q = _q(r, n, cplx)
        M = Q @ _glued(n) @ Q.conj().T
    elif family == "half_integer":                # multiplicities, split at the 1e-9 level
        Q = _q(r, n, cplx)
        M = (Q * half_integer_spectrum(n, seed)) @ Q.conj().T + 1e-9 * _sym(r, n, cplx)
    elif family == "identity_plus":
        M = np.eye(n) + 1e-15 * _sym(r, n, cplx)
    elif family == "rank_one":                    # an (n - 1)-fold eigenvalue 1
        v = _normal(r, n, cplx)
        M = np.eye(n) + np.outer(v, v.conj())
    elif family == "clement":
        off = np.sqrt(i[1:] * (n - i[1:]).astype(np.float64))
        M = _phased(r, np.diag(off, 1) + np.diag(off, -1), cplx)
    elif family == "blocks":                      # block diagonal, blocks of 7 of scale 1 and 1e-8: zero columns in the reduction
        M = np.zeros((n, n), dtype=np.complex128 if cplx else np.float64)
        for b, s in enumerate(range(0, n, 7)):
            t = min(s + 7, n)
            M[s:t, s:t] = (1.0 if b % 2 == 0 else 1e-8) * _sym(r, t - s, cplx)
    elif family == "frank":
        M = _phased(r, np.minimum.outer(i + 1, i + 1).astype(np.float64), cplx)
    elif family == "diagonal":
        M = np.diag(r.standard_normal(n))
    elif family == "identity":
        M = np.eye(n)
    elif family == "zero":
        M = np.zeros((n, n))
    else:
        raise ValueError(family)
    return _from_upper(np.asarray(M, dtype=np.complex128 if cplx else np.float64))


def overlap(n, c, cplx=False, seed=0):
    """B of a pencil: the identity (c = 0) or Q diag(logspace(0, -c, n)) Q^H"""
    if c == 0:
        return np.eye(n, dtype=np.complex128 if cplx else np.float64)
    Q = _q(_rng(seed, n, 100 + c), n, cplx)
    return _from_upper((Q * np.logspace(0.0, -float(c), n)) @ Q.conj().T)


def windows(n):
    """(il, iu, mode) of the window kind, 1-based: the lowest and the highest MW, (1, 1), (n, n), MW in the middle starting and
    ending inside a cluster of the half_integer family, and one mode 'N' window of width n"""
    mw = window_width(n)
    d = half_integer_spectrum(n)
    inside = [il for il in range(2, n - mw + 1) if d[il - 2] == d[il - 1] and d[il + mw - 2] == d[il + mw - 1]]
    assert inside, n
    il = min(inside, key=lambda q: abs(q - (n - mw) // 2))
    return [(1, mw, "A"), (n - mw + 1, n, "A"), (1, 1, "A"), (n, n, "A"), (il, il + mw - 1, "A"), (1, n, "N")]


def cases(kind):
    """the case table of one kind: (n, family) for s and h, (n, family of A, c) for gev and hgev, (n, family, il, iu, mode) for
    window.  Pencils at n = 96 come with c = 4 only (their references dominate the run time)."""
    if kind in ("s", "h"):
        return [(n, f) for n in SIZES[kind] for f in FAMILIES]
    if kind in ("gev", "hgev"):
        return [(n, f, c) for n in SIZES[kind] for f in PENCIL_A for c in ((4,) if n == 96 else PENCIL_C)]
    if kind == "window":
        return [(n, f, il, iu, mode) for n in SIZES[kind] for il, iu, mode in windows(n) for f in FAMILIES]
    raise ValueError(kind)


def case_id(kind, case):
    if kind in ("s", "h"):
        return f"{kind}-n{case[0]}-{case[1]}"
    if kind in ("gev", "hgev"):
        return f"{kind}-n{case[0]}-{case[1]}-c{case[2]}"
    return f"window-n{case[0]}-{case[1]}-{case[2]}-{case[3]}-{case[4]}"


# ------------------------------------------------------------------------------------------------ references
def embed(A):
    """the real symmetric [[Re, -Im], [Im, Re]] of order 2 n: every eigenvalue of the Hermitian A twice"""
    return np.block([[A.real, -A.imag], [A.imag, A.real]])


def reference_eigenvalues(A):
    """ascending eigenvalues of the symmetric or Hermitian A (float64, longdouble or their complex types) in longdouble"""
    A = np.asarray(A)
    if not A.any():                               # the zero matrix: what the bisection returns after 9 s at n = 330
        return np.zeros(A.shape[0], dtype=LD)
    with np.errstate(over="ignore"):             # a Sturm pivot of 1e-4900 next to a double eigenvalue: e^2 / q = inf is meant
        if np.iscomplexobj(A):
            return np.sort(hb._bisect_tridiagonal(*hb._householder_tridiagonalise(embed(A))))[::2].copy()
        return np.sort(hb._bisect_tridiagonal(*hb._householder_tridiagonalise(A)))


def _to_ld(x):
    """an mpmath real rounded to longdouble (two float64 pieces: 106 bits)"""
    hi = float(x)
    return LD(hi) + LD(float(x - hi))


def reduced_pencil(A, B):
    """C = L^-1 A L^-H, B = L L^H, in mpmath at 50 digits, rounded to longdouble (clongdouble for complex input)"""
    import mpmath

    n = A.shape[0]
    cplx = np.iscomplexobj(A) or np.iscomplexobj(B)
    with mpmath.workdps(50):
        num = (lambda x: mpmath.mpc(x.real, x.imag)) if cplx else (lambda x: mpmath.mpf(float(x)))
        conj = mpmath.conj if cplx else (lambda x: x)
        zero = mpmath.mpf(0)
        Lr = [[zero] * n for _ in range(n)]      # rows of L
        for j in range(n):
            s = mpmath.re(num(B[j, j])) - mpmath.fsum(abs(x) ** 2 for x in Lr[j][:j])
            assert s > 0, "B is not positive definite"
            Lr[j][j] = mpmath.sqrt(s)
            cj = [conj(x) for x in Lr[j][:j]]
            for i in range(j + 1, n):
                Lr[i][j] = (num(B[i, j]) - mpmath.fdot(Lr[i][:j], cj)) / Lr[j][j]

        def solve_columns(cols):
            """L^-1 applied to every column"""
            out = []
            for x in cols:
                y = []
                for i in range(n):
                    y.append((x[i] - mpmath.fdot(Lr[i][:i], y)) / Lr[i][i])
                out.append(y)
            return out

        X = solve_columns([[num(A[i, j]) for i in range(n)] for j in range(n)])        # X[j][i] = (L^-1 A)(i, j)
        # C = X L^-H = (L^-1 X^H)^H: the columns of X^H are the conjugated rows of X
        Y = solve_columns([[conj(X[j][i]) for j in range(n)] for i in range(n)])       # Y[i][j] = conj(C(i, j))
        C = np.zeros((n, n), dtype=np.clongdouble if cplx else LD)
        for i in range(n):
            for j in range(n):
                v = conj(Y[i][j])
                C[i, j] = _to_ld(mpmath.re(v)) + (1j * _to_ld(mpmath.im(v)) if cplx else 0)
    return (C + C.conj().T) / 2


class Case:
    """one standard problem: A, its reference eigenvalues lam (longdouble, ascending, read-only) and |A|_2"""

    def __init__(self, kind, n, family):
        self.kind, self.n, self.family = kind, n, family
        self.A = matrix(family, n, cplx=kind == "h")
        self.A.setflags(write=False)
        self.lam = reference_eigenvalues(self.A)
        self.lam.setflags(write=False)
        self.anorm = float(np.abs(self.lam).max())


class Pencil:
    """one pencil: A, B, the reference eigenvalues lam, |A|_2, |B|_2 and cond_2(B)"""

    def __init__(self, kind, n, family, c):
        cplx = kind == "hgev"
        self.kind, self.n, self.family, self.c = kind, n, family, c
        self.A = matrix(family, n, cplx=cplx)
        self.B = overlap(n, c, cplx=cplx)
        self.A.setflags(write=False)
        self.B.setflags(write=False)
        self.lam = reference_eigenvalues(reduced_pencil(self.A, self.B))
        self.lam.setflags(write=False)
        self.anorm = float(np.abs(np.linalg.eigvalsh(self.A)).max())
        wb = np.linalg.eigvalsh(self.B)
        self.bnorm, self.cond = float(wb[-1]), float(wb[-1] / wb[0])


@functools.lru_cache(maxsize=None)
def case(kind, n, family):
    """the standard problem (kind s or h; the window kind uses s), computed once per process"""
    return Case("s" if kind == "window" else kind, n, family)


@functools.lru_cache(maxsize=None)
def pencil(kind, n, family, c):
    """the pencil (kind gev or hgev), its reference computed once per process"""
    return Pencil(kind, n, family, c)


# ------------------------------------------------------------------------------------------------ metrics
def metrics(cs, w, Z, il=1):
    """(E_w, E_r, E_o) of the columns il .. il + m - 1 of a standard problem, in eps: E_w = max |w_k - lambda_k| / (eps |A|_2),
    E_r = max_j |A z_j - w_j z_j|_2 / (eps |A|_2), E_o = max |Z^H Z - I| / eps.  Z = None: E_w only (the others 0).  The zero
    matrix: its w is held to 0 exactly by the caller; E_w and E_r are 0 here."""
    w = np.asarray(w, dtype=np.float64)
    m = len(w)
    tn = cs.anorm if cs.anorm > 0 else 1.0
    E_w = float(np.abs(w.astype(LD) - cs.lam[il - 1:il - 1 + m]).max()) / (EPS * tn)
    if Z is None:
        return E_w, 0.0, 0.0
    if np.iscomplexobj(cs.A):
        E_r, _ = hb.dense_metrics(embed(cs.A), w, np.vstack([Z.real, Z.imag]))
        E_o = float(np.abs(Z.conj().T @ Z - np.eye(m)).max()) / EPS
    else:
        E_r, E_o = hb.dense_metrics(cs.A, w, np.asarray(Z, dtype=np.float64))
    return E_w, E_r, E_o


def pencil_metrics(pc, w, Z, U, il=1):
    """(E_w, E_r, E_o, E_f) of the columns il .. il + m - 1 of a pencil in eps, products in longdouble: E_w = max_k |w_k -
    lambda_k| / (eps cond(B) max(|lambda_k|, |A|_2 / |B|_2)), E_r = max_j |A z_j - w_j B z_j|_2 / (eps cond(B) (|A|_2 + |w_j|
    |B|_2) |z_j|_2), E_o = max |Z^H B Z - I| / (eps cond(B)), E_f = max |U^H U - B| / (eps |B|_2) for the returned factor (U =
    None: 0)"""
    cplx = np.iscomplexobj(pc.A)
    T = np.clongdouble if cplx else LD
    w = np.asarray(w, dtype=np.float64)
    m = len(w)
    lam = pc.lam[il - 1:il - 1 + m]
    ek = EPS * pc.cond
    den = np.maximum(np.abs(lam), LD(pc.anorm / pc.bnorm))
    den = np.where(den > 0, den, LD(1))
    E_w = float((np.abs(w.astype(LD) - lam) / den).max()) / ek
    Zl, Al, Bl = np.asarray(Z, dtype=T), np.asarray(pc.A, dtype=T), np.asarray(pc.B, dtype=T)
    BZ = Bl @ Zl
    R = Al @ Zl - BZ * w.astype(LD)[None, :]
    rn = np.sqrt((np.abs(R) ** 2).sum(axis=0))
    zn = np.sqrt((np.abs(Zl) ** 2).sum(axis=0))
    scale = (LD(pc.anorm) + np.abs(w).astype(LD) * LD(pc.bnorm)) * zn
    scale = np.where(scale > 0, scale, LD(1))
    E_r = float((rn / scale).max()) / ek
    E_o = float(np.abs(Zl.conj().T @ BZ - np.eye(m)).max()) / ek
    E_f = 0.0
    if U is not None:
        Ul = np.asarray(U, dtype=T)
        E_f = float(np.abs(Ul.conj().T @ Ul - Bl).max()) / (EPS * pc.bnorm)
    return E_w, E_r, E_o, E_f


# ------------------------------------------------------------------------------------------------ bounds
@functools.lru_cache(maxsize=None)
def _record():
    return json.load(open(BOUNDS_JSON))


def bounds(kind, c=None, family=None):
    """the bounds in force, {metric: bound}: BOUND_FACTOR x LAPACK's worst value per (kind, metric), for pencils per cond group
    c; the window kind uses those of s.  A family the record lists under "family_bounds" has its own (with the reason there)."""
    rec = _record()
    kind = "s" if kind == "window" else kind
    worst = rec["worst"][kind] if c is None else rec["worst"][kind][f"c{c}"]
    out = {k: BOUND_FACTOR * v for k, v in worst.items()}
    own = rec.get("family_bounds", {}).get(f"{kind}-{family}")
    if own:
        out.update(own["bounds"])
    return out


# ------------------------------------------------------------------------------------------------ dense pencils: stages
def nan_lower(M, diag=True):
    """M with NaN in the strict lower triangle and, for a complex M (unless diag is False), in Im of the diagonal: what a
    routine that reads the upper triangle only must not notice"""
    M = np.array(M)
    lower = np.tril(np.ones(M.shape, dtype=bool), -1)
    if np.iscomplexobj(M):
        M[lower] = np.nan + 1j * np.nan
        if diag:
            M.imag[np.diag_indices(M.shape[0])] = np.nan
    else:
        M[lower] = np.nan
    return M


def upper_of(M):
    """the upper triangular matrix a routine has left in the upper triangle of M (the strict lower triangle as zero)"""
    return np.triu(np.nan_to_num(np.asarray(M), nan=0.0))


def solve_upper_ld(U, R, trans):
    """op(U)^-1 R for the upper triangular U by substitution in longdouble / clongdouble: trans 'N' -> U, anything else ->
    U^H.  All right-hand sides advance together, one row of U per step."""
    cplx = np.iscomplexobj(U) or np.iscomplexobj(R)
    T = np.clongdouble if cplx else LD
    Ul, X = np.asarray(U, dtype=T), np.array(R, dtype=T)
    n = Ul.shape[0]
    if trans == "N":
        for i in range(n - 1, -1, -1):
            X[i] = (X[i] - Ul[i, i + 1:] @ X[i + 1:]) / Ul[i, i]
    else:
        L = Ul.conj().T
        for i in range(n):
            X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def reduce_ld(A, U):
    """U^-H A U^-1 by two substitutions in longdouble with the float64 U as it is"""
    X = solve_upper_ld(U, A, "C")                             # U^-H A
    return solve_upper_ld(U, X.conj().T, "C").conj().T        # (U^-H (U^-H A)^H)^H


class Stage:
    """what the stage tests of one (kind, n, c) share: B = overlap(n, c), its float64 factor U from LAPACK (B = U^H U: the solve
    and reduction stages are judged independently of the project's factorisation), |B|_2, |U^-1|_2^2, max(n, STAGE_NRHS) seeded
    normal right-hand sides R (so that every nrhs the tests pass has that many columns behind it) and op(U)^-1 R for both ops
    in longdouble.  Read-only."""

    def __init__(self, kind, n, c):
        import scipy.linalg

        cplx = kind == "hgev"
        self.kind, self.n, self.c = kind, n, c
        self.B = overlap(n, c, cplx=cplx)
        self.U = np.triu(scipy.linalg.cholesky(self.B))
        sv = np.linalg.svd(self.U, compute_uv=False)
        self.bnorm, self.uinv2 = float(np.linalg.eigvalsh(self.B)[-1]), float(sv[-1] ** -2.0)
        self.R = _normal(_rng(1, n, 200 + c), (n, n), cplx)
        if n < STAGE_NRHS:                         # the first n columns stay what they were: LAPACK's record is taken on those
            self.R = np.hstack([self.R, _normal(_rng(1, n, 300 + c), (n, STAGE_NRHS - n), cplx)])
        self.X = {"N": solve_upper_ld(self.U, self.R, "N"), "C": solve_upper_ld(self.U, self.R, "C")}
        for M in (self.B, self.U, self.R, self.X["N"], self.X["C"]):
            M.setflags(write=False)


class Reduction:
    """A = matrix(family, n), U of stage(kind, n, c), |A|_2 and C_ref = U^-H A U^-1 in longdouble.  Read-only."""

    def __init__(self, kind, n, family, c):
        self.st = stage(kind, n, c)
        self.A = matrix(family, n, cplx=kind == "hgev")
        self.anorm = float(np.abs(np.linalg.eigvalsh(self.A)).max())
        self.C = reduce_ld(self.A, self.st.U)
        self.A.setflags(write=False)
        self.C.setflags(write=False)


@functools.lru_cache(maxsize=None)
def stage(kind, n, c):
    return Stage(kind, n, c)


@functools.lru_cache(maxsize=None)
def reduction(kind, n, family, c):
    return Reduction(kind, n, family, c)


def factor_error(B, U, bnorm):
    """E_f = max |U^H U - B| / (eps |B|_2), the product in longdouble"""
    T = np.clongdouble if np.iscomplexobj(B) else LD
    Ul = np.asarray(U, dtype=T)
    return float(np.abs(Ul.conj().T @ Ul - np.asarray(B, dtype=T)).max()) / (EPS * bnorm)


def solve_error(X, Xref):
    """E_t = max_j |x_j - xref_j|_2 / (eps |xref_j|_2), column by column"""
    T = Xref.dtype
    d = np.sqrt((np.abs(np.asarray(X, dtype=T) - Xref) ** 2).sum(axis=0))
    r = np.sqrt((np.abs(Xref) ** 2).sum(axis=0))
    return float((d / np.where(r > 0, r, LD(1))).max()) / EPS


def solve_residual(U, X, R, trans):
    """max_j |op(U) x_j - r_j|_2 / (eps |U|_2 |x_j|_2) in longdouble: reported, not bounded (substitution's is ten times smaller
    than a correct block inversion's for op = U^H)"""
    T = np.clongdouble if np.iscomplexobj(U) or np.iscomplexobj(X) else LD
    Ul, Xl = np.asarray(U, dtype=T), np.asarray(X, dtype=T)
    D = (Ul if trans == "N" else Ul.conj().T) @ Xl - np.asarray(R, dtype=T)
    d = np.sqrt((np.abs(D) ** 2).sum(axis=0))
    x = np.sqrt((np.abs(Xl) ** 2).sum(axis=0))
    return float((d / np.where(x > 0, x, LD(1))).max()) / (EPS * float(np.linalg.norm(U, 2)))


def reduction_error(rd, Cu):
    """E_c = max over the upper triangle of |C - C_ref| / (eps |U^-1|_2^2 |A|_2); of a complex C's diagonal the real part"""
    C = np.array(Cu)
    if np.iscomplexobj(C):
        C[np.diag_indices(rd.st.n)] = C.real.diagonal()
    up = np.triu_indices(rd.st.n)
    scale = rd.st.uinv2 * (rd.anorm if rd.anorm > 0 else 1.0)
    return float(np.abs(np.asarray(C, dtype=rd.C.dtype)[up] - rd.C[up]).max()) / (EPS * scale)


# ------------------------------------------------------------------------------------------------ dense pencils: whole solves
def dense_cases(kind):
    """(n, family of A, c) of the whole solves: every pencil at n = 65; at n = 130 every real one and, of the complex ones,
    (glued_rot, 8) alone (their references take 10 s each)"""
    out = [(65, f, c) for f in PENCIL_A for c in PENCIL_C]
    if kind == "gev":
        return out + [(130, f, c) for f in PENCIL_A for c in PENCIL_C]
    return out + [(130, "glued_rot", 8)]


class ScaledPencil:
    """the pencil (A 2^ka, B 2^kb) of pc: the scaling and with it the reference (lam 2^(ka - kb)) are exact, cond(B) is that of
    pc, and every metric of pencil_metrics is invariant"""

    def __init__(self, pc, ka, kb):
        self.kind, self.n, self.family, self.c, self.cond = pc.kind, pc.n, pc.family, pc.c, pc.cond
        sc = (lambda M, k: np.ldexp(M.real, k) + 1j * np.ldexp(M.imag, k)) if np.iscomplexobj(pc.A) else np.ldexp
        self.A, self.B = sc(pc.A, ka), sc(pc.B, kb)
        self.lam = pc.lam * LD(2) ** (ka - kb)
        self.anorm, self.bnorm = float(np.ldexp(pc.anorm, ka)), float(np.ldexp(pc.bnorm, kb))
        for M in (self.A, self.B, self.lam):
            M.setflags(write=False)


def windows_dense(n):
    """(il, iu) of the range solvers' cases, 1-based: everything, the lowest 8, the highest 8, 8 in the middle"""
    mid = (n - 8) // 2 + 1
    return [(1, n), (1, 8), (n - 7, n), (mid, mid + 7)]


def basis_error(pc, F):
    """max |F^H B F - I| / (eps cond(B)) for the B-orthonormal basis the spectral route returns, products in longdouble"""
    T = np.clongdouble if np.iscomplexobj(pc.A) else LD
    Fl = np.asarray(F, dtype=T)
    return float(np.abs(Fl.conj().T @ (np.asarray(pc.B, dtype=T) @ Fl) - np.eye(pc.n)).max()) / (EPS * pc.cond)


@functools.lru_cache(maxsize=None)
def _dense_record():
    return json.load(open(DENSE_BOUNDS_JSON))


def dense_bounds(kind, c, route=None):
    """the bounds of the whole solves, {metric: bound}: BOUND_FACTOR x what LAPACK's gv / gvd and potrf reach at worst on
    dense_cases(kind) in the cond group c.  A route ("cholesky", "spectral") the record lists under "family_bounds" as
    kind-route has bounds of its own there, per cond group, with the reason."""
    rec = _dense_record()
    out = {k: BOUND_FACTOR * v for k, v in rec["worst"][kind]["whole"][f"c{c}"].items()}
    own = rec.get("family_bounds", {}).get(f"{kind}-{route}")
    if own:
        out.update(own["bounds"].get(f"c{c}", {}))
    return out


def stage_bounds(kind, what):
    """the bounds of one stage (chol, trsm, reduce), {metric: bound}: BOUND_FACTOR x LAPACK's worst value (potrf, trtrs, sygst /
    hegst) over STAGE_SIZES and PENCIL_C"""
    return {k: BOUND_FACTOR * v for k, v in _dense_record()["worst"][kind][what].items()}


# ------------------------------------------------------------------------------------------------ dense standard drivers
# eigx_sx / eigx_s / eigx_h and their stages eigx_band_reduce_dev / eigx_trbak_dev (tests/test_dense_driver_accuracy.py,
# tests/golden/make_dense_driver_bounds.py)
DRIVER_BOUNDS_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dense_driver_bounds.json")
# (n, m_forward, m_backward, q), q = eigx_tune key 2 (super-block factor of the back-transformation): the smallest sizes with
# more than one panel, a partial last panel and a partial last back-transformation block; (330, 32, 128, 2) has one super-block
# of 256 reflectors and a head range of 72 (band 1) / 71 (band 2), (517, 64, 128, 4) one super-block of 512
DRIVER_TABLE = ((5, 4, 8, 0), (65, 16, 16, 0), (130, 48, 48, 0), (330, 128, 128, 0), (330, 32, 128, 2), (517, 64, 128, 4))
DRIVER_LARGE_FAMILIES = ("random", "graded", "glued_rot", "blocks")         # the families at n = 517
DRIVER_H_TABLE = ((5, 4, 8, 0), (17, 4, 8, 0), (65, 16, 16, 0), (130, 48, 48, 0), (200, 48, 48, 0))
DRIVER_STAGES = {"reduce": ("E_s", "E_q"), "trbak": ("E_b",), "whole": METRICS}
BACK_INPUTS = ("identity", "normal", "scaled")
# reflector norms over 14 decades (graded both ways), trivial reflectors (glued_tri, diagonal) and whole trivial blocks (blocks)
BACK_FAMILIES = ("graded", "graded_rev", "blocks", "diagonal", "glued_tri", "random")


def driver_table(kind):
    return DRIVER_H_TABLE if kind == "h" else DRIVER_TABLE


def driver_families(n):
    return DRIVER_LARGE_FAMILIES if n > 330 else FAMILIES


def driver_cases(kind, max_n=None):
    """the case table of the dense drivers, kind s or h: (n, m_forward, m_backward, q, family)"""
    return [row + (f,) for row in driver_table(kind) if max_n is None or row[0] <= max_n for f in driver_families(row[0])]


def driver_problems(kind):
    """(n, family) of the table without repetition: what LAPACK's record is taken on (it has no panel widths)"""
    return sorted({(c[0], c[4]) for c in driver_cases(kind)}, key=lambda c: (c[0], FAMILIES.index(c[1])))


def driver_case_id(kind, c):
    return f"{kind}-n{c[0]}-mf{c[1]}-mb{c[2]}-q{c[3]}-{c[4]}"


def similarity_metrics(A, Q, T=None, anorm=None):
    """(E_s, E_q) of a reduction A -> T = Q^H A Q in eps, products in longdouble / clongdouble: E_s = max |Q^H A Q - T| /
    (eps |A|_2) over all entries, E_q = max |Q^H Q - I| / eps.  anorm = |A|_2 (Case.anorm; LAPACK's if None), 1 for the zero
    matrix.  T = None (a driver that does not return (d, e)): T is the real part of the tridiagonal part of Q^H A Q itself, so
    that E_s measures what lies outside the band and the imaginary part inside it."""
    cplx = np.iscomplexobj(A) or np.iscomplexobj(Q)
    Tt = np.clongdouble if cplx else LD
    if anorm is None:
        anorm = float(np.abs(np.linalg.eigvalsh(A)).max())
    anorm = anorm if anorm > 0 else 1.0
    Ql = np.asarray(Q, dtype=Tt)
    S = Ql.conj().T @ (np.asarray(A, dtype=Tt) @ Ql)
    n = S.shape[0]
    if T is None:
        i, j = np.indices((n, n))
        T = np.where(np.abs(i - j) <= 1, S.real, LD(0))
    E_s = float(np.abs(S - np.asarray(T, dtype=Tt)).max()) / (EPS * anorm)
    E_q = float(np.abs(Ql.conj().T @ Ql - np.eye(n)).max()) / EPS
    return E_s, E_q


def apply_reflectors_ld(refl, e, band, Z):
    """the back-transformation H_(n-1) ... H_band Z reflector by reflector in longdouble, from the stored form of the band
    reduction: H_i = I - u u^T / beta_i with the un-normalised u = refl[0:L, i], L = i - band + 1, and beta_i = -u_(L-1)
    e[band-1, i] (a zero beta is the identity), as orc_trbak of oracle/eigx_oracle.c recovers it.  Returns Z_ref (longdouble);
    E_b = solve_error(Z, Z_ref) = max_j |z_j - zref_j|_2 / (eps |zref_j|_2)."""
    R = np.asarray(refl, dtype=LD)
    el = np.asarray(e, dtype=LD).reshape(band, -1)
    X = np.array(Z, dtype=LD)
    for i in range(band, R.shape[0]):
        L = i - band + 1
        beta = -R[L - 1, i] * el[band - 1, i]
        if beta == 0:
            continue
        u = R[:L, i]
        X[:L] -= np.outer(u, (u @ X[:L]) / beta)
    return X


def back_input(n, which, cplx=False):
    """seeded Z of the back-transformation tests: the identity, normal random, normal random with the columns scaled by
    logspace(0, -14)"""
    if which == "identity":
        return np.eye(n, dtype=np.complex128 if cplx else np.float64)
    Z = _normal(_rng(2, n, 400), (n, n), cplx)
    if which == "scaled":
        Z = Z * np.logspace(0.0, -14.0, n)[None, :]
    elif which != "normal":
        raise ValueError(which)
    return Z


class ScaledDense:
    """the standard problem A 2^k of a Case: the scaling and with it the reference (lam 2^k) are exact, and every metric of
    metrics and similarity_metrics is invariant"""

    def __init__(self, cs, k):
        self.kind, self.n, self.family, self.k = cs.kind, cs.n, cs.family, k
        self.A = (np.ldexp(cs.A.real, k) + 1j * np.ldexp(cs.A.imag, k)) if np.iscomplexobj(cs.A) else np.ldexp(cs.A, k)
        self.lam = cs.lam * LD(2) ** k
        self.anorm = float(np.ldexp(cs.anorm, k))
        self.A.setflags(write=False)
        self.lam.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _driver_record():
    return json.load(open(DRIVER_BOUNDS_JSON))


def driver_stage_bounds(kind, what, family=None):
    """the bounds of one stage of the dense drivers (reduce: E_s, E_q; trbak: E_b; whole: E_w, E_r, E_o), {metric: bound}:
    BOUND_FACTOR x LAPACK's worst value over the table (sytrd / hetrd with Q formed, ormqr / unmqr, syevd / heevd).  A family
    the record lists under "family_bounds" as kind-family has bounds of its own there, per stage, with the reason and the
    measured value."""
    rec = _driver_record()
    out = {k: BOUND_FACTOR * v for k, v in rec["worst"][kind][what].items()}
    own = rec.get("family_bounds", {}).get(f"{kind}-{family}")
    if own:
        out.update(own["bounds"].get(what, {}))
    return out


def driver_bounds(kind, family=None):
    """the bounds of the whole solves of eigx_sx / eigx_s (kind s) and eigx_h (kind h)"""
    return driver_stage_bounds(kind, "whole", family)
