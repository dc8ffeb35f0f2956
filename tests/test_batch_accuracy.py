"""The one-workgroup-per-matrix eigensolvers (eigen_s_batch, eigen_h_batch, eigen_gev_batch, eigen_hgev_batch, their ragged
forms and the window kernel of eigen_s_batch_range) held to LAPACK-level accuracy on small hard matrices (tests/hard_dense.py):
graded and glued input, multiplicities, near-identity, zero columns in the reduction, B of cond 1e1 .. 1e8, judged column by
column and entry by entry against extended-precision references.

Bounds: 16 x what LAPACK reaches on the same case table (tests/golden/batch_accuracy_bounds.json, written by
tests/golden/make_batch_accuracy_bounds.py), per kind and metric, for the pencils per cond group; the window kind uses those of
s.  They come from an independent implementation of the operation, never from the code under test.  A bound of 0 (the factor of
B = I) asks for exactly 0: every comparison is <=.

The existing gates of the batched tests (residual 768, eigenvalues to 1e-12, pencils 1e-12 scale n) pass a solver that loses
three digits; test_bounds_bite shows on a numpy restatement of the algorithm (tred2 + tql2 with the deflation factor as a
parameter) that these bounds do not.

Measured on an MI355X (worst per kind over the table, in eps; LAPACK's worst beside it): see DESIGN section 8h-A and
profiles/batch_accuracy.log."""
import json
import math

import numpy as np
import pytest

import hard_band as hb
import hard_dense as hd

EPS, LD = hd.EPS, hd.LD
POW2 = (400, -400, 700, -700)                    # A 2^k: all outside [1e-90, 1e90], the kernels rescale by a power of two


def _judge(kind, tag, names, values, bnd):
    line = " ".join(f"{k}={v:.3f} (<={bnd[k]:.2f})" for k, v in zip(names, values))
    print(f"BATCH-ACC {kind} {tag}: {line}")
    bad = [k for k, v in zip(names, values) if not v <= bnd[k]]
    assert not bad, (kind, tag, bad, values)
    return values


def _check_standard(kind, tag, cs, w, Z, il=1, label=None):
    """finite, ascending, the zero matrix's w exactly 0, every metric at or under the bound of its kind"""
    assert np.isfinite(w).all() and (Z is None or np.isfinite(Z).all()), tag
    assert (np.diff(w) >= 0).all(), f"{tag}: w is not ascending"
    if not cs.A.any():
        assert (w == 0.0).all(), f"{tag}: the zero matrix"
    names = hd.METRICS if Z is not None else hd.METRICS[:1]
    return _judge(label or kind, tag, names, hd.metrics(cs, w, Z, il), hd.bounds(kind, family=cs.family))


def _check_pencil(kind, tag, pc, w, Z, U, label=None):
    assert np.isfinite(w).all() and np.isfinite(Z).all() and np.isfinite(U).all(), tag
    assert (np.diff(w) >= 0).all(), f"{tag}: w is not ascending"
    return _judge(label or kind, tag, hd.PENCIL_METRICS, hd.pencil_metrics(pc, w, Z, U), hd.bounds(kind, c=pc.c, family=pc.family))


# ------------------------------------------------------------------------------------------------ the algorithm, restated
def tred2_tql2(A, factor=0.5):
    """Householder tridiagonalisation in tred2's order (i = n-1 .. 1, no column scaling) and implicit QL with Wilkinson shift
    (tql2), plain numpy float64: the algorithm class of the batched kernels, not their code.  e[m] counts as negligible when
    |e[m]| <= factor eps (|d[m]| + |d[m+1]|), eps = 2^-52.  Returns ascending w and Z."""
    A = np.array(A, dtype=np.float64)
    n = A.shape[0]
    Q, e = np.eye(n), np.zeros(n)
    for i in range(n - 1, 0, -1):
        u = A[:i, i].copy()
        h = u @ u
        if i == 1 or h == 0.0:
            e[i] = u[i - 1]
            continue
        g = -math.copysign(math.sqrt(h), u[i - 1])
        h -= u[i - 1] * g
        u[i - 1] -= g
        p = A[:i, :i] @ u / h
        q = p - (u @ p) / (2 * h) * u
        A[:i, :i] -= np.outer(u, q) + np.outer(q, u)
        Q[:, :i] -= np.outer(Q[:, :i] @ u, u) / h             # Q <- Q H_i
        e[i] = g
    d = np.diagonal(A).copy()
    e = np.r_[e[1:], 0.0]
    tol, sweeps = factor * EPS, 0
    for l in range(n):
        while True:
            m = l
            while m < n - 1 and abs(e[m]) > tol * (abs(d[m]) + abs(d[m + 1])):
                m += 1
            if m == l:
                break
            sweeps += 1
            assert sweeps <= 30 * n, "no convergence"
            g = (d[l + 1] - d[l]) / (2 * e[l])
            g = d[m] - d[l] + e[l] / (g + math.copysign(math.hypot(g, 1.0), g))
            s = c = 1.0
            p = 0.0
            for i in range(m - 1, l - 1, -1):
                f, b = s * e[i], c * e[i]
                r = math.hypot(f, g)
                e[i + 1] = r
                if r == 0.0:                                   # recover from underflow
                    d[i + 1] -= p
                    e[m] = 0.0
                    break
                s, c = f / r, g / r
                g = d[i + 1] - p
                r = (d[i] - g) * s + 2 * c * b
                p = s * r
                d[i + 1] = g + p
                g = c * r - b
                zi, zn = Q[:, i].copy(), Q[:, i + 1].copy()
                Q[:, i + 1] = s * zi + c * zn
                Q[:, i] = c * zi - s * zn
            else:
                d[l] -= p
                e[l] = g
                e[m] = 0.0
    order = np.argsort(d, kind="stable")
    return d[order], Q[:, order]


def _old_gates(A, w, Z):
    """the gates of tests/test_batch.py: (|w - w_lapack| <= 1e-12 max(1, max|w|), residual ||A Z - Z W||_F / (n eps ||A||_F) <
    768, orthogonality ||Z^T Z - I||_F / (n eps) < 8) as booleans"""
    n = A.shape[0]
    wr = np.linalg.eigvalsh(A)
    anorm = np.linalg.norm(A)
    res = np.linalg.norm(A @ Z - Z * w) / (n * EPS * anorm) if anorm > 0 else float(np.abs(w).max())
    orth = np.linalg.norm(Z.T @ Z - np.eye(n)) / (n * EPS)
    return np.abs(w - wr).max() <= 1e-12 * max(1.0, np.abs(wr).max()), res < 768, orth < 8


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("n", [5, 33, 96])
def test_reference_matches_closed_forms(n):
    """the dense route against spectra known in closed form, to 0.1 eps |A|_2: Clement's integers (the off-diagonal formed in
    longdouble: rounded to float64 it is another matrix), the Toeplitz (2, -1) matrix rotated dense by a reflector formed in
    longdouble (orthogonal to 1e-19); the Hermitian route on the embedding of a real case and on i K, K the antisymmetric
    Toeplitz (1, -1) matrix with spectrum 2 cos(k pi / (n + 1))"""
    pi = 4 * np.arctan(LD(1))
    k = np.arange(1, n + 1).astype(LD)
    i = np.arange(1, n).astype(LD)
    off = np.sqrt(i * (n - i))
    w = hd.reference_eigenvalues(np.diag(off, 1) + np.diag(off, -1))
    assert float(np.abs(w - np.arange(-(n - 1), n, 2).astype(LD)).max()) <= 0.1 * EPS * (n - 1)
    T = 2 * np.eye(n, dtype=LD) - np.eye(n, k=1, dtype=LD) - np.eye(n, k=-1, dtype=LD)
    v = np.random.default_rng(n).standard_normal(n).astype(LD)
    H = np.eye(n, dtype=LD) - 2 * np.outer(v, v) / (v @ v)
    A = H @ T @ H
    assert np.count_nonzero(np.triu(A, 2)) > n                # dense
    exact = 4 * np.sin(k * pi / (2 * (n + 1))) ** 2            # 2 - 2 cos(k pi / (n + 1)) without the cancellation
    assert float(np.abs(hd.reference_eigenvalues((A + A.T) / 2) - exact).max()) <= 0.1 * EPS * 4
    cs = hd.case("s", n, "glued_rot")
    assert float(np.abs(hd.reference_eigenvalues(cs.A.astype(np.complex128)) - cs.lam).max()) <= 0.1 * EPS * cs.anorm
    K = np.eye(n, k=1) - np.eye(n, k=-1)
    exact = np.sort(2 * np.cos(k * pi / (n + 1)))
    assert float(np.abs(hd.reference_eigenvalues(1j * K) - exact).max()) <= 0.1 * EPS * 2


@pytest.mark.parametrize("kind,std", [("gev", "s"), ("hgev", "h")])
def test_pencil_reference(kind, std):
    """with B = I the pencil's reference is the dense one; with B = diag(4^-k) of cond 2^26 and A = D T D, D = diag(2^-k) (an
    exact scaling of the Toeplitz (2, -1) matrix) the mpmath route returns the closed form to 0.1 eps |T|_2"""
    n = 33
    pc, cs = hd.pencil(kind, n, "glued_rot", 0), hd.case(std, n, "glued_rot")
    assert np.array_equal(pc.A, cs.A)
    assert float(np.abs(pc.lam - cs.lam).max()) <= 0.1 * EPS * cs.anorm
    kk = np.arange(n) % 14
    D = np.ldexp(1.0, -kk)
    T = 2 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
    A, B = D[:, None] * T * D[None, :], np.diag(D * D)
    if kind == "hgev":
        ph = np.array([1, 1j, -1, -1j])[kk % 4]                                      # exact unit phases
        A = A.astype(np.complex128) * ph[:, None] * ph.conj()[None, :]
        B = B.astype(np.complex128)
    pi = 4 * np.arctan(LD(1))
    exact = 4 * np.sin(np.arange(1, n + 1).astype(LD) * pi / (2 * (n + 1))) ** 2
    w = hd.reference_eigenvalues(hd.reduced_pencil(A, B))
    assert float(np.abs(w - exact).max()) <= 0.1 * EPS * 4


def test_bounds_file_is_what_lapack_reaches():
    """the committed JSON covers the case table, its worst values are the maxima of its cases, and LAPACK recomputed on two small
    cases per kind is at or under them"""
    import importlib.util
    import os

    spec = importlib.util.spec_from_file_location("make_batch_accuracy_bounds",
                                                  os.path.join(os.path.dirname(hd.BOUNDS_JSON), "make_batch_accuracy_bounds.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    rec = json.load(open(hd.BOUNDS_JSON))
    assert rec["factor"] == hd.BOUND_FACTOR == hb.BOUND_FACTOR
    ids = {hd.case_id(kind, c) for kind in gen.DRIVERS for c in hd.cases(kind)}
    assert set(rec["per_case"]) == ids
    for kind, drivers in gen.DRIVERS.items():
        names = hd.METRICS if kind in ("s", "h") else hd.PENCIL_METRICS
        groups = [None] if kind in ("s", "h") else sorted({c[2] for c in hd.cases(kind)})
        for grp in groups:
            rows = [rec["per_case"][hd.case_id(kind, c)][d] for c in hd.cases(kind) if grp is None or c[2] == grp for d in drivers]
            worst = rec["worst"][kind] if grp is None else rec["worst"][kind][f"c{grp}"]
            assert worst == {k: max(r[q] for r in rows) for q, k in enumerate(names)}, (kind, grp)
            assert hd.bounds(kind, c=grp) == {k: hd.BOUND_FACTOR * v for k, v in worst.items()}
    assert hd.bounds("window") == hd.bounds("s")
    small = {"s": [(33, "glued_rot"), (5, "graded")], "h": [(33, "half_integer"), (32, "rank_one")],
             "gev": [(33, "random", 4), (33, "glued_rot", 4)], "hgev": [(33, "random", 8), (5, "random", 0)]}
    # (cases that stay under 0.6 of the worst of their group here: B goes through LAPACK's QR and differs in its last bits from
    # machine to machine, and with it what LAPACK reaches on a pencil)
    for kind, cases in small.items():
        for case in cases:
            worst = rec["worst"][kind] if len(case) == 2 else rec["worst"][kind][f"c{case[2]}"]
            for drv in gen.DRIVERS[kind]:
                for k, v in zip(worst, gen.lapack_case(kind, case, drv)):
                    assert round(v, 3) <= worst[k], (kind, case, drv, k, v)


BITE_CASES = [c for c in hd.cases("s") if c[0] <= 65]


def test_bounds_bite():
    """the restated algorithm with the kernels' deflation factor (0.5 eps) meets every s bound at n <= 65; with the factor
    raised by 1e3 it still passes the old gates on every case (eigenvalues to 1e-12, residual 768, orthogonality 8) and misses
    a new bound on at least one: the new test sees what the old one cannot"""
    bnd = hd.bounds("s")
    missed = []
    for n, family in BITE_CASES:
        cs = hd.case("s", n, family)
        w, Z = tred2_tql2(cs.A)
        _check_standard("s", f"{family} n={n}", cs, w, Z, label="restated")
        w, Z = tred2_tql2(cs.A, factor=0.5e3)
        assert all(_old_gates(cs.A, w, Z)), (n, family)
        m = hd.metrics(cs, w, Z)
        if any(not v <= bnd[k] for k, v in zip(hd.METRICS, m)):
            missed.append((n, family) + tuple(round(v, 1) for v in m))
    print(f"deflation factor 500 eps: {len(missed)} of {len(BITE_CASES)} cases miss a bound {bnd}:")
    for row in missed:
        print("  ", row)
    assert missed


# ------------------------------------------------------------------------------------------------ GPU
def _std_module(kind):
    import test_batch
    import test_hbatch

    return test_batch if kind == "s" else test_hbatch


def _solve_standard(lib, kind, mats):
    B = _std_module(kind).Batch(mats)
    assert B.run(lib) == 0
    w, Z, info = B.results()
    assert (info == 0).all()
    return w, Z


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", [(k, n) for k in ("s", "h") for n in hd.SIZES[k]])
def test_standard(gpu_lib, kind, n):
    """every family at one size in one call of eigx_s_batch_dev / eigx_h_batch_dev"""
    css = [hd.case(kind, n, f) for f in hd.FAMILIES]
    w, Z = _solve_standard(gpu_lib, kind, [cs.A for cs in css])
    for k, cs in enumerate(css):
        _check_standard(kind, f"{cs.family} n={n}", cs, w[k], Z[k])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", [(k, n) for k in ("gev", "hgev") for n in hd.SIZES[k]])
def test_pencils(gpu_lib, kind, n):
    """every pencil of one size in one call of eigx_gev_batch_dev / eigx_hgev_batch_dev (n = 65 of hgev is above that entry's
    cutoff and goes pencil by pencil through the range solver)"""
    import test_gbatch
    import test_hgbatch

    pcs = [hd.pencil(kind, *c) for c in hd.cases(kind) if c[0] == n]
    P = (test_gbatch if kind == "gev" else test_hgbatch).Pencils([p.A for p in pcs], [p.B for p in pcs])
    assert P.run(gpu_lib) == 0
    w, Z, U, info, _ = P.results()
    assert (info == 0).all()
    for k, pc in enumerate(pcs):
        _check_pencil(kind, f"{pc.family} c={pc.c} n={n}", pc, w[k], Z[k], U[k])


@pytest.mark.gpu
@pytest.mark.parametrize("n", hd.SIZES["window"])
def test_windows(gpu_lib, n):
    """the window kernel (route key 26 = 1): every family under each window of hard_dense.windows(n), one call per window; the
    m columns against the il .. iu slice of the reference, bounds of s"""
    import test_batch_range as tr

    css = [hd.case("window", n, f) for f in hd.FAMILIES]
    redone = 0
    with tr._Key(gpu_lib, 26, 1):
        for il, iu, mode in hd.windows(n):
            B = tr.RBatch([cs.A for cs in css], il, iu)
            assert B.run(gpu_lib, mode=mode.encode(), z=mode == "A") == 0
            route, m, rd = tr._range_info(gpu_lib)
            assert route == 1 and m == iu - il + 1
            redone += rd
            w, Z, info = B.results(want_z=mode == "A")
            assert (info == 0).all()
            for k, cs in enumerate(css):
                _check_standard("window", f"{cs.family} n={n} {il}..{iu} {mode}", cs, w[k], Z[k] if mode == "A" else None, il)
    print(f"BATCH-ACC window n={n}: {redone} matrices redone by route 2")


def _ragged_order(count):
    return np.random.default_rng(7).permutation(count)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["s", "h"])
def test_ragged_standard(gpu_lib, kind):
    """the whole table of one kind, shuffled, in one call of eigx_s_vbatch_dev / eigx_h_vbatch_dev"""
    import test_vbatch as tv

    cases = hd.cases(kind)
    css = [hd.case(kind, *cases[q]) for q in _ragged_order(len(cases))]
    R = tv.Ragged(tv.S if kind == "s" else tv.H, [cs.A for cs in css])
    assert R.run(gpu_lib) == 0
    ws, Zs, info = R.results()
    assert (info == 0).all()
    for k, cs in enumerate(css):
        _check_standard(kind, f"{cs.family} n={cs.n}", cs, ws[k], Zs[k], label=f"{kind}-ragged")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["gev", "hgev"])
def test_ragged_pencils(gpu_lib, kind):
    """the whole table of one kind, shuffled, in one call of eigx_gev_vbatch_dev / eigx_hgev_vbatch_dev"""
    import test_gvbatch as tgv

    cases = hd.cases(kind)
    pcs = [hd.pencil(kind, *cases[q]) for q in _ragged_order(len(cases))]
    fam = tgv.G if kind == "gev" else tgv.HG
    R = tgv.RaggedPencils(fam, [p.A for p in pcs], [p.B for p in pcs])
    assert R.run(gpu_lib) == 0
    ws, Zs, Us, info = R.results(by_range=[k for k, p in enumerate(pcs) if p.n > fam.top])
    assert (info == 0).all()
    for k, pc in enumerate(pcs):
        _check_pencil(kind, f"{pc.family} c={pc.c} n={pc.n}", pc, ws[k], Zs[k], Us[k], label=f"{kind}-ragged")


def _times_pow2(A, k):
    """A 2^k, exactly"""
    return np.ldexp(A.real, k) + 1j * np.ldexp(A.imag, k) if np.iscomplexobj(A) else np.ldexp(A, k)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", [(k, n) for k in ("s", "h") for n in (33, 96)])
def test_power_of_two_copies(gpu_lib, kind, n):
    """A 2^k, k = 400, -400, 700, -700 (outside [1e-90, 1e90]: the kernel scales by the nearest power of two): Z bit for bit the
    same in the four copies and w_k 2^-k == w_400 2^-400 exactly.  And at the unscaled edge, 2^k the largest with max|a| 2^k <=
    1e90 and the smallest with max|a| 2^k >= 1e-90 per matrix: those copies meet the bounds."""
    css = [hd.case(kind, n, f) for f in hd.FAMILIES]
    w0 = Z0 = None
    for k in POW2:
        w, Z = _solve_standard(gpu_lib, kind, [_times_pow2(cs.A, k) for cs in css])
        assert np.isfinite(w).all()
        w = np.ldexp(w, -k)
        if w0 is None:
            w0, Z0 = w, Z
            for q, cs in enumerate(css):
                _check_standard(kind, f"{cs.family} n={n} 2^{k}", cs, w[q], Z[q])
        assert np.array_equal(w, w0), f"2^{k}: w"
        assert np.array_equal(Z, Z0), f"2^{k}: Z"
    for edge in (1e90, 1e-90):
        ks, mats = [], []
        for cs in css:
            mx = float(np.abs(np.r_[cs.A.real.ravel(), cs.A.imag.ravel()]).max())
            if mx == 0.0:
                k = 0
            elif edge > 1:
                k = math.floor(math.log2(edge / mx))
                k -= math.ldexp(mx, k) > edge
            else:
                k = math.ceil(math.log2(edge / mx))
                k += math.ldexp(mx, k) < edge
            beyond = math.ldexp(mx, k + (1 if edge > 1 else -1))
            assert mx == 0.0 or (1e-90 <= math.ldexp(mx, k) <= 1e90 and not 1e-90 <= beyond <= 1e90)
            ks.append(k)
            mats.append(_times_pow2(cs.A, k))
        w, Z = _solve_standard(gpu_lib, kind, mats)
        for q, cs in enumerate(css):
            _check_standard(kind, f"{cs.family} n={n} unscaled 2^{ks[q]}", cs, np.ldexp(w[q], -ks[q]), Z[q])
