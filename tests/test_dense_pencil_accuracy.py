"""The dense generalised solvers held to LAPACK-level accuracy on hard pencils (tests/hard_dense.py): the stages of the Cholesky
route (eigx_chol_dev, eigx_trsm_upper_dev, eigx_gev_reduce_dev and their complex siblings: block inversion, csrc/tri.hip and
csrc/ztri.hip), the range solvers eigx_gev_range_dev / eigx_hgev_range_dev built from them, and the spectral route of the full
drivers eigx_gev_dev / eigx_hgev_dev.  A from hard_dense.PENCIL_A, B = overlap(n, c) of cond 1, 1e1, 1e4, 1e8, real and
complex, upper triangles only (NaN below them and in Im of the complex diagonals), judged entry by entry and column by column
against longdouble / mpmath references, in units of eps = 2^-52.

Bounds: hard_dense.BOUND_FACTOR (16) x what LAPACK reaches on the same cases (tests/golden/dense_pencil_bounds.json, written by
tests/golden/make_dense_pencil_bounds.py): potrf, trtrs, sygst / hegst for the stages, gv / gvd per cond group for the whole
solves.  They come from an independent implementation of the operation, never from the code under test.  A bound of 0 (the
factor of B = I) asks for exactly 0: every comparison is <=.

The gates of tests/test_gev_range.py and tests/test_hgev_range.py (1e-12 n, about 4500 n eps, on B of cond 1.2 .. 1e4) pass a
block inverse that is wrong in its 42nd bit; test_bounds_bite shows on a numpy restatement of the route (64-wide inverses by
substitution, doubling, the three solves, NB as a parameter) that these bounds do not.

Which (n, NB) reaches which branch of tri_inverses_dev / ztri_inverses_dev (BRANCHES) was derived from the loop of that
function, restated in tri_inverses below, not observed on a GPU; test_branch_table holds the table to the restated loop.

Measured on an MI355X: DESIGN section 8h-B and profiles/dense_pencil_accuracy.log."""
import ctypes as C
import contextlib
import json
import os

import numpy as np
import pytest

import hard_band as hb
import hard_dense as hd

EPS, LD = hd.EPS, hd.LD
KINDS = ("gev", "hgev")
NB_KEYS = (64, 128, 192, "default")
NB_DEFAULT = 256
ENTRY = {"gev": {"chol": "eigx_chol_dev", "trsm": "eigx_trsm_upper_dev", "reduce": "eigx_gev_reduce_dev",
                 "range": "eigx_gev_range_dev", "range_v": "eigx_gev_range_v_dev", "full": "eigx_gev_dev", "op": "T"},
         "hgev": {"chol": "eigx_zchol_dev", "trsm": "eigx_ztrsm_upper_dev", "reduce": "eigx_hgev_reduce_dev",
                  "range": "eigx_hgev_range_dev", "range_v": "eigx_hgev_range_v_dev", "full": "eigx_hgev_dev", "op": "C"}}
# the branches of the doubling loop of tri_inverses_dev that a stage call at (n, NB) takes, NB = 256 the default:
#   full   pairs of equal width in the full outer blocks          rem   a right block narrower than the left, full outer block
#   last   pairs of equal width in the last, narrower outer block reml  the same in the last outer block
# At n <= 64, and at NB = 64, the loop forms no pair.  Derived from the loop, not observed.
BRANCHES = {(65, 128): {"reml"},                       # one block of 65: 64 + 1 (reml > w at w = 64), and so at 192 and 256
            (65, 192): {"reml"},
            (65, 256): {"reml"},
            (130, 128): {"full"},                      # blocks 128 + 2: one pair in the full block
            (130, 192): {"last", "reml"},              # one block of 130: 64 + 64, then 128 + 2 (reml > w at w = 128)
            (130, 256): {"last", "reml"},              # the same at the default: reml > w at w = 128
            (200, 128): {"full", "reml"},              # blocks 128 + 72: reml > w at w = 64 (64 + 8)
            (200, 192): {"full", "rem"},               # blocks 192 + 8: rem > w at w = 128 (128 + 64), batch2 = 1
            (200, 256): {"last", "reml"},              # one block of 200: 64 + 64, 64 + 8, then 128 + 72
            (330, 128): {"full", "reml"},              # blocks 128 + 128 + 74: batch2 = 2; 64 + 10 in the last
            (330, 192): {"full", "rem", "last", "reml"},   # blocks 192 + 138: rem > w with the narrow last block (128 + 10)
            (330, 256): {"full", "reml"}}              # blocks 256 + 74: two levels in the full block; 64 + 10 in the last


def _judge(kind, tag, names, values, bnd):
    line = " ".join(f"{k}={v:.3f} (<={bnd[k]:.2f})" for k, v in zip(names, values))
    print(f"GEV-ACC {kind} {tag}: {line}")
    bad = [k for k, v in zip(names, values) if not v <= bnd[k]]
    assert not bad, (kind, tag, bad, values)
    return values


def _misses(names, values, bnd):
    return [k for k, v in zip(names, values) if not v <= bnd[k]]


# ------------------------------------------------------------------------------------------------ the routes, restated
def _inverse_by_substitution(S):
    """the inverse of the upper triangular S, all columns at once, one row per step (inv64_wave)"""
    n = S.shape[0]
    V = np.zeros_like(S)
    for i in range(n - 1, -1, -1):
        e = np.zeros(n, dtype=S.dtype)
        e[i] = 1.0
        V[i] = (e - S[i, i + 1:] @ V[i + 1:]) / S[i, i]
    return V


def tri_inverses(U, NB, defect=None, taken=None):
    """the inverses of the NB-wide diagonal blocks of U as tri_inverses_dev builds them, plain numpy: 64-wide blocks by
    substitution, then widths doubled by V12 = -V11 (U12 V22) -- per outer block the pairs of equal width w and, where the rest
    is wider than w, one pair with a narrower right block.  defect = (K, q, rel): the 64-wide inverse q of outer block K is
    multiplied by 1 + rel.  taken: a set that collects the names of the branches (see BRANCHES)."""
    n = U.shape[0]
    nfull = n // NB
    out = []
    for K in range(-(-n // NB)):
        k0 = K * NB
        W = min(NB, n - k0)
        Ub = U[k0:k0 + W, k0:k0 + W]
        V = np.zeros_like(Ub)
        for q, j0 in enumerate(range(0, W, 64)):
            j1 = min(j0 + 64, W)
            V[j0:j1, j0:j1] = _inverse_by_substitution(Ub[j0:j1, j0:j1])
            if defect is not None and defect[:2] == (K, q):
                V[j0:j1, j0:j1] *= 1.0 + defect[2]

        def join(o, w, wr):
            a, b, c = o, o + w, o + w + wr
            V[a:b, b:c] = -V[a:b, a:b] @ (Ub[a:b, b:c] @ V[b:c, b:c])

        w = 64
        while w < NB:
            npair = W // (2 * w)
            rem = W - npair * 2 * w
            for p in range(npair):
                join(2 * w * p, w, w)
            if rem > w:
                join(npair * 2 * w, w, rem - w)
            if taken is not None:
                taken.update(({"full"} if K < nfull else {"last"}) if npair else set())
                taken.update(({"rem"} if K < nfull else {"reml"}) if rem > w else set())
            w *= 2
        out.append(V)
    return out


def trsm_upper(U, X, V, NB, trans):
    """op(U)^-1 X as trsm_upper_dev forms it: per block row X_k <- op(V_kk) X_k, then the rest minus op(U_k,rest) X_k"""
    X = np.array(X, dtype=np.result_type(U, X))
    n = U.shape[0]
    nblk = len(V)
    for q in range(nblk):
        K = q if trans != "N" else nblk - 1 - q
        k0, k1 = K * NB, min(K * NB + NB, n)
        if trans == "N":
            X[k0:k1] = V[K] @ X[k0:k1]
            X[:k0] -= U[:k0, k0:k1] @ X[k0:k1]
        else:
            X[k0:k1] = V[K].conj().T @ X[k0:k1]
            X[k1:] -= U[k0:k1, k1:].conj().T @ X[k0:k1]
    return X


def reduce_upper(A, U, V, NB):
    """C = U^-H A U^-1 by two block-inversion solves, Hermitian from its upper triangle (gev_reduce_dev)"""
    X = trsm_upper(U, A, V, NB, "C")
    return hd._from_upper(trsm_upper(U, X.conj().T, V, NB, "C"))


def cholesky_route(A, B, NB=NB_DEFAULT, il=1, iu=None, defect=None):
    """the route of eigx_gev_range_dev / eigx_hgev_range_dev in numpy float64: B = U^H U (LAPACK), the block inverses, C =
    U^-H A U^-1, numpy.linalg.eigh of C, Z = U^-1 Y on the columns il .. iu.  Returns w, Z, U, C."""
    import scipy.linalg

    U = np.triu(scipy.linalg.cholesky(B))
    V = tri_inverses(U, NB, defect)
    Cm = reduce_upper(A, U, V, NB)
    w, Y = np.linalg.eigh(Cm)
    sl = slice(il - 1, iu if iu else A.shape[0])
    return w[sl], trsm_upper(U, Y[:, sl], V, NB, "N"), U, Cm


def spectral_route(A, B):
    """the route of eigx_gev_dev / eigx_hgev_dev in numpy float64: B = Z_B W_B Z_B^H, F = Z_B W_B^-1/2, C = F^H A F, eigh of C,
    Z = F Y.  Returns w, Z, F."""
    wb, Zb = np.linalg.eigh(B)
    F = Zb / np.sqrt(wb)
    Cm = F.conj().T @ (A @ F)
    w, Y = np.linalg.eigh((Cm + Cm.conj().T) / 2)
    return w, F @ Y, F


# ------------------------------------------------------------------------------------------------ CPU: the references
def _mp_solve(U, R, trans):
    """op(U)^-1 R by substitution in mpmath at 50 digits, as complex128-rounded pairs (hi, lo) -> clongdouble"""
    import mpmath

    n, k = R.shape
    with mpmath.workdps(50):
        M = [[mpmath.mpc(complex(U[i, j])) for j in range(n)] for i in range(n)]
        if trans != "N":
            M = [[mpmath.conj(M[j][i]) for j in range(n)] for i in range(n)]
        X = np.zeros((n, k), dtype=np.clongdouble)
        for c in range(k):
            x = [None] * n
            for i in (range(n - 1, -1, -1) if trans == "N" else range(n)):
                js = range(i + 1, n) if trans == "N" else range(i)
                x[i] = (mpmath.mpc(complex(R[i, c])) - mpmath.fsum(M[i][j] * x[j] for j in js)) / M[i][i]
                X[i, c] = hd._to_ld(mpmath.re(x[i])) + 1j * hd._to_ld(mpmath.im(x[i]))
    return X


@pytest.mark.parametrize("kind", KINDS)
def test_stage_references(kind):
    """longdouble substitution against mpmath at 50 digits on a factor of cond 1e4 (B of cond 1e8), both ops: column-wise within
    0.01 eps; the reduction's reference is the product form U^H C_ref U = A to 0.01 eps |U|^2 |C_ref|; E_f of LAPACK's own factor
    is below 2; a window of pencil_metrics is the full call on those columns; the scaled copy's metrics are bit for bit those of
    the pencil"""
    n = 24
    st = hd.stage(kind, n, 8)
    for op in "NC":
        X = _mp_solve(st.U, st.R[:, :3], op)
        assert hd.solve_error(X, st.X[op][:, :3].astype(np.clongdouble)) <= 0.01, op
    rd = hd.reduction(kind, n, "glued_rot", 8)
    T = rd.C.dtype
    Ul = st.U.astype(T)
    back = Ul.conj().T @ rd.C @ Ul
    assert float(np.abs(back - rd.A).max()) <= 0.01 * EPS * np.linalg.norm(st.U, 2) ** 2 * float(np.abs(rd.C).max())
    assert hd.reduction_error(rd, np.asarray(rd.C, dtype=st.U.dtype)) <= 1.0   # rounding C_ref to fp64: within 1 eps |C|
    assert 0 < hd.factor_error(st.B, st.U, st.bnorm) < 2
    pc = hd.pencil(kind, 33, "glued_rot", 4)
    w, Z, U, _ = cholesky_route(pc.A, pc.B, 64)
    full = hd.pencil_metrics(pc, w, Z, U)
    win = hd.pencil_metrics(pc, w[9:17], Z[:, 9:17], U, il=10)
    assert all(a <= b for a, b in zip(win, full)) and win[3] == full[3]
    assert hd.pencil_metrics(pc, w, Z, U, il=1) == full
    sp = hd.ScaledPencil(pc, 60, -40)
    assert hd.pencil_metrics(sp, np.ldexp(w, 100), np.ldexp(Z.real, 20) + (1j * np.ldexp(Z.imag, 20) if kind == "hgev" else 0),
                             np.ldexp(U.real, -20) + (1j * np.ldexp(U.imag, -20) if kind == "hgev" else 0)) == full


def test_branch_table():
    """BRANCHES is what the restated loop of tri_inverses_dev takes at every (n, NB) of the stage tests; the four branches are
    all reached, rem (a narrower right block inside a full outer block) only with NB = 192"""
    seen = set()
    for n in hd.STAGE_SIZES:
        for nb in (64, 128, 192, NB_DEFAULT):
            taken = set()
            V = tri_inverses(np.triu(np.ones((n, n))) + n * np.eye(n), nb, taken=taken)
            assert len(V) == -(-n // nb)
            assert taken == BRANCHES.get((n, nb), set()), (n, nb, taken)
            seen |= taken
    assert seen == {"full", "rem", "last", "reml"}
    assert {k[1] for k, v in BRANCHES.items() if "rem" in v} == {192}


def _load_generator():
    import importlib.util

    spec = importlib.util.spec_from_file_location("make_dense_pencil_bounds",
                                                  os.path.join(os.path.dirname(hd.DENSE_BOUNDS_JSON), "make_dense_pencil_bounds.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_bounds_file_is_what_lapack_reaches():
    """the committed JSON covers the case table, its worst values are the maxima of its cases, and LAPACK recomputed on a sample
    (of the stage cases at n = 65 and 130 and the whole solves at n = 65 what the record has at or under 0.6 of its group's
    worst value) is at or under them"""
    gen = _load_generator()
    rec = json.load(open(hd.DENSE_BOUNDS_JSON))
    assert rec["factor"] == hd.BOUND_FACTOR == hb.BOUND_FACTOR
    ids = {gen.stage_id(k, what, c) for k in KINDS for what in hd.STAGES for c in gen.stage_cases(what)}
    ids |= {hd.case_id(k, c) for k in KINDS for c in hd.dense_cases(k)}
    assert set(rec["per_case"]) == ids
    for kind in KINDS:
        for what, names in hd.STAGES.items():
            rows = [m for c in gen.stage_cases(what) for m in rec["per_case"][gen.stage_id(kind, what, c)].values()]
            worst = rec["worst"][kind][what]
            assert worst == {k: max(r[q] for r in rows) for q, k in enumerate(names)}, (kind, what)
            assert hd.stage_bounds(kind, what) == {k: hd.BOUND_FACTOR * v for k, v in worst.items()}
        for grp in hd.PENCIL_C:
            rows = [rec["per_case"][hd.case_id(kind, c)][d] for c in hd.dense_cases(kind) if c[2] == grp for d in gen.DRIVERS]
            worst = rec["worst"][kind]["whole"][f"c{grp}"]
            assert worst == {k: max(r[q] for r in rows) for q, k in enumerate(hd.PENCIL_METRICS)}, (kind, grp)
            assert hd.dense_bounds(kind, grp) == {k: hd.BOUND_FACTOR * v for k, v in worst.items()}
    # B goes through LAPACK's QR and differs in its last bits from machine to machine, and with it what LAPACK reaches: the
    # recomputed sample is held to the group's worst value, not to the case's own, and is taken among the cases that the
    # record has at or under 0.6 of that worst value, so that another BLAS build cannot fail it with nothing wrong
    def roomy(case_id, worst, names):
        return all(v <= 0.6 * worst[k] for m in rec["per_case"][case_id].values() for k, v in zip(names, m))

    for kind in KINDS:
        for what, names in hd.STAGES.items():
            worst = rec["worst"][kind][what]
            sample = [c for c in gen.stage_cases(what) if c[0] in (65, 130) and c[-1] > 0
                      and roomy(gen.stage_id(kind, what, c), worst, names)]
            assert len(sample) >= 4, (kind, what, sample)
            for case in sample:
                for m in gen.lapack_stage(kind, what, case).values():
                    for k, v in zip(names, m):
                        assert round(v, 3) <= worst[k], (kind, what, case, v)
        # whole solves: a cond group has two to four cases, so the margin is asked per metric and driver, not per case
        compared = 0
        for case in [c for c in hd.dense_cases(kind) if c[0] == 65 and c[2] > 0]:
            worst = rec["worst"][kind]["whole"][f"c{case[2]}"]
            held = rec["per_case"][hd.case_id(kind, case)]
            if not any(v <= 0.6 * worst[k] for d in gen.DRIVERS for k, v in zip(worst, held[d])):
                continue
            for drv in gen.DRIVERS:
                for (k, v), old in zip(zip(worst, gen.lapack_whole(kind, case, drv)), held[drv]):
                    if old <= 0.6 * worst[k]:
                        compared += 1
                        assert round(v, 3) <= worst[k], (kind, case, drv, k, v)
        assert compared >= 8, (kind, compared)


# ------------------------------------------------------------------------------------------------ CPU: the bounds bite
BITE_N = (65, 130, 200)
DEFECT = (0, 0, 2.0 ** -42)                      # the first 64-wide inverse of the first outer block, times 1 + 2^-42


def _restated_cases(kind, defect=None):
    """(tag, names, values, bounds) of the restated Cholesky route over the stages at BITE_N x (64, 128, 192, 256) x PENCIL_C and
    the whole solves at n = 65"""
    op = ENTRY[kind]["op"]
    for n in BITE_N:
        for nb in (64, 128, 192, NB_DEFAULT):
            for c in hd.PENCIL_C:
                st = hd.stage(kind, n, c)
                V = tri_inverses(st.U, nb, defect)
                for trans in ("N", "C"):
                    X = trsm_upper(st.U, st.R, V, nb, trans)
                    yield (f"trsm n={n} NB={nb} c={c} op={trans if trans == 'N' else op}", hd.STAGES["trsm"],
                           (hd.solve_error(X, st.X[trans]),), hd.stage_bounds(kind, "trsm"))
                for family in hd.PENCIL_A:
                    rd = hd.reduction(kind, n, family, c)
                    yield (f"reduce n={n} NB={nb} c={c} {family}", hd.STAGES["reduce"],
                           (hd.reduction_error(rd, reduce_upper(rd.A, st.U, V, nb)),), hd.stage_bounds(kind, "reduce"))
    for case in hd.dense_cases(kind):
        if case[0] == 65:
            pc = hd.pencil(kind, *case)
            for nb in (64, NB_DEFAULT):
                w, Z, U, _ = cholesky_route(pc.A, pc.B, nb, defect=defect)
                yield (f"whole n={pc.n} NB={nb} c={pc.c} {pc.family}", hd.PENCIL_METRICS, hd.pencil_metrics(pc, w, Z, U),
                       hd.dense_bounds(kind, pc.c, "cholesky"))


def _old_gates(kind, defect):
    """the gates of tests/test_gev_range.py / tests/test_hgev_range.py on their own pencils (Helmert / random_hpd B at n = 65 and
    130, B of cond 1e4 at n = 130) for the restated route at NB = 64 and 256: solves, reduction, whole solve; True if all hold"""
    import scipy.linalg
    import test_gev_range
    import test_hgev_range

    mod = test_gev_range if kind == "gev" else test_hgev_range
    ok = True
    for n, which in ((65, None), (130, None), (130, "cond1e4")):
        A, B = mod._pencil(n) if which is None else mod._pencil(n, which)
        wref = scipy.linalg.eigh(A, B, eigvals_only=True)
        scale = max(1.0, np.abs(wref).max())
        R = hd._normal(np.random.default_rng(5 + n), (n, n), kind == "hgev")
        for nb in (64, NB_DEFAULT):
            w, Z, U, Cm = cholesky_route(A, B, nb, defect=defect)
            V = tri_inverses(U, nb, defect)
            for trans in ("N", "C"):
                X = trsm_upper(U, R, V, nb, trans)
                err = np.linalg.norm((U if trans == "N" else U.conj().T) @ X - R)
                ok &= bool(err < 1e-12 * n * np.linalg.norm(U) * np.linalg.norm(X))
            ok &= bool(np.linalg.norm(U.conj().T @ Cm @ U - A) < 1e-12 * n * np.linalg.norm(A))
            ok &= bool(np.abs(w - wref).max() < 1e-12 * scale)
            ok &= bool(np.linalg.norm(A @ Z - B @ Z * w) < 1e-12 * scale * n)
            ok &= bool(np.linalg.norm(Z.conj().T @ B @ Z - np.eye(n)) < 1e-12 * n)
    return ok


@pytest.mark.parametrize("kind", KINDS)
def test_bounds_bite(kind):
    """The restated block-inversion route meets every new bound on its table (per kind 96 solves and 96 reductions at n = 65,
    130, 200 under NB = 64, 128, 192, 256, and 16 whole solves at n = 65), without a bound of its own.

    With one 64-wide diagonal-block inverse multiplied by 1 + 2^-42 (DEFECT: a slip in the 42nd bit, 1024 eps) the route still
    passes every gate of tests/test_gev_range.py / tests/test_hgev_range.py on those tests' own pencils (2.3e-13 against gates
    of 1e-12 n), and misses the new bounds on (gev / hgev, measured on the CPU): 96 / 96 of the 96 solves (E_t about 650 ..
    1020: 64 rows of every column are off by 1024 eps, against a bound of 170), 76 / 89 of the 96 reductions (E_c 38 .. 1090
    against 92 / 38; those that stay under are of the random family at c >= 4, where |U^-1|^2 |A| is far above |C_kk|), and
    8 / 8 of the 16 whole solves (every one at c = 0 and c = 1, E_w and E_o about 2050 and 205; at c = 4 and 8 the
    normalisation by eps cond(B) hides a slip of 2^-42, which only the stages see).  2^-42 separates the gates; nothing larger
    was needed.  The counts are printed; every solve, a reduction and half of the whole solves must miss."""
    missed = {"trsm": 0, "reduce": 0, "whole": 0}
    total = dict(missed)
    for tag, names, values, bnd in _restated_cases(kind):
        _judge(f"{kind}-restated", tag, names, values, bnd)
    assert _old_gates(kind, None)
    assert _old_gates(kind, DEFECT), "the planted defect must pass the old gates"
    for tag, names, values, bnd in _restated_cases(kind, DEFECT):
        what = tag.split()[0]
        total[what] += 1
        if _misses(names, values, bnd):
            missed[what] += 1
            print(f"  defect missed: {tag}: " + " ".join(f"{k}={v:.1f}" for k, v in zip(names, values)))
    print(f"{kind}: block inverse x (1 + 2^-42): old gates pass; new bounds missed on {missed} of {total}")
    assert missed["trsm"] == total["trsm"] and missed["reduce"] > 0 and 2 * missed["whole"] >= total["whole"]


@pytest.mark.parametrize("kind", KINDS)
def test_spectral_route_restated(kind):
    """the restated spectral route (F = Z_B W_B^-1/2) meets the bounds in force for eigx_gev_dev / eigx_hgev_dev at n = 65, the
    basis F held to E_o's bound"""
    for case in hd.dense_cases(kind):
        if case[0] == 65:
            pc = hd.pencil(kind, *case)
            w, Z, F = spectral_route(pc.A, pc.B)
            bnd = dict(hd.dense_bounds(kind, pc.c, "spectral"))
            bnd["E_b"] = bnd["E_o"]
            m = hd.pencil_metrics(pc, w, Z, None)[:3] + (hd.basis_error(pc, F),)
            _judge(f"{kind}-spectral-restated", f"n={pc.n} c={pc.c} {pc.family}", ("E_w", "E_r", "E_o", "E_b"), m, bnd)


# ------------------------------------------------------------------------------------------------ GPU
def _dev():
    import torch

    return torch.device("cuda:0")


def _to_dev(M, ld):
    """column-major image of M (rows x cols) with leading dimension ld: tensor (cols, ld), t[j, i] = M(i, j)"""
    import torch

    t = torch.zeros(M.shape[1], ld, dtype=torch.complex128 if np.iscomplexobj(M) else torch.float64, device=_dev())
    t[:, :M.shape[0]] = torch.from_numpy(np.ascontiguousarray(M.T)).to(_dev())
    return t


def _from_dev(t, rows):
    return np.ascontiguousarray(t[:, :rows].T.cpu().numpy())


@contextlib.contextmanager
def _key20(lib, nb):
    """eigx_tune key 20 (outer block width of the triangular stages) at nb, restored on the way out"""
    if nb == "default":
        assert lib.eigx_tune(20, NB_DEFAULT) == NB_DEFAULT, "the default of key 20 is no longer 256: BRANCHES assumes it"
        yield
        return
    old = lib.eigx_tune(20, nb)
    assert old >= 64
    try:
        yield
    finally:
        lib.eigx_tune(20, old)


def _ld(n):
    return n + 2 + (n & 1)          # even: eigx_gev_dev and eigx_gev_range_dev ask for it


STAGE_PARAMS = [(k, n, nb) for k in KINDS for n in hd.STAGE_SIZES for nb in NB_KEYS]


def _tag(n, nb, c):
    taken = BRANCHES.get((n, NB_DEFAULT if nb == "default" else nb), set())
    return f"n={n} NB={nb} c={c} [{'+'.join(sorted(taken)) or 'no pair'}]"


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,nb", STAGE_PARAMS)
def test_cholesky_stage(gpu_lib, kind, n, nb):
    """eigx_chol_dev / eigx_zchol_dev on overlap(n, c): E_f under 16 x potrf's; the diagonal real and > 0 (Im written as 0), the
    upper triangle finite"""
    ld = n + 2
    with _key20(gpu_lib, nb):
        for c in hd.PENCIL_C:
            st = hd.stage(kind, n, c)
            b = _to_dev(hd.nan_lower(st.B), ld)
            assert getattr(gpu_lib, ENTRY[kind]["chol"])(n, b.data_ptr(), ld) == 0
            out = _from_dev(b, n)
            assert np.isfinite(out[np.triu_indices(n)]).all()
            assert (out.real.diagonal() > 0).all()
            if kind == "hgev":
                assert (out.imag.diagonal() == 0.0).all()
            U = hd.upper_of(out)
            _judge(f"{kind}-chol", _tag(n, nb, c), hd.STAGES["chol"], (hd.factor_error(st.B, U, st.bnorm),),
                   hd.stage_bounds(kind, "chol"))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,nb", STAGE_PARAMS)
def test_triangular_solve_stage(gpu_lib, kind, n, nb):
    """eigx_trsm_upper_dev / eigx_ztrsm_upper_dev with LAPACK's factor of overlap(n, c), both ops, nrhs = 1, 7, n: the column-
    wise forward error E_t against substitution in longdouble under 16 x trtrs's.  The residual is printed only: for op = U^H
    substitution's is ten times smaller than a correct block inversion's."""
    ld = n + 2
    fn = getattr(gpu_lib, ENTRY[kind]["trsm"])
    with _key20(gpu_lib, nb):
        for c in hd.PENCIL_C:
            st = hd.stage(kind, n, c)
            u = _to_dev(hd.nan_lower(st.U, diag=False), ld)
            for nrhs in sorted({1, 7, n}):
                for trans in ("N", ENTRY[kind]["op"]):
                    key = "N" if trans == "N" else "C"
                    x = _to_dev(st.R[:, :nrhs], ld)
                    assert x.shape == (nrhs, ld)      # the stage holds max(n, 7) right-hand sides: nrhs columns are there
                    assert fn(trans.encode(), n, nrhs, u.data_ptr(), ld, x.data_ptr(), ld) == 0
                    X = _from_dev(x, n)
                    assert np.isfinite(X).all()
                    res = hd.solve_residual(st.U, X, st.R[:, :nrhs], key)
                    _judge(f"{kind}-trsm", f"{_tag(n, nb, c)} nrhs={nrhs} op={trans} (residual {res:.2f})", hd.STAGES["trsm"],
                           (hd.solve_error(X, st.X[key][:, :nrhs]),), hd.stage_bounds(kind, "trsm"))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,nb", STAGE_PARAMS)
def test_reduction_stage(gpu_lib, kind, n, nb):
    """eigx_gev_reduce_dev / eigx_hgev_reduce_dev with LAPACK's factor: the upper triangle of C against two longdouble
    substitutions with the same U, E_c under 16 x sygst's / hegst's; the complex entry leaves the strict lower triangle of a bit
    for bit as it was passed"""
    ld = n + 2
    fn = getattr(gpu_lib, ENTRY[kind]["reduce"])
    low = np.tril_indices(n, -1)
    with _key20(gpu_lib, nb):
        for c in hd.PENCIL_C:
            u = _to_dev(hd.nan_lower(hd.stage(kind, n, c).U), ld)
            for family in hd.PENCIL_A:
                rd = hd.reduction(kind, n, family, c)
                a = _to_dev(hd.nan_lower(rd.A), ld)
                before = _from_dev(a, n)
                assert fn(n, a.data_ptr(), ld, u.data_ptr(), ld) == 0
                out = _from_dev(a, n)
                assert np.isfinite(out.real[np.triu_indices(n)]).all() and np.isfinite(out.imag[np.triu_indices(n, 1)]).all()
                if kind == "hgev":
                    assert np.array_equal(out[low].view(np.uint64), before[low].view(np.uint64)), "the strict lower triangle of a"
                _judge(f"{kind}-reduce", f"{_tag(n, nb, c)} {family}", hd.STAGES["reduce"],
                       (hd.reduction_error(rd, np.triu(np.nan_to_num(out, nan=0.0))),), hd.stage_bounds(kind, "reduce"))


def _range(lib, kind, pc, il, iu):
    """eigx_gev_range_dev / eigx_hgev_range_dev in mode 'A' on the poisoned upper triangles: w, Z and the U left in b"""
    import torch

    n, m, ld = pc.n, iu - il + 1, _ld(pc.n)
    a, b = _to_dev(hd.nan_lower(pc.A), ld), _to_dev(hd.nan_lower(pc.B), ld)
    z = torch.zeros(m, ld, dtype=a.dtype, device=_dev())
    w = torch.zeros(m, dtype=torch.float64, device=_dev())
    rc = getattr(lib, ENTRY[kind]["range"])(n, il, iu, a.data_ptr(), ld, b.data_ptr(), ld, w.data_ptr(), z.data_ptr(), ld, b"A")
    assert rc == 0
    return w.cpu().numpy(), _from_dev(z, n), _from_dev(b, n)


def _check_range(kind, tag, pc, w, Z, bout, il):
    assert np.isfinite(w).all() and np.isfinite(Z).all() and np.isfinite(bout[np.triu_indices(pc.n)]).all(), tag
    assert (np.diff(w) >= 0).all(), f"{tag}: w is not ascending"
    if kind == "hgev":
        assert (bout.imag.diagonal() == 0.0).all()
    return _judge(f"{kind}-range", tag, hd.PENCIL_METRICS, hd.pencil_metrics(pc, w, Z, hd.upper_of(bout), il),
                  hd.dense_bounds(kind, pc.c, "cholesky"))


WHOLE_PARAMS = [(k,) + c for k in KINDS for c in hd.dense_cases(k)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,family,c", WHOLE_PARAMS)
def test_range_solvers(gpu_lib, kind, n, family, c):
    """eigx_gev_range_dev / eigx_hgev_range_dev, mode 'A', key 20 at 64 and at its default, windows (1, n), (1, 8), (n - 7, n)
    and 8 in the middle: the window's columns under the bounds of the cond group, the returned b a factor that passes E_f"""
    pc = hd.pencil(kind, n, family, c)
    for nb in (64, "default"):
        with _key20(gpu_lib, nb):
            for il, iu in hd.windows_dense(n):
                w, Z, bout = _range(gpu_lib, kind, pc, il, iu)
                _check_range(kind, f"n={n} NB={nb} c={c} {family} {il}..{iu}", pc, w, Z, bout, il)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_range_by_value(gpu_lib, kind):
    """the by-value entries on (n = 65, glued_rot, c = 4): vl and vu half-way between reference eigenvalues around 8 in the
    middle, the gaps there wide enough (1e-6 of the spectrum's width) for m = 8 to be known"""
    import torch

    pc = hd.pencil(kind, 65, "glued_rot", 4)
    n, ld = pc.n, _ld(pc.n)
    lam = pc.lam
    gap = np.diff(lam)
    width = float(lam[-1] - lam[0])
    il = min((q for q in range(2, n - 8) if gap[q - 2] > 1e-6 * width and gap[q + 6] > 1e-6 * width), key=lambda q: abs(q - n // 2))
    vl, vu = float((lam[il - 2] + lam[il - 1]) / 2), float((lam[il + 6] + lam[il + 7]) / 2)
    a, b = _to_dev(hd.nan_lower(pc.A), ld), _to_dev(hd.nan_lower(pc.B), ld)
    z = torch.zeros(8, ld, dtype=a.dtype, device=_dev())
    w = torch.zeros(8, dtype=torch.float64, device=_dev())
    m, first = C.c_int(-1), C.c_int(-1)
    rc = getattr(gpu_lib, ENTRY[kind]["range_v"])(n, vl, vu, 8, C.byref(m), C.byref(first), a.data_ptr(), ld, b.data_ptr(), ld,
                                                  w.data_ptr(), z.data_ptr(), ld, b"A")
    assert rc == 0 and (m.value, first.value) == (8, il)
    _check_range(kind, f"n={n} c=4 glued_rot [{vl:.6g}, {vu:.6g}) -> {il}..{il + 7}", pc, w.cpu().numpy(), _from_dev(z, n),
                 _from_dev(b, n), il)


def _full(lib, kind, pc):
    """eigx_gev_dev / eigx_hgev_dev on the poisoned upper triangles: w, Z, the F left in b and the Y left in a"""
    import torch

    n, ld = pc.n, _ld(pc.n)
    a, b = _to_dev(hd.nan_lower(pc.A), ld), _to_dev(hd.nan_lower(pc.B), ld)
    z = torch.zeros(n, ld, dtype=a.dtype, device=_dev())
    w = torch.zeros(n, dtype=torch.float64, device=_dev())
    assert getattr(lib, ENTRY[kind]["full"])(n, a.data_ptr(), ld, b.data_ptr(), ld, w.data_ptr(), z.data_ptr(), ld) == 0
    return w.cpu().numpy(), _from_dev(z, n), _from_dev(b, n), _from_dev(a, n)


def _check_full(kind, tag, pc, w, Z, F, Y):
    """the three pencil metrics under the bounds of the cond group, and the returned basis F (F^H B F = I, normalised as E_o is)
    under E_o's: F is a B-orthonormal basis as Z is, and LAPACK's Z is the independent measure of what one can reach.  The
    on-exit contract: b holds F = Z_B W_B^-1/2 with W_B ascending (column norms w_B^-1/2 do not grow, to 1e-10 where they are
    equal) and a the Y with Z = F Y (entry-wise within the bound of an fp64 product, n eps |F| |Y|)."""
    assert np.isfinite(w).all() and np.isfinite(Z).all() and np.isfinite(F).all() and np.isfinite(Y).all(), tag
    assert (np.diff(w) >= 0).all(), f"{tag}: w is not ascending"
    fn = np.linalg.norm(F, axis=0)
    assert (fn[1:] <= fn[:-1] * (1 + 1e-10)).all(), f"{tag}: the columns of F are not in ascending order of w_B"
    T = np.clongdouble if kind == "hgev" else LD
    assert (np.abs(F.astype(T) @ Y.astype(T) - Z) <= pc.n * EPS * (np.abs(F) @ np.abs(Y))).all(), f"{tag}: Z is not F Y"
    bnd = dict(hd.dense_bounds(kind, pc.c, "spectral"))
    bnd["E_b"] = bnd["E_o"]
    m = hd.pencil_metrics(pc, w, Z, None)[:3] + (hd.basis_error(pc, F),)
    return _judge(f"{kind}-full", tag, ("E_w", "E_r", "E_o", "E_b"), m, bnd)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,family,c", WHOLE_PARAMS)
def test_full_drivers(gpu_lib, kind, n, family, c):
    """eigx_gev_dev / eigx_hgev_dev (the spectral route F = Z_B W_B^-1/2) on the same pencils.  (gev, 130, glued_rot, 4) is the
    case that measured E_w = 1.913 against 1.78 while F's columns stood in ascending order of w_B between the two solves;
    0.198 since they stand in descending order."""
    pc = hd.pencil(kind, n, family, c)
    _check_full(kind, f"n={n} c={c} {family}", pc, *_full(gpu_lib, kind, pc))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_scaled_copy(gpu_lib, kind):
    """(n = 65, glued_rot, c = 4) with A 2^60 and B 2^-40: the reference scales exactly and the metrics are scale-invariant, so
    the range solver (which does not scale B) and the full driver meet the same bounds"""
    pc = hd.ScaledPencil(hd.pencil(kind, 65, "glued_rot", 4), 60, -40)
    for il, iu in hd.windows_dense(pc.n)[:2]:
        w, Z, bout = _range(gpu_lib, kind, pc, il, iu)
        _check_range(kind, f"n={pc.n} c=4 glued_rot A 2^60, B 2^-40 {il}..{iu}", pc, w, Z, bout, il)
    _check_full(kind, f"n={pc.n} c=4 glued_rot A 2^60, B 2^-40", pc, *_full(gpu_lib, kind, pc))
