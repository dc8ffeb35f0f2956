"""The dense standard drivers eigx_sx / eigx_s / eigx_h and their stages eigx_band_reduce_dev / eigx_trbak_dev held to
LAPACK-level accuracy on the hard matrix table of tests/hard_dense.py: graded both ways, glued Wilkinson plain and rotated,
multiplicities, identity plus 1e-15, rank one, Clement, blocks of scale 1 and 1e-8 (zero columns in the reduction), Frank,
diagonal, identity, zero; real and Hermitian; upper triangles only (NaN below them and in Im of the complex diagonal); judged
entry by entry and column by column against longdouble references, in units of eps = 2^-52.

  reduce   E_s = max |Q^H A Q - T| / (eps |A|_2), E_q = max |Q^H Q - I| / eps with Q the back-transformed identity and T the
           returned (d, e); for band 1 the eigenvalues of (d, e) in longdouble against those of A (E_w)
  trbak    E_b = max_j |z_j - zref_j|_2 / (eps |zref_j|_2) against the same reflectors applied one by one in longdouble
  whole    E_w, E_r, E_o of hard_dense.metrics

Bounds: hard_dense.BOUND_FACTOR (16) x what LAPACK reaches on the same table (tests/golden/dense_driver_bounds.json, written by
tests/golden/make_dense_driver_bounds.py): sytrd / hetrd with Q formed, ormqr / unmqr, syevd / heevd.  They come from an
independent implementation of the operation, never from the code under test, and do not depend on n.  The pentadiagonal
reduction (band 2) has no LAPACK counterpart and borrows the tridiagonal record.  The CPU oracle restates the algorithm
(un-normalised reflectors, bottom-up order) and is held to the same bounds at n <= 130 without a GPU.

The gates of tests/test_gpu_parity.py are normwise (|A Z - Z W|_F / (n eps |A|_F) < 768, |Z^T Z - I|_F / (n eps) < 8);
test_bounds_bite shows an eigenvector pair rotated by 2^-40 that passes them and misses these bounds.

Out of scope here: modes 'N' / 'X' / 'S' / 'C' of the real drivers (the Sturm, subset and range paths), several ranks, host
entry points, and the documented overflow of eigx_h between 1e77 and 1e90 (test_scaling_extremes).

Measured on an MI355X: DESIGN section 8h-C and profiles/dense_driver_accuracy.log."""
import ctypes as C
import contextlib
import importlib.util
import json
import os

import numpy as np
import pytest

import hard_band as hb
import hard_dense as hd

EPS, LD = hd.EPS, hd.LD
KINDS = ("s", "h")
ENTRY = {"sx": "eigx_sx_dev", "s": "eigx_s_dev", "h": "eigx_h_dev"}
KIND_OF = {"sx": "s", "s": "s", "h": "h"}
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "known_answers.json")))
GATE_RES, GATE_ORTH = GOLD["gates"]["residual"], GOLD["gates"]["orthogonality"]


def _judge(tag, names, values, bnd):
    print(f"DENSE-DRIVER {tag}: " + " ".join(f"{k}={v:.3f} (<={bnd[k]:.1f})" for k, v in zip(names, values)))
    bad = [k for k, v in zip(names, values) if not v <= bnd[k]]
    assert not bad, (tag, bad, values)
    return values


def _band_eigenvalue_error(cs, d, e):
    """E_w of the tridiagonal (d, e) a reduction returned: its eigenvalues in longdouble against those of A"""
    lam = hb.reference_eigenvalues(np.asarray(d), np.asarray(e).reshape(1, -1), 1)
    return float(np.abs(lam - cs.lam).max()) / (EPS * (cs.anorm if cs.anorm > 0 else 1.0))


def _check_reduction(tag, cs, band, d, e, Q, family=None):
    """E_s, E_q of (d, e, Q), and for band 1 the E_w of (d, e), under the bounds of the reduction"""
    assert np.isfinite(d).all() and np.isfinite(e).all() and np.isfinite(Q).all(), tag
    bnd = dict(hd.driver_stage_bounds("s", "reduce", family or cs.family))
    names = ("E_s", "E_q")
    vals = hd.similarity_metrics(cs.A, Q, hb.band_matrix(d, e, band), cs.anorm)
    if band == 1:
        bnd["E_w"] = hd.driver_bounds("s", family or cs.family)["E_w"]
        names, vals = names + ("E_w",), vals + (_band_eigenvalue_error(cs, d, e),)
    return _judge(tag, names, vals, bnd)


def _check_whole(tag, cs, w, Z, nvec=None):
    """all of w and the nvec columns of Z under the bounds of the whole solves; the zero matrix: w exactly 0"""
    kind = "h" if np.iscomplexobj(cs.A) else "s"
    assert np.isfinite(w).all() and np.isfinite(Z).all(), tag
    assert (np.diff(w) >= 0).all(), f"{tag}: w is not ascending"
    if cs.family == "zero":
        assert (w == 0.0).all(), f"{tag}: w of the zero matrix"
    bnd = hd.driver_bounds(kind, cs.family)
    E_w = hd.metrics(cs, w, None)[0]
    m = Z.shape[1] if nvec is None else nvec
    _, E_r, E_o = hd.metrics(cs, w[:m], Z[:, :m])
    return _judge(tag, hd.METRICS, (E_w, E_r, E_o), bnd)


# ------------------------------------------------------------------------------------------------ CPU: the record
def _load_generator():
    spec = importlib.util.spec_from_file_location("make_dense_driver_bounds",
                                                  os.path.join(os.path.dirname(hd.DRIVER_BOUNDS_JSON), "make_dense_driver_bounds.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_case_table():
    """the table of the issue: six real rows and five Hermitian ones, all 14 families but at n = 517"""
    assert [c[:4] for c in hd.DRIVER_TABLE] == [(5, 4, 8, 0), (65, 16, 16, 0), (130, 48, 48, 0), (330, 128, 128, 0),
                                                (330, 32, 128, 2), (517, 64, 128, 4)]
    assert [c[:2] for c in hd.DRIVER_H_TABLE] == [(5, 4), (17, 4), (65, 16), (130, 48), (200, 48)]
    assert len(hd.driver_cases("s")) == 5 * 14 + 4 and len(hd.driver_cases("h")) == 5 * 14
    assert {c[4] for c in hd.driver_cases("s") if c[0] == 517} == {"random", "graded", "glued_rot", "blocks"}
    assert len(hd.driver_problems("s")) == 4 * 14 + 4 and len(hd.driver_problems("h")) == 5 * 14


def test_bounds_file_is_what_lapack_reaches():
    """the committed JSON covers the case table, its worst values are the maxima of its cases, the loaders return BOUND_FACTOR
    x them, and LAPACK recomputed on two small cases (matrices that do not go through a QR, so that they are the same on
    every machine) is at or under the worst values"""
    gen = _load_generator()
    rec = json.load(open(hd.DRIVER_BOUNDS_JSON))
    assert rec["factor"] == hd.BOUND_FACTOR == hb.BOUND_FACTOR
    assert set(rec["per_case"]) == {gen.problem_id(k, n, f) for k in KINDS for n, f in hd.driver_problems(k)}
    assert rec["worst"] == gen.worst_of(rec["per_case"])
    for kind in KINDS:
        for what, names in hd.DRIVER_STAGES.items():
            assert set(rec["worst"][kind][what]) == set(names)
            assert hd.driver_stage_bounds(kind, what) == {k: hd.BOUND_FACTOR * v for k, v in rec["worst"][kind][what].items()}
        assert hd.driver_bounds(kind) == hd.driver_stage_bounds(kind, "whole")
    own = rec.get("family_bounds", {})
    assert len(own) <= 2 and not any(k.endswith("-random") for k in own)
    for key, entry in own.items():
        assert entry["reason"] and entry["measured"], key
    for kind, n, family in (("s", 65, "graded"), ("h", 17, "clement")):
        for what, m in gen.lapack_problem(kind, n, family).items():
            for k, v in zip(hd.DRIVER_STAGES[what] * len(m), m):
                assert gen._sig(v) <= rec["worst"][kind][what][k], (kind, n, family, what, k, v)


def test_helpers():
    """similarity_metrics is (0, 0) for an exact similarity and sees one wrong entry at its size; the Hermitian form (T = None)
    sees an entry outside the band and an imaginary part inside it; a scaled copy's metrics are those of the case; the
    reference of the zero matrix is 0"""
    n = 12
    P = np.eye(n)[:, ::-1]
    cs = hd.case("s", n, "frank")
    T = P.T @ cs.A @ P
    assert hd.similarity_metrics(cs.A, P, T, cs.anorm) == (0.0, 0.0)
    T2 = T.copy()
    T2[3, 7] += 64 * EPS * cs.anorm
    assert abs(hd.similarity_metrics(cs.A, P, T2, cs.anorm)[0] - 64) < 0.5     # (the addition itself rounds)
    H = np.diag(np.arange(1.0, n + 1)).astype(np.complex128)
    H[0, 1], H[1, 0] = 1 + 0.25j, 1 - 0.25j
    H[0, 5] = H[5, 0] = 0.5
    assert hd.similarity_metrics(H, np.eye(n), None, 1.0)[0] == 0.5 / EPS
    H[0, 5] = H[5, 0] = 0.0
    assert hd.similarity_metrics(H, np.eye(n), None, 1.0)[0] == 0.25 / EPS
    assert hd.similarity_metrics(H, np.eye(n) * (1 + 8 * EPS), None, 1.0)[1] > 15
    cs = hd.case("s", 33, "glued_rot")
    w, Z = np.linalg.eigh(cs.A)
    for k in (600, -600):
        sc = hd.ScaledDense(cs, k)
        assert hd.metrics(sc, np.ldexp(w, k), Z) == pytest.approx(hd.metrics(cs, w, Z), rel=1e-9)   # (|A|_2 of E_r: LAPACK's)
        assert hd.similarity_metrics(sc.A, Z, np.diag(np.ldexp(w, k)), sc.anorm) == hd.similarity_metrics(cs.A, Z, np.diag(w),
                                                                                                        cs.anorm)
    for kind in KINDS:
        assert not hd.reference_eigenvalues(hd.matrix("zero", 9, cplx=kind == "h")).any()
    for which in hd.BACK_INPUTS:
        assert hd.back_input(7, which).shape == (7, 7) and np.iscomplexobj(hd.back_input(7, which, True))


# ------------------------------------------------------------------------------------------------ CPU: the oracle
def _orc_trbak(orc, refl, e, band, Z):
    p = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    n = refl.shape[0]
    out = np.asfortranarray(Z, dtype=np.float64).copy(order="F")
    ee = np.ascontiguousarray(e, dtype=np.float64)
    rf = np.asfortranarray(refl)
    assert orc.load().orc_trbak(n, out.shape[1], p(rf), n, p(out), n, p(ee), ee.shape[1], band) == 0
    return out


ORACLE_S = hd.driver_cases("s", max_n=130)
ORACLE_H = hd.driver_cases("h", max_n=130)


@pytest.mark.parametrize("band", [1, 2])
@pytest.mark.parametrize("case", ORACLE_S, ids=[hd.driver_case_id("s", c) for c in ORACLE_S])
def test_oracle_stage_pair(orc, case, band):
    """orc.band_reduce, then orc_trbak on the identity and on the three Z: the bounds are reachable by this algorithm
    (un-normalised reflectors, bottom-up order) and not only by LAPACK's"""
    n, _, _, _, family = case
    cs = hd.case("s", n, family)
    d, e, refl = orc.band_reduce(cs.A, band)
    Q = _orc_trbak(orc, refl, e, band, np.eye(n))
    _check_reduction(f"oracle reduce band={band} n={n} {family}", cs, band, d, e, Q)
    bnd = hd.driver_stage_bounds("s", "trbak", family)
    for which in hd.BACK_INPUTS:
        Z0 = hd.back_input(n, which)
        E_b = hd.solve_error(_orc_trbak(orc, refl, e, band, Z0), hd.apply_reflectors_ld(refl, e, band, Z0))
        _judge(f"oracle trbak band={band} n={n} {family} Z={which}", ("E_b",), (E_b,), bnd)


@pytest.mark.parametrize("route", ["sx", "s"])
@pytest.mark.parametrize("case", ORACLE_S, ids=[hd.driver_case_id("s", c) for c in ORACLE_S])
def test_oracle_whole(orc, case, route):
    n, _, _, _, family = case
    cs = hd.case("s", n, family)
    w, Z, _, _ = orc.eigen(cs.A, route)
    _check_whole(f"oracle {route} n={n} {family}", cs, w, Z)


@pytest.mark.parametrize("case", ORACLE_H, ids=[hd.driver_case_id("h", c) for c in ORACLE_H])
def test_oracle_whole_hermitian(orc, case):
    n, _, _, _, family = case
    cs = hd.case("h", n, family)
    w, Z = orc.eigen_h(cs.A)
    _check_whole(f"oracle h n={n} {family}", cs, w, Z)
    _, Q = orc.eigen_h(cs.A, mode="S")
    _judge(f"oracle h mode S n={n} {family}", ("E_s", "E_q"), hd.similarity_metrics(cs.A, Q, None, cs.anorm),
           hd.driver_stage_bounds("h", "reduce", family))


# ------------------------------------------------------------------------------------------------ CPU: the bounds bite
def test_bounds_bite():
    """numpy.linalg.eigh's result on glued_rot at n = 130 with the eigenvectors of the lowest and the highest eigenvalue rotated
    into each other by 2^-40 (a rotation: Z stays orthogonal): the gates of tests/test_gpu_parity.py still pass (the residual
    gate reads about 6 of 768), and E_r misses its bound by a factor of 20 (about 4500 against 16 x LAPACK's worst)"""
    from eigenexa_amd import layout

    cs = hd.case("s", 130, "glued_rot")
    w, Z = np.linalg.eigh(cs.A)
    bnd = hd.driver_bounds("s", cs.family)
    clean = hd.metrics(cs, w, Z)
    assert all(v <= bnd[k] for k, v in zip(hd.METRICS, clean)), clean
    s = 2.0 ** -40
    c = np.sqrt(1.0 - s * s)
    Zr = Z.copy()
    Zr[:, 0], Zr[:, -1] = c * Z[:, 0] + s * Z[:, -1], c * Z[:, -1] - s * Z[:, 0]
    res, orth = layout.accuracy_metrics(cs.A, w, Zr)
    E_w, E_r, E_o = hd.metrics(cs, w, Zr)
    print(f"DENSE-DRIVER bite: old gates residual {res:.2f} (<{GATE_RES}) orthogonality {orth:.3f} (<{GATE_ORTH}); "
          f"E_r={E_r:.1f} (<={bnd['E_r']:.1f}) E_o={E_o:.1f} (<={bnd['E_o']:.1f}), clean E_r={clean[1]:.2f}")
    assert res < GATE_RES and orth < GATE_ORTH
    assert E_r > bnd["E_r"] or E_o > bnd["E_o"]


# ------------------------------------------------------------------------------------------------ GPU
def _dev():
    import torch

    return torch.device("cuda:0")


def _ld(n):
    return n + 2 + (n & 1)          # even, and not n


def _to_dev(M, ld):
    """column-major image of M (rows x cols) with leading dimension ld: tensor (cols, ld), t[j, i] = M(i, j)"""
    import torch

    t = torch.zeros(M.shape[1], ld, dtype=torch.complex128 if np.iscomplexobj(M) else torch.float64, device=_dev())
    t[:, :M.shape[0]] = torch.from_numpy(np.ascontiguousarray(M.T)).to(_dev())
    return t


def _from_dev(t, rows):
    return np.ascontiguousarray(t[:, :rows].T.cpu().numpy())


@contextlib.contextmanager
def _tuned(lib, settings):
    """eigx_tune keys at the given values, every one restored on the way out"""
    old = []
    try:
        for key, v in settings:
            prev = lib.eigx_tune(key, v)
            assert prev >= 0, (key, v)
            old.append((key, prev))
        yield
    finally:
        for key, prev in reversed(old):
            lib.eigx_tune(key, prev)


def _gpu_reduce(lib, A, m, band):
    """eigx_band_reduce_dev on the poisoned upper triangle: d, e[band, n], the device matrix with the reflectors, its ld"""
    import torch

    n, ld = A.shape[0], _ld(A.shape[0])
    a = _to_dev(hd.nan_lower(A), ld)
    d = torch.zeros(n, dtype=torch.float64, device=_dev())
    e = torch.zeros(2 * n, dtype=torch.float64, device=_dev())
    assert lib.eigx_band_reduce_dev(n, a.data_ptr(), ld, d.data_ptr(), e.data_ptr(), n, m, band) == 0
    return d.cpu().numpy(), e.cpu().numpy().reshape(2, n)[:band].copy(), a, e


def _gpu_trbak(lib, a, e_dev, n, band, mb, Z0):
    """eigx_trbak_dev on a copy of the reflectors: Z_out (n x nvec)"""
    nvec, ld = Z0.shape[1], a.shape[1]
    z = _to_dev(Z0, ld)
    refl = a.clone()                 # (the entry zeroes below the reflectors: every call starts from what the reduction left)
    assert lib.eigx_trbak_dev(n, nvec, refl.data_ptr(), ld, z.data_ptr(), ld, e_dev.data_ptr(), n, mb, band) == 0
    return _from_dev(z, n)


def _stage_pair(lib, cs, m, mb, band, tag, family=None):
    d, e, a, e_dev = _gpu_reduce(lib, cs.A, m, band)
    Q = _gpu_trbak(lib, a, e_dev, cs.n, band, mb, np.eye(cs.n))
    return _check_reduction(tag, cs, band, d, e, Q, family)


STAGE_CASES = hd.driver_cases("s")
STAGE_IDS = [hd.driver_case_id("s", c) for c in STAGE_CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("band", [1, 2])
@pytest.mark.parametrize("case", STAGE_CASES, ids=STAGE_IDS)
def test_stage_pair(gpu_lib, case, band):
    """eigx_band_reduce_dev, then eigx_trbak_dev on the identity: Q^T A Q is the returned band matrix entry by entry, Q is
    orthogonal entry by entry, and (band 1) the eigenvalues of (d, e) are those of A"""
    n, m, mb, q, family = case
    cs = hd.case("s", n, family)
    with _tuned(gpu_lib, [(2, q)]):
        _stage_pair(gpu_lib, cs, m, mb, band, f"reduce band={band} n={n} m={m} mb={mb} q={q} {family}")


# eigx_tune keys of the reduction, each setting alone.  Key 7 = 1: ka_grid_one_gpu gives G = ceil(ng / key7) > 1 row groups
# per workgroup as soon as ng = ceil(rows / 16) > 2 key7, so 1 is the smallest value and puts every step above 32 rows on
# the several-groups form (at n = 330: up to 21 groups in one workgroup)
KNOB_N, KNOB_M = 330, 48
KNOB_FAMILIES = ("graded", "glued_rot", "blocks", "identity_plus")
KNOBS = {"tiles-100-220-150": [(3, 100), (4, 220), (5, 150)],      # 128, 256 and 512 tiles and the non-temporal loads
         "key11=0": [(11, 0)], "key7=1": [(7, 1)], "key10=0": [(10, 0)], "key12=0": [(12, 0)], "key12=1": [(12, 1)],
         "key25=0": [(25, 0)]}


@pytest.mark.gpu
@pytest.mark.parametrize("band", [1, 2])
@pytest.mark.parametrize("family", KNOB_FAMILIES)
@pytest.mark.parametrize("knob", list(KNOBS))
def test_reduction_knobs(gpu_lib, knob, family, band):
    """every load form, tile size and launch shape of the reduction that a knob selects meets the bounds of the stage pair"""
    cs = hd.case("s", KNOB_N, family)
    with _tuned(gpu_lib, KNOBS[knob]):
        _stage_pair(gpu_lib, cs, KNOB_M, 128, band, f"reduce band={band} n={KNOB_N} m={KNOB_M} {knob} {family}")


BACK_CASES = [c for c in STAGE_CASES if c[4] in hd.BACK_FAMILIES]


@pytest.mark.gpu
@pytest.mark.parametrize("band", [1, 2])
@pytest.mark.parametrize("case", BACK_CASES, ids=[hd.driver_case_id("s", c) for c in BACK_CASES])
def test_back_transformation(gpu_lib, case, band):
    """eigx_trbak_dev alone on the reflectors of the GPU reduction (norms over 14 decades, trivial reflectors, whole trivial
    blocks), Z the identity, normal and normal with graded columns, nvec = n, n // 3, 1: column by column against the same
    reflectors applied one by one in longdouble"""
    n, m, mb, q, family = case
    cs = hd.case("s", n, family)
    d, e, a, e_dev = _gpu_reduce(gpu_lib, cs.A, m, band)
    refl = _from_dev(a, n)
    assert np.isfinite(refl[np.triu_indices(n)]).all() and np.isfinite(e).all()
    bnd = hd.driver_stage_bounds("s", "trbak", family)
    with _tuned(gpu_lib, [(2, q)]):
        for which in hd.BACK_INPUTS:
            Z0 = hd.back_input(n, which)
            Zref = hd.apply_reflectors_ld(np.triu(np.nan_to_num(refl, nan=0.0)), e, band, Z0)
            for nvec in sorted({n, max(n // 3, 1), 1}, reverse=True):
                Z = _gpu_trbak(gpu_lib, a, e_dev, n, band, mb, Z0[:, :nvec])
                assert np.isfinite(Z).all()
                _judge(f"trbak band={band} n={n} mb={mb} q={q} {family} Z={which} nvec={nvec}", ("E_b",),
                       (hd.solve_error(Z, Zref[:, :nvec]),), bnd)


def _gpu_solve(lib, driver, cs, m, mb, nvec=None, mode=b"A"):
    """the device entry of a driver on the poisoned upper triangle: all of w, the nvec columns of Z"""
    import torch

    n, ld = cs.n, _ld(cs.n)
    nvec = n if nvec is None else nvec
    a = _to_dev(hd.nan_lower(cs.A), ld)
    z = torch.zeros(n, ld, dtype=a.dtype, device=_dev())
    w = torch.zeros(n, dtype=torch.float64, device=_dev())
    assert getattr(lib, ENTRY[driver])(n, nvec, a.data_ptr(), ld, w.data_ptr(), z.data_ptr(), ld, m, mb, mode) == 0
    return w.cpu().numpy(), _from_dev(z, n)[:, :nvec]


WHOLE_PARAMS = [(drv,) + c for drv in ("sx", "s") for c in hd.driver_cases("s")] + [("h",) + c for c in hd.driver_cases("h")]


@pytest.mark.gpu
@pytest.mark.parametrize("driver,n,m,mb,q,family", WHOLE_PARAMS,
                         ids=[f"{p[0]}-" + hd.driver_case_id(KIND_OF[p[0]], p[1:]) for p in WHOLE_PARAMS])
def test_whole_solves(gpu_lib, driver, n, m, mb, q, family):
    """eigx_sx_dev / eigx_s_dev / eigx_h_dev, mode 'A': nvec = n, and nvec = n // 3 with all of w and the returned columns"""
    cs = hd.case(KIND_OF[driver], n, family)
    with _tuned(gpu_lib, [(2, q)]):
        w, Z = _gpu_solve(gpu_lib, driver, cs, m, mb)
        _check_whole(f"whole {driver} n={n} m={m} mb={mb} q={q} {family}", cs, w, Z)
        nvec = max(n // 3, 1)
        w, Z = _gpu_solve(gpu_lib, driver, cs, m, mb, nvec=nvec)
        _check_whole(f"whole {driver} n={n} m={m} mb={mb} q={q} {family} nvec={nvec}", cs, w, Z)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [600, -600])
@pytest.mark.parametrize("family", ["random", "graded", "glued_rot"])
@pytest.mark.parametrize("driver", ["sx", "s", "h"])
def test_exact_scaling(gpu_lib, driver, family, k):
    """A 2^600 and A 2^-600 at n = 130 (inside the rescale range of both scaling rules): the reference scales exactly and the
    metrics are invariant, so the same bounds hold"""
    sc = hd.ScaledDense(hd.case(KIND_OF[driver], 130, family), k)
    w, Z = _gpu_solve(gpu_lib, driver, sc, 48, 48)
    _check_whole(f"whole {driver} n=130 {family} A 2^{k}", sc, w, Z)


H_CASES = hd.driver_cases("h")


@pytest.mark.gpu
@pytest.mark.parametrize("case", H_CASES, ids=[hd.driver_case_id("h", c) for c in H_CASES])
def test_hermitian_reduction_mode_s(gpu_lib, case):
    """eigx_h_dev mode 'S': Z is the reduction's unitary Q.  Q^H A Q is real tridiagonal (E_s: what lies outside the band and
    the imaginary part inside it) and Q is unitary entry by entry.  w of this mode comes from bisection and is not judged."""
    n, m, mb, _, family = case
    cs = hd.case("h", n, family)
    w, Q = _gpu_solve(gpu_lib, "h", cs, m, mb, mode=b"S")
    assert np.isfinite(w).all() and np.isfinite(Q).all()
    assert (np.diff(w) >= 0).all()
    _judge(f"reduce h mode S n={n} m={m} mb={mb} {family}", ("E_s", "E_q"), hd.similarity_metrics(cs.A, Q, None, cs.anorm),
           hd.driver_stage_bounds("h", "reduce", family))
