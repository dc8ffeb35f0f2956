"""The band divide and conquer under deflation (tests/hard_band.py): glued and perturbed Wilkinson matrices, exactly equal
poles, zero couplings, graded and near-identity input, judged column by column and entry by entry against an
extended-precision eigenvalue reference.

Bounds: 16 x what LAPACK's own D&C reaches on the same case table (tests/golden/dc_hard_bounds.json, written by
tests/golden/make_dc_hard_bounds.py), per metric and independent of n.  They come from an independent implementation of the
operation, not from the code under test.  The CPU oracle restates the algorithm of csrc/dc.hip and is held to the same
bounds at n <= 200 without a GPU."""
import os

import numpy as np
import pytest

import hard_band as hb

B_W, B_R, B_O = hb.bounds()
CASES = hb.cases()
SWITCH_FAMILIES = ("glued", "equal_d_tiny_e", "half_identity", "wilkinson")


def _check(tag, d, e, band, w, Z, w_ref, nvec=None):
    n = len(d)
    assert np.isfinite(w).all() and np.isfinite(Z).all(), tag
    assert (np.diff(w) >= 0).all(), f"{tag}: w is not ascending"
    E_w, E_r, E_o = hb.metrics(d, e, band, w, Z if nvec is None else Z[:, :nvec], w_ref)
    print(f"DC-HARD {tag} band={band} n={n}: E_w={E_w:.2f} (<{B_W:.1f}) E_r={E_r:.2f} (<{B_R:.1f}) E_o={E_o:.2f} (<{B_O:.1f})")
    assert E_w < B_W and E_r < B_R and E_o < B_O, (tag, E_w, E_r, E_o)
    return E_w, E_r, E_o


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("n", [33, 65, 200])
def test_reference_matches_closed_forms(n):
    """the extended-precision bisection against spectra known in closed form, to 0.1 eps |T|_2 (eps = 2^-52)"""
    LD = hb.LD
    pi = 4 * np.arctan(LD(1))
    k = np.arange(1, n + 1).astype(LD)
    d, e, w = hb.case("toeplitz", n, 1)
    exact = 4 * np.sin(k * pi / (2 * (n + 1))) ** 2            # 2 - 2 cos(k pi / (n + 1)) without the cancellation
    assert float(np.abs(w - exact).max()) < 0.1 * hb.EPS * float(exact.max())
    # Clement's off-diagonal sqrt(i (n - i)) formed in longdouble: rounded to fp64 (as the family stores it) the matrix is
    # another one, up to eps |T|_2 / 2 away from the integer spectrum
    i = np.arange(n).astype(LD)
    w = hb.reference_eigenvalues(np.zeros(n), np.sqrt(i * (n - i))[None, :], 1)
    exact = np.arange(-(n - 1), n, 2).astype(LD)
    assert float(np.abs(w - exact).max()) < 0.1 * hb.EPS * (n - 1)


@pytest.mark.parametrize("n", [33, 65])
def test_reference_band2_route_matches_closed_form(n):
    """the Householder route of band 2 on J^2, J = tridiag(-1, 2, -1): pentadiagonal (1, -4, 6, -4, 1) with 5 in the two
    corners, spectrum 16 sin^4(k pi / (2 (n + 1)))"""
    LD = hb.LD
    pi = 4 * np.arctan(LD(1))
    d = np.full(n, 6.0)
    d[0] = d[-1] = 5.0
    e = np.zeros((2, n))
    e[0, 1:] = -4.0
    e[1, 2:] = 1.0
    w = hb.reference_eigenvalues(d, e, 2)
    exact = 16 * np.sin(np.arange(1, n + 1).astype(LD) * pi / (2 * (n + 1))) ** 4
    assert float(np.abs(w - exact).max()) < 0.1 * hb.EPS * float(exact.max())


def test_bounds_file_is_what_lapack_reaches():
    """the committed JSON covers the case table, and LAPACK recomputed on two small cases is at or under its worst values"""
    import json

    rec = json.load(open(hb.BOUNDS_JSON))
    assert rec["factor"] == hb.BOUND_FACTOR
    assert set(rec["per_case"]) == {f"band{b}-n{n}-{f}" for b, n, f in CASES}
    for k, i in (("E_w", 0), ("E_r", 1), ("E_o", 2)):
        assert rec["worst"][k] == max(v[i] for v in rec["per_case"].values())
    for band, n, name in ((1, 65, "glued"), (2, 33, "equal_d_tiny_e")):
        d, e, w_ref = hb.case(name, n, band)
        w, Z = np.linalg.eigh(hb.band_matrix(d, e, band))
        m = hb.metrics(d, e, band, w, Z, w_ref)
        for k, v in zip(("E_w", "E_r", "E_o"), m):
            assert v <= rec["worst"][k], (name, k, v)


@pytest.mark.parametrize("band,n,family", [c for c in CASES if c[1] <= 200])
def test_oracle_hard_cases(orc, band, n, family):
    d, e, w_ref = hb.case(family, n, band)
    w, Z = orc.band_dc(d, e, band)
    _check(f"oracle {family}", d, e, band, w, Z, w_ref)


# ------------------------------------------------------------------------------------------------ GPU
def _gpu_dc(gpu_lib, d, e, band, nvec=None):
    import torch

    dev = torch.device("cuda:0")
    n = len(d)
    dd = torch.from_numpy(np.ascontiguousarray(d)).to(dev)
    ee = torch.from_numpy(e.reshape(-1).copy()).to(dev)
    ldz = n + (n & 1)
    z = torch.zeros(n, ldz, dtype=torch.float64, device=dev)
    w = torch.zeros(n, dtype=torch.float64, device=dev)
    rc = gpu_lib.eigx_band_dc_dev(n, n if nvec is None else nvec, dd.data_ptr(), ee.data_ptr(), n, band, w.data_ptr(),
                                  z.data_ptr(), ldz)
    assert rc == 0, rc
    return w.cpu().numpy(), z[:, :n].T.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("band,n,family", CASES)
def test_band_dc_hard_cases(gpu_lib, band, n, family):
    d, e, w_ref = hb.case(family, n, band)
    w, Z = _gpu_dc(gpu_lib, d, e, band)
    _check(family, d, e, band, w, Z, w_ref)


@pytest.mark.gpu
@pytest.mark.parametrize("band", [1, 2])
@pytest.mark.parametrize("family", SWITCH_FAMILIES)
def test_band_dc_hard_pipeline_switches(gpu_lib, band, family):
    """every form of the one-GPU pass pipeline (eigx_tune keys 15 / 16; 15 = 64 puts the merges above 64 columns on the side
    stream) on input that deflates: deflated columns copied ahead of the product, rotations, K = 0 merges beside full ones.
    Each setting meets the bounds, and the eigenvalues agree across settings to the tolerance of
    test_band_dc_pass_pipeline_switches"""
    for n in (65, hb.SIZES[band][-1]):
        d, e, w_ref = hb.case(family, n, band)
        tn = max(np.abs(d).max(), np.abs(e).max())
        ws = []
        try:
            for k15, k16 in ((1, 1), (0, 1), (1, 0), (0, 0), (64, 1)):
                if k15 >= 2:
                    gpu_lib.eigx_tune(15, 1)       # a value >= 2 moves the side-stream threshold only: pipeline on first
                gpu_lib.eigx_tune(15, k15)
                gpu_lib.eigx_tune(16, k16)
                w, Z = _gpu_dc(gpu_lib, d, e, band)
                _check(f"{family} keys=({k15},{k16})", d, e, band, w, Z, w_ref)
                ws.append(w)
        finally:
            gpu_lib.eigx_tune(15, 1024)
            gpu_lib.eigx_tune(15, 1)
            gpu_lib.eigx_tune(16, 1)
        for w in ws[1:]:
            assert np.abs(w - ws[0]).max() < 1e-13 * tn * max(1, n / 100), (family, n)


@pytest.mark.gpu
@pytest.mark.parametrize("band", [1, 2])
@pytest.mark.parametrize("family", ["glued", "half_identity"])
def test_band_dc_hard_partial_vectors(gpu_lib, band, family):
    """nvec = n // 3: all of w, and the nvec columns that come back, within the bounds"""
    n = 200
    nvec = n // 3
    d, e, w_ref = hb.case(family, n, band)
    w, Z = _gpu_dc(gpu_lib, d, e, band, nvec=nvec)
    _check(f"{family} nvec={nvec}", d, e, band, w, Z, w_ref, nvec=nvec)


@pytest.mark.gpu
@pytest.mark.parametrize("world,dims", [(2, ""), (4, "2x2"), (3, "3x1")])
def test_multi_rank_dc_under_deflation(world, dims):
    """the distributed D&C (roots split by index, Loewner and eigenvector kernels of the process grid, rotations and
    deflated columns on every rank's rows) on glued, equal_d_tiny_e (eigen_s) and wilkinson band 2 (eigen_sx) at n = 200:
    route `hard` of tests/mg_worker.py, E_r and E_o against the dense input on rank 0"""
    import socket
    import subprocess
    import sys

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = os.path.join(os.path.dirname(__file__), "mg_worker.py")
    env = dict(os.environ)
    env.setdefault("EIGX_SELFTEST_ROUNDS", "40")
    procs = [subprocess.Popen([sys.executable, script, str(r), str(world), str(port), "200", "hard", "0", dims or "-"],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env) for r in range(world)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=600)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    print("".join(line + "\n" for line in outs[0].splitlines() if line.startswith("DC-HARD-MG")), end="")
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"OK rank {r}/{world}" in o, o[-3000:]
