"""The one-GPU trailing update C(upper tiles) = alpha P Q^T + beta C at short K, through eigx_dgemm_dev(..., tri_mode = 1):
the ring kernel's late-C path (eigx_tune key 25 = largest K it serves, 0 = the early-C path everywhere) against torch fp64
on edge tiles of every kind, and the reduction that uses it against the oracle.  Helpers and tolerances of
test_gpu_parity.py."""
import numpy as np
import pytest

from test_gpu_parity import TRD_ELEMENT_TOL, _dev, _to_colmajor

pytestmark = pytest.mark.gpu

KEY = 25
# n: one tile (2, 127, 128), one row / column in the second tile (129), a 3 x 3 grid with a one-wide edge (257), a 6 x 6
# grid (700, tile blocks of 1), a 10 x 10 grid walked in 2 x 2 blocks that the grid is no multiple of (1153)
SIZES = [2, 127, 128, 129, 257, 700, 1153]
# K: less than one slab (2), one slab (8), just below / at / just above the S - 1 = 3 prologue slabs (22, 24, 26), the
# panel widths m = 48 and 64 (96, 128), the largest short K (256), and 512, which stays on the early-C path
KS = [2, 8, 22, 24, 26, 96, 128, 256, 512]
K_LONG = 512


def _bits(t):
    import torch

    return t.contiguous().view(torch.int64)


def _tri_update(gpu_lib, Pt, Qt, Ct, n, k, ld, alpha, beta):
    import torch

    torch.cuda.synchronize()
    assert gpu_lib.eigx_dgemm_dev(b"N", b"T", n, n, k, alpha, Pt.data_ptr(), ld, Qt.data_ptr(), ld, beta,
                                  Ct.data_ptr(), ld, 1) == 0


@pytest.fixture(params=[0, None], ids=["early_c", "default"])
def key_setting(request, gpu_lib):
    """key 25 at 0 (the early-C path for every K) and at the library's default"""
    if request.param is None:
        default = gpu_lib.eigx_tune(KEY, 0)   # read the default, put it back
        gpu_lib.eigx_tune(KEY, default)
        yield default
        return
    old = gpu_lib.eigx_tune(KEY, request.param)
    try:
        yield request.param
    finally:
        gpu_lib.eigx_tune(KEY, old)


def test_key_range(gpu_lib):
    """the default serves K = 96 .. 256 and not K = 512; values that would reach K = 512 are refused"""
    default = gpu_lib.eigx_tune(KEY, 0)
    assert gpu_lib.eigx_tune(KEY, default) == 0
    assert 256 <= default < K_LONG
    assert gpu_lib.eigx_tune(KEY, K_LONG) == -1 and gpu_lib.eigx_tune(KEY, -1) == -1
    assert gpu_lib.eigx_tune(KEY, default) == default


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", SIZES)
def test_short_k_upper_triangle(gpu_lib, key_setting, n, k):
    """tiles that touch the upper triangle hold alpha P Q^T + beta C to 1e-12 K (the ring kernel's bound in
    test_gpu_parity.py); the tiles strictly below the block diagonal and the padding rows keep their bits; with NaN in the
    strictly lower tiles the upper result does not change, so no chunk of C came from a wrong tile.  K = 512 runs the
    early-C path whatever the key says: bit-identical to the key at 0."""
    import torch

    torch.manual_seed(1000 * n + k)
    ld = n + (n & 1) + 2
    P = torch.randn(n, k, dtype=torch.float64, device=_dev())
    Q = torch.randn(n, k, dtype=torch.float64, device=_dev())
    Pt = torch.zeros(k, ld, dtype=torch.float64, device=_dev()); Pt[:, :n] = P.T
    Qt = torch.zeros(k, ld, dtype=torch.float64, device=_dev()); Qt[:, :n] = Q.T
    C0t = torch.randn(n, ld, dtype=torch.float64, device=_dev())   # padding rows random too
    C0 = C0t[:, :n].T
    PQ = P @ Q.T
    t = torch.arange(n, device=_dev()) // 128
    mask = t[:, None] <= t[None, :]
    for alpha, beta in ((-1.0, 1.0), (-0.5, 2.0)):
        Ct = C0t.clone()
        _tri_update(gpu_lib, Pt, Qt, Ct, n, k, ld, alpha, beta)
        got = Ct[:, :n].T
        ref = alpha * PQ + beta * C0
        err = ((got - ref) * mask).abs().max().item()
        print(f"SHORT-K n={n} K={k} key={key_setting} alpha={alpha} beta={beta}: err {err:.2e} (bound {1e-12 * k:.1e})")
        assert err < 1e-12 * k
        assert torch.equal(_bits(got[~mask]), _bits(C0[~mask]))
        assert torch.equal(_bits(Ct[:, n:]), _bits(C0t[:, n:]))
        # NaN in every strictly lower tile
        Cn = C0t.clone()
        Cn[:, :n].T[~mask] = float("nan")
        Cn0 = Cn.clone()
        _tri_update(gpu_lib, Pt, Qt, Cn, n, k, ld, alpha, beta)
        gn = Cn[:, :n].T
        assert torch.isfinite(gn[mask]).all()
        assert torch.equal(_bits(gn[mask]), _bits(got[mask]))
        assert torch.equal(_bits(Cn[:, :n].T[~mask]), _bits(Cn0[:, :n].T[~mask]))
        assert torch.equal(_bits(Cn[:, n:]), _bits(Cn0[:, n:]))
        if k >= K_LONG and key_setting != 0:
            old = gpu_lib.eigx_tune(KEY, 0)
            try:
                Ce = C0t.clone()
                _tri_update(gpu_lib, Pt, Qt, Ce, n, k, ld, alpha, beta)
            finally:
                gpu_lib.eigx_tune(KEY, old)
            assert torch.equal(_bits(Ce), _bits(Ct))


@pytest.mark.parametrize("n,m", [(513, 48), (700, 64)])
def test_tridiagonal_matches_oracle_short_k(gpu_lib, orc, key_setting, n, m):
    """the reduction whose trailing updates have K = 2 m = 96 and 128: (d, |e|) element-wise against the oracle, bound
    1e-12 n max|A| as in test_tridiagonal_matches_oracle"""
    import torch
    from eigenexa_amd import layout

    A = layout.random_symmetric(n, seed=11)
    do, eo, _ = orc.band_reduce(A, 1)
    a, lda = _to_colmajor(A)
    il = torch.tril_indices(n, n, -1, device=_dev())
    a[il[1], il[0]] = float("nan")   # the strict lower triangle must never be read
    d = torch.zeros(n, dtype=torch.float64, device=_dev())
    e = torch.zeros(n, dtype=torch.float64, device=_dev())
    assert gpu_lib.eigx_band_reduce_dev(n, a.data_ptr(), lda, d.data_ptr(), e.data_ptr(), n, m, 1) == 0
    scale = np.abs(A).max() * n
    err_d = np.abs(d.cpu().numpy() - do).max() / scale
    err_e = np.abs(np.abs(e.cpu().numpy()) - np.abs(eo[0])).max() / scale
    print(f"PARITY-MARGIN tridiagonal n={n} m={m} key={key_setting}: |d - d_oracle| = {err_d:.2e}, "
          f"||e| - |e_oracle|| = {err_e:.2e}  (x n max|A|)")
    assert err_d < TRD_ELEMENT_TOL and err_e < TRD_ELEMENT_TOL
