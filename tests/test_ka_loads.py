"""ka_kernel's load forms on one GPU, through the C-ABI: the panel-dot loads by panel width class (m <= 64, m <= 128, any)
and the tile scalars packed by tile index (eigx_tune keys 10 and 12).  Helpers and tolerances of test_gpu_parity.py."""
import numpy as np
import pytest

from test_gpu_parity import EPS, SIMILARITY_TOL, _band_matrix, _dev, _to_colmajor

pytestmark = pytest.mark.gpu


def _reduce(gpu_lib, A, m, band, poison=False):
    """band reduction of A on the GPU: (a, lda, d, e) as device tensors; a holds the reflectors in its upper triangle"""
    import torch

    n = A.shape[0]
    a, lda = _to_colmajor(A)
    if poison:
        il = torch.tril_indices(n, n, -1, device=_dev())
        a[il[1], il[0]] = float("nan")   # the strict lower triangle must never be read
    d = torch.zeros(n, dtype=torch.float64, device=_dev())
    e = torch.zeros(2 * n, dtype=torch.float64, device=_dev())
    assert gpu_lib.eigx_band_reduce_dev(n, a.data_ptr(), lda, d.data_ptr(), e.data_ptr(), n, m, band) == 0
    return a, lda, d, e


def _fit_pair(gpu_lib, A, m, band, poison=False):
    """the reduction with matched (key 10 = 1) and with the largest (key 10 = 0) load batches: (d, e, upper triangle of a)"""
    n = A.shape[0]
    up = np.triu(np.ones((n, n), dtype=bool)).T          # a[j, i] = A(i, j): upper triangle + reflectors
    out = []
    for fit in (1, 0):
        old = gpu_lib.eigx_tune(10, fit)
        try:
            a, _, d, e = _reduce(gpu_lib, A, m, band, poison)
        finally:
            gpu_lib.eigx_tune(10, old)
        out.append((d.cpu().numpy().copy(), e.cpu().numpy().copy(), a.cpu().numpy()[:, :n][up].copy()))
    return out


def _assert_bit_identical(out):
    for q in range(3):
        assert np.isfinite(out[0][q]).all()
        assert np.array_equal(out[0][q], out[1][q])


def _assert_spectrum(A, d, e, band):
    n = A.shape[0]
    wr = np.linalg.eigvalsh(A)
    T = _band_matrix(d, e.reshape(2, n)[:band], band)
    assert np.abs(np.linalg.eigvalsh(T) - wr).max() < 1e-13 * n * np.abs(wr).max()


# (n, m, strict lower triangle poisoned): (600, 8) smallest class; (600, 50) odd / even rounding of m in the pentadiagonal
# route; (1700, 64): pd_rows_for() gives 4, 3, 2 and 1 row chunks as the active rows shrink through 1536 / 1024 / 512;
# (700, 100), (700, 128): the m <= 128 class; (700, 192): the widest class
PANEL_CASES = [(600, 8, False), (600, 50, False), (600, 64, True), (1700, 64, False), (700, 100, False), (700, 128, False),
               (700, 192, False)]


@pytest.mark.parametrize("band", [1, 2])
@pytest.mark.parametrize("n,m,poison", PANEL_CASES)
def test_panel_dot_width_classes_are_bit_identical(gpu_lib, band, n, m, poison):
    """ka_kernel loads the panel dots once per panel column where the panel is narrow (wave = row chunk for m <= 64, half a
    workgroup = two row chunks for m <= 128) and adds the chunks through LDS in the order of the wide form,
    ((c0 + c1) + c2) + c3; eigx_tune key 10 = 0 selects the wide form everywhere.  d, e and the reflectors must be
    bit-identical either way, the band matrix must have A's spectrum, and nothing may read the strict lower triangle."""
    from eigenexa_amd import layout

    A = layout.random_symmetric(n, seed=41 + band)
    out = _fit_pair(gpu_lib, A, m, band, poison)
    _assert_bit_identical(out)
    _assert_spectrum(A, out[0][0], out[0][1], band)


@pytest.mark.parametrize("band", [1, 2])
@pytest.mark.parametrize("n", [3000, 4100])
def test_packed_tile_scalars_similarity_elementwise(gpu_lib, band, n):
    """the mat-vec stores a tile's three bilinear scalars at its index in the 1-D grid and ka_kernel loads entries
    tid + 256 j: n = 3000 has 24 x 24 tiles of 128 (300 tiles, two batches), n = 4100 has 33 x 33 (561 tiles, three
    batches).  With Q from the real back-transformation, Q^T A Q must be the band matrix element by element (as in
    test_band_is_the_reflectors_similarity_elementwise), evaluated on the GPU."""
    import torch
    from eigenexa_amd import layout

    m, mb = 64, 128
    A = layout.random_symmetric(n, seed=51 + band)
    a, lda, d, e = _reduce(gpu_lib, A, m, band)
    z = torch.zeros(n, lda, dtype=torch.float64, device=_dev())
    z[:, :n] = torch.eye(n, dtype=torch.float64, device=_dev())
    assert gpu_lib.eigx_trbak_dev(n, n, a.data_ptr(), lda, z.data_ptr(), lda, e.data_ptr(), n, mb, band) == 0
    Q = z[:, :n].T
    At = torch.from_numpy(A).to(_dev())
    T = torch.diag(d)
    e2 = e.reshape(2, n)
    for b in range(1, band + 1):
        T += torch.diag(e2[b - 1, b:n], b) + torch.diag(e2[b - 1, b:n], -b)
    anorm = np.abs(A).max() * n
    err_sim = (Q.T @ At @ Q - T).abs().max().item() / anorm
    err_orth = (Q.T @ Q - torch.eye(n, dtype=torch.float64, device=_dev())).abs().max().item()
    print(f"PARITY-MARGIN packed tile scalars band={band} n={n}: |Q^T A Q - T| = {err_sim:.2e} (x n max|A|), |Q^T Q - I| = {err_orth:.2e}")
    assert np.isfinite(err_sim) and err_sim < SIMILARITY_TOL and err_orth < 50 * n * EPS


@pytest.mark.parametrize("band", [1, 2])
def test_packed_tile_scalars_all_tile_sizes_bit_identical(gpu_lib, band):
    """n = 900 with the tile switches forced to 200 / 450 (and non-temporal loads from 300 on), so that the 256 and 512
    tiles store at the packed index as well: matched and largest load batches must agree bit for bit"""
    from eigenexa_amd import layout

    n, m = 900, 64
    A = layout.random_symmetric(n, seed=61 + band)
    tiles = [gpu_lib.eigx_tune(3, 200), gpu_lib.eigx_tune(4, 450), gpu_lib.eigx_tune(5, 300)]
    try:
        out = _fit_pair(gpu_lib, A, m, band)
    finally:
        for key, v in zip((3, 4, 5), tiles):
            gpu_lib.eigx_tune(key, v)
    _assert_bit_identical(out)
    _assert_spectrum(A, out[0][0], out[0][1], band)


@pytest.mark.parametrize("band", [1, 2])
def test_earlier_load_forms_stay_selectable(gpu_lib, band):
    """eigx_tune key 12 keeps the earlier load forms for A/B runs (0: folded tile-scalar rows and wide panel dots, 1: packed
    tile scalars only); each is a correct reduction, and values outside 0 .. 2 are refused"""
    from eigenexa_amd import layout

    n, m = 900, 64
    A = layout.random_symmetric(n, seed=71 + band)
    assert gpu_lib.eigx_tune(12, 3) == -1 and gpu_lib.eigx_tune(12, -1) == -1
    for form in (0, 1):
        old = gpu_lib.eigx_tune(12, form)
        try:
            assert old == 2
            _, _, d, e = _reduce(gpu_lib, A, m, band)
        finally:
            gpu_lib.eigx_tune(12, old)
        _assert_spectrum(A, d.cpu().numpy(), e.cpu().numpy(), band)
