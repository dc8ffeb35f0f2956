"""Ragged batched complex generalised eigensolves (eigen_hgev_vbatch, an EXTENSION: the reference has no complex generalised
solver): the complex sibling of eigen_gev_vbatch -- Hermitian-definite pencils of differing orders (n <= 64 by the kernels, the
arithmetic of eigen_hgev_batch bit for bit; above the cutoff, eigx_tune key 24, by eigx_hgev_range_dev) in one call; a, b and z
interleaved complex, offsets and leading dimensions in complex elements.  The buffers of a ragged call and the bodies of the
tests are those of tests/test_gvbatch.py, run here for the family HG: pencils of tests/test_hgbatch.py with NaN in the strict
lower triangles, the padding rows, the gaps and the imaginary parts of both diagonals; the gates of tests/test_hgbatch.py
(conjugate transposes; Im diag(U) exactly 0)."""
import os

import numpy as np
import pytest

import test_gvbatch as gv

HG = gv.HG


@pytest.mark.gpu
def test_ragged_mixed_call(gpu_lib):
    gv.check_mixed(gpu_lib, HG)


@pytest.mark.gpu
def test_bit_identity_with_the_uniform_entry(gpu_lib):
    """w and both planes of z and b, block by block, against eigx_hgev_batch_dev(n_k, 1, ...); twice; reversed order"""
    gv.check_bits(gpu_lib, HG)


@pytest.mark.gpu
def test_ragged_equals_uniform_at_the_class_edges_with_failed_blocks(gpu_lib):
    """n = 1, 2, 32, 33, 64, a NaN block and one with an indefinite B between good ones: w, both planes of z and b, and info"""
    gv.check_edges_with_failed_blocks(gpu_lib, HG)


@pytest.mark.gpu
def test_uniform_failed_pencil_leaves_its_neighbours(gpu_lib):
    """eigx_hgev_batch_dev on three pencils, the second failing (NaN in A; indefinite B), at n = 5, 33: the neighbours equal
    their solo results"""
    gv.check_uniform_failed_middle(gpu_lib, HG)


@pytest.mark.gpu
def test_more_workgroups_than_the_card_holds(gpu_lib):
    gv.check_many(gpu_lib, HG)


@pytest.mark.gpu
def test_mode_n(gpu_lib):
    gv.check_mode_n(gpu_lib, HG)


@pytest.mark.gpu
def test_failures_are_local(gpu_lib):
    """a NaN in a real part of A, an Inf in an imaginary part of B, B = -I: b of all three failed blocks is as it was passed"""
    gv.check_failures(gpu_lib, HG)


@pytest.mark.gpu
def test_above_the_cutoff(gpu_lib):
    gv.check_above_cutoff(gpu_lib, HG)


@pytest.mark.gpu
def test_empty_blocks(gpu_lib):
    gv.check_empty(gpu_lib, HG)


@pytest.mark.gpu
def test_host_and_device_forms_agree(gpu_lib):
    gv.check_host_form(gpu_lib, HG)


@pytest.mark.gpu
def test_arguments_and_timers(gpu_lib):
    gv.check_arguments(gpu_lib, HG)


@pytest.mark.gpu
def test_python_wrapper_on_numpy_and_torch(gpu_lib):
    """api.eigen_gev_vbatch and api.eigen_hgev_vbatch on pencils packed by layout.ragged_offsets: flat numpy arrays (host form),
    flat GPU tensors (device form)"""
    import torch

    import eigenexa_amd as ee
    from eigenexa_amd import api, layout

    n = [4, 0, 33, 50]
    for fam, fn, dt in ((gv.G, ee.eigen_gev_vbatch, np.float64), (HG, ee.eigen_hgev_vbatch, np.complex128)):
        pairs = [fam.random(k, 1, 3 + k) if k else ([np.zeros((0, 0), dtype=dt)], [np.zeros((0, 0), dtype=dt)]) for k in n]
        As, Bs = [p[0][0] for p in pairs], [p[1][0] for p in pairs]
        off, la = layout.ragged_offsets(n)
        off_w, lw = layout.ragged_offsets(n, ld=1)
        a, b = np.zeros(la, dtype=dt), np.zeros(la, dtype=dt)
        for k in range(4):
            a[off[k]:off[k] + n[k] * n[k]] = As[k].T.reshape(-1)       # column-major
            b[off[k]:off[k] + n[k] * n[k]] = Bs[k].T.reshape(-1)
        w, z, info = np.zeros(lw), np.zeros(la, dtype=dt), np.full(4, 77, dtype=np.int32)
        u = b.copy()
        fn(4, n, a.copy(), off, n, u, off, n, w, off_w, z, off, n, info=info)
        assert api.last_status() == 0 and (info == 0).all()
        for k in range(4):
            if n[k]:
                Z = z[off[k]:off[k] + n[k] * n[k]].reshape(n[k], n[k]).T
                U = np.triu(u[off[k]:off[k] + n[k] * n[k]].reshape(n[k], n[k]).T)
                fam.gates(As[k], Bs[k], w[off_w[k]:off_w[k] + n[k]], Z, U, f"{fam.name}: numpy, block {k}")
        ad, bd = torch.from_numpy(a).to("cuda:0"), torch.from_numpy(b).to("cuda:0")
        wd, zd = torch.zeros(lw, dtype=torch.float64, device="cuda:0"), torch.zeros_like(torch.from_numpy(z)).to("cuda:0")
        fn(4, n, ad, off, n, bd, off, n, wd, off_w, zd, off, n)
        assert api.last_status() == 0
        assert np.array_equal(wd.cpu().numpy(), w) and np.array_equal(zd.cpu().numpy(), z) and np.array_equal(bd.cpu().numpy(), u)
        wd.zero_()
        ad.copy_(torch.from_numpy(a))
        bd.copy_(torch.from_numpy(b))
        fn(4, n, ad, off, n, bd, off, n, wd, off_w, None, None, None, mode="N")
        assert api.last_status() == 0 and np.array_equal(wd.cpu().numpy(), w) and np.array_equal(bd.cpu().numpy(), u)


@pytest.mark.gpu
def test_fortran_hgvbatch_caller(gpu_lib, tmp_path):
    """a Fortran program calls eigen_hgev_vbatch of module eigen_libs_mod on phased Frank / Helmert pencils of the orders 7, 30, 60
    and 12 held in flat arrays with 1-based start indices"""
    if not os.path.exists(gv.FLANG):
        pytest.skip("no flang")
    gv.run_fortran_caller(tmp_path, "hgvbatch_caller")


# ------------------------------------------------------------------------------------------------ CPU
def test_python_wrapper_rejects_bad_arguments_before_the_library(monkeypatch, capsys):
    gv.wrapper_refusals("eigen_hgev_vbatch", np.complex128, monkeypatch, capsys)
