"""Ragged batched complex Hermitian eigensolves (eigen_h_vbatch, an EXTENSION: the reference solves one matrix per call): the
complex sibling of eigen_s_vbatch -- blocks of differing orders (n <= 96 by the kernels, the arithmetic of eigen_h_batch bit for
bit; above the cutoff, eigx_tune key 22, by eigen_h) in one call; a and z interleaved complex, offsets and leading dimensions in
complex elements.  The buffers of a ragged call and the bodies of the tests are those of tests/test_vbatch.py, run here for the
family H: blocks of tests/test_hbatch.py's families with NaN in the strict lower triangles, the padding rows, the gaps and the
imaginary parts of the diagonals; the gates of tests/test_hbatch.py (conjugate transposes)."""
import os

import numpy as np
import pytest

import test_vbatch as vb

H = vb.H


@pytest.mark.gpu
def test_ragged_mixed_call(gpu_lib):
    vb.check_mixed(gpu_lib, H)


@pytest.mark.gpu
def test_more_workgroups_than_the_card_holds(gpu_lib):
    vb.check_many(gpu_lib, H)


@pytest.mark.gpu
def test_bit_identity_with_the_uniform_entry(gpu_lib):
    """w and both planes of z, block by block, against eigx_h_batch_dev(n_k, 1, ...); reversed order; twice"""
    vb.check_bits(gpu_lib, H)


@pytest.mark.gpu
def test_ragged_equals_uniform_at_the_class_edges_with_a_failed_block(gpu_lib):
    """n = 1, 2, 32, 33, 64, 65, 96 and a NaN block between two good ones: w, both planes of z and info, bit for bit"""
    vb.check_edges_with_a_failed_block(gpu_lib, H)


@pytest.mark.gpu
def test_uniform_failed_matrix_leaves_its_neighbours(gpu_lib):
    """eigx_h_batch_dev on three matrices, a NaN in the second, at n = 5, 33, 65: the neighbours equal their solo results"""
    vb.check_uniform_failed_middle(gpu_lib, H)


@pytest.mark.gpu
def test_mode_n(gpu_lib):
    vb.check_mode_n(gpu_lib, H)


@pytest.mark.gpu
def test_failures_are_local(gpu_lib):
    """a NaN in a real part (first block), an Inf in an imaginary part (a middle block), a NaN on a diagonal (last block)"""
    vb.check_failures(gpu_lib, H)


@pytest.mark.gpu
def test_above_the_cutoff(gpu_lib):
    vb.check_above_cutoff(gpu_lib, H)


@pytest.mark.gpu
def test_empty_blocks(gpu_lib):
    vb.check_empty(gpu_lib, H)


@pytest.mark.gpu
def test_scales_in_one_call(gpu_lib):
    vb.check_scales(gpu_lib, H)


@pytest.mark.gpu
def test_host_and_device_forms_agree(gpu_lib):
    vb.check_host_form(gpu_lib, H)


@pytest.mark.gpu
def test_arguments_and_timers(gpu_lib):
    vb.check_arguments(gpu_lib, H)


@pytest.mark.gpu
def test_python_wrapper_on_numpy_and_torch(gpu_lib):
    """api.eigen_h_vbatch and api.eigen_s_vbatch on blocks packed by layout.ragged_offsets: flat numpy arrays (host form), flat
    GPU tensors (device form)"""
    import torch

    import eigenexa_amd as ee
    from eigenexa_amd import api, layout

    n = [4, 0, 33, 70]
    for fam, fn, dt in ((vb.S, ee.eigen_s_vbatch, np.float64), (H, ee.eigen_h_vbatch, np.complex128)):
        mats = [fam.random(k, seed=3 + k) if k else np.zeros((0, 0), dtype=dt) for k in n]
        off_a, la = layout.ragged_offsets(n)
        off_w, lw = layout.ragged_offsets(n, ld=1)
        a = np.zeros(la, dtype=dt)
        for k, M in enumerate(mats):
            a[off_a[k]:off_a[k] + n[k] * n[k]] = M.T.reshape(-1)       # column-major
        w, z, info = np.zeros(lw), np.zeros(la, dtype=dt), np.full(4, 77, dtype=np.int32)
        fn(4, n, a.copy(), off_a, n, w, off_w, z, off_a, n, info=info)
        assert api.last_status() == 0 and (info == 0).all()
        for k, M in enumerate(mats):
            if n[k]:
                Z = z[off_a[k]:off_a[k] + n[k] * n[k]].reshape(n[k], n[k]).T
                fam.check_matrix(M, w[off_w[k]:off_w[k] + n[k]], Z, f"{fam.name}: numpy, block {k}")
        ad, wd, zd = torch.from_numpy(a).to("cuda:0"), torch.zeros(lw, dtype=torch.float64, device="cuda:0"), torch.zeros_like(torch.from_numpy(z)).to("cuda:0")
        fn(4, n, ad, off_a, n, wd, off_w, zd, off_a, n)
        assert api.last_status() == 0
        assert np.array_equal(wd.cpu().numpy(), w) and np.array_equal(zd.cpu().numpy(), z)
        wd.zero_()
        ad.copy_(torch.from_numpy(a))
        fn(4, n, ad, off_a, n, wd, off_w, None, None, None, mode="N")
        assert api.last_status() == 0 and np.array_equal(wd.cpu().numpy(), w)


@pytest.mark.gpu
def test_fortran_hvbatch_caller(gpu_lib, tmp_path):
    """a Fortran program calls eigen_h_vbatch of module eigen_libs_mod on phased Frank blocks of the orders 7, 30, 70 and 12 held
    in flat arrays with 1-based start indices"""
    if not os.path.exists(vb.FLANG):
        pytest.skip("no flang")
    vb.run_fortran_caller(tmp_path, "hvbatch_caller")


# ------------------------------------------------------------------------------------------------ CPU
def test_python_wrapper_rejects_bad_arguments_before_the_library(monkeypatch, capsys):
    vb.wrapper_refusals("eigen_h_vbatch", np.complex128, monkeypatch, capsys)
