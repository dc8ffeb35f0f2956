"""ctypes binding of libeigenexa_amd.so (the C-ABI declared in include/eigenexa_amd.h and the files it includes).

There is no CPU fallback: if the HIP library is missing or no GPU is visible the calls fail loudly.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# EIGX_LIB: alternative build of the same library (tools/: the diagnostic build with in-kernel stamps)
LIB_PATH = os.environ.get("EIGX_LIB") or os.path.join(_HERE, "lib", "libeigenexa_amd.so")

_c_double_p = C.POINTER(C.c_double)
_c_int_p = C.POINTER(C.c_int)

# argument lists that several entries share: the host and the device form of an entry, the sx / s / h routes, the real
# and the complex sibling.  Arrays are void*.
_INT, _PTR = C.c_int, C.c_void_p
# n, nvec, a, lda, w, z, ldz, m_forward, m_backward, mode
_SOLVE = [_INT, _INT, _PTR, _INT, _PTR, _PTR, _INT, _INT, _INT, C.c_char]
# route, n, nvec, a, lda, w, z, ldz, nb, m_forward, m_backward, mode
_SOLVE_BC = [_INT, _INT, _INT, _PTR, _INT, _PTR, _PTR, _INT, _INT, _INT, _INT, C.c_char]
# n, il, iu, a, lda, w, z, ldz, m_forward, m_backward, mode
_RANGE = [_INT, _INT, _INT, _PTR, _INT, _PTR, _PTR, _INT, _INT, _INT, C.c_char]
# n, vl, vu, mmax, m, il, a, lda, w, z, ldz, m_forward, m_backward, mode
_RANGE_V = [_INT, C.c_double, C.c_double, _INT, _c_int_p, _c_int_p, _PTR, _INT, _PTR, _PTR, _INT, _INT, _INT, C.c_char]
# n, a, lda, b, ldb, w, z, ldz
_GEV = [_INT, _PTR, _INT, _PTR, _INT, _PTR, _PTR, _INT]
# n, il, iu, a, lda, b, ldb, w, z, ldz, mode
_GEV_RANGE = [_INT, _INT, _INT, _PTR, _INT, _PTR, _INT, _PTR, _PTR, _INT, C.c_char]
# n, vl, vu, mmax, m, il, a, lda, b, ldb, w, z, ldz, mode
_GEV_RANGE_V = [_INT, C.c_double, C.c_double, _INT, _c_int_p, _c_int_p, _PTR, _INT, _PTR, _INT, _PTR, _PTR, _INT, C.c_char]
# n, batch, a, lda, stride_a, w, ldw, z, ldz, stride_z, mode, info
_BATCH = [_INT, _INT, _PTR, _INT, C.c_int64, _PTR, _INT, _PTR, _INT, C.c_int64, C.c_char, _PTR]
# n, batch, a, lda, stride_a, b, ldb, stride_b, w, ldw, z, ldz, stride_z, mode, info
_GEV_BATCH = [_INT, _INT, _PTR, _INT, C.c_int64, _PTR, _INT, C.c_int64, _PTR, _INT, _PTR, _INT, C.c_int64, C.c_char, _PTR]
# the index helpers: index, nnod, inod
_INDEX = [_INT, _INT, _INT]
# stages of the Cholesky route: (n, b, ldb), (trans, n, nrhs, u, ldu, x, ldx), (n, a, lda, u, ldu)
_CHOL = [_INT, _PTR, _INT]
_TRSM = [C.c_char, _INT, _INT, _PTR, _INT, _PTR, _INT]
_REDUCE = [_INT, _PTR, _INT, _PTR, _INT]

# name -> (restype, argtypes); mirrors include/eigenexa_amd.h one to one
SIGNATURES = {
    "eigx_init": (C.c_int, [C.c_int]),
    "eigx_init_multi": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_char]),
    "eigx_get_rccl_unique_id": (C.c_int, [C.c_void_p]),
    "eigx_get_device_count": (C.c_int, []),
    "eigx_get_comm": (C.c_int, [C.POINTER(C.c_int)] * 4),
    "eigx_comm_seconds": (C.c_double, []),
    "eigx_comm_info": (C.c_int, [C.c_char_p, C.c_int]),
    "eigx_rccl_selftest": (C.c_int, []),
    "eigx_free": (C.c_int, []),
    "eigx_get_version": (C.c_int, [_c_int_p, C.c_char_p, C.c_char_p]),
    "eigx_get_procs": (C.c_int, [_c_int_p, _c_int_p, _c_int_p]),
    "eigx_get_id": (C.c_int, [_c_int_p, _c_int_p, _c_int_p]),
    "eigx_get_errinfo": (C.c_int, [C.POINTER(C.c_int64)]),
    "eigx_get_matdims": (C.c_int, [C.c_int, _c_int_p, _c_int_p, C.c_int, C.c_int, C.c_char]),
    "eigx_matdims_for_grid": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char, _c_int_p, _c_int_p]),
    "eigx_held_bytes": (C.c_int64, []),
    "eigx_held_bytes_named": (C.c_int64, [C.c_char_p]),
    "eigx_transpose_plan": (C.c_int, [C.c_int] * 6 + [C.POINTER(C.c_int)] * 5),
    "eigx_memory_internal": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "eigx_loop_start": (C.c_int, _INDEX),
    "eigx_loop_end": (C.c_int, _INDEX),
    "eigx_translate_l2g": (C.c_int, _INDEX),
    "eigx_translate_g2l": (C.c_int, _INDEX),
    "eigx_owner_node": (C.c_int, _INDEX),
    "eigx_owner_index": (C.c_int, _INDEX),
    "eigx_sx": (C.c_int, _SOLVE),
    "eigx_s": (C.c_int, _SOLVE),
    "eigx_sx_dev": (C.c_int, _SOLVE),
    "eigx_s_dev": (C.c_int, _SOLVE),
    "eigx_solve_bc": (C.c_int, _SOLVE_BC),
    "eigx_solve_bc_dev": (C.c_int, _SOLVE_BC),
    "eigx_numroc": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "eigx_h": (C.c_int, _SOLVE),
    "eigx_h_dev": (C.c_int, _SOLVE),
    "eigx_set_grid_dims": (C.c_int, [C.c_int, C.c_int]),
    "eigx_band_reduce_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_int, C.c_int]),
    "eigx_band_dc_dev": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_int]),
    "eigx_gev": (C.c_int, _GEV),
    "eigx_gev_dev": (C.c_int, _GEV),
    # extension (not in the reference): complex Hermitian generalised problem
    "eigx_hgev": (C.c_int, _GEV),
    "eigx_hgev_dev": (C.c_int, _GEV),
    # extension (not in the reference): index-range solves on one GPU and their stages
    "eigx_sx_range": (C.c_int, _RANGE),
    "eigx_s_range": (C.c_int, _RANGE),
    "eigx_sx_range_dev": (C.c_int, _RANGE),
    "eigx_s_range_dev": (C.c_int, _RANGE),
    # extension: the same by value window (vl <= lambda < vu); m and il come back through host int pointers
    "eigx_sx_range_v": (C.c_int, _RANGE_V),
    "eigx_s_range_v": (C.c_int, _RANGE_V),
    "eigx_sx_range_v_dev": (C.c_int, _RANGE_V),
    "eigx_s_range_v_dev": (C.c_int, _RANGE_V),
    "eigx_gev_range_v": (C.c_int, _GEV_RANGE_V),
    "eigx_gev_range_v_dev": (C.c_int, _GEV_RANGE_V),
    "eigx_band_count_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "eigx_band_bisect_range_dev": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                             C.c_void_p]),
    "eigx_band_eigvec_dev": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_int]),
    "eigx_range_info": (C.c_int, [_c_int_p, _c_int_p, _c_double_p]),
    "eigx_range_timers": (C.c_int, [_c_double_p]),
    # extension (not in the reference): Cholesky-route generalised range solver and its triangular stages
    "eigx_gev_range": (C.c_int, _GEV_RANGE),
    "eigx_gev_range_dev": (C.c_int, _GEV_RANGE),
    "eigx_chol_dev": (C.c_int, _CHOL),
    "eigx_trsm_upper_dev": (C.c_int, _TRSM),
    "eigx_gev_reduce_dev": (C.c_int, _REDUCE),
    # extension (not in the reference): the same for the complex Hermitian generalised problem (csrc/ztri.hip, on the
    # split planes of csrc/zplanes.hip)
    "eigx_hgev_range": (C.c_int, _GEV_RANGE),
    "eigx_hgev_range_dev": (C.c_int, _GEV_RANGE),
    # extension: index and value windows of eigen_h, the value window of the complex generalised problem
    "eigx_h_range": (C.c_int, _RANGE),
    "eigx_h_range_dev": (C.c_int, _RANGE),
    "eigx_h_range_v": (C.c_int, _RANGE_V),
    "eigx_h_range_v_dev": (C.c_int, _RANGE_V),
    "eigx_hgev_range_v": (C.c_int, _GEV_RANGE_V),
    "eigx_hgev_range_v_dev": (C.c_int, _GEV_RANGE_V),
    # extension: many small symmetric matrices in one call (csrc/batch.hip); strides are int64_t, info int*
    "eigx_s_batch": (C.c_int, _BATCH),
    "eigx_s_batch_dev": (C.c_int, _BATCH),
    # extension: many small complex Hermitian matrices in one call (csrc/hbatch.hip); a, z interleaved complex
    "eigx_h_batch": (C.c_int, _BATCH),
    "eigx_h_batch_dev": (C.c_int, _BATCH),
    "eigx_zchol_dev": (C.c_int, _CHOL),
    "eigx_ztrsm_upper_dev": (C.c_int, _TRSM),
    "eigx_hgev_reduce_dev": (C.c_int, _REDUCE),
    "eigx_band_bisect_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "eigx_trbak_dev": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                 C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "eigx_dgemm_dev": (C.c_int, [C.c_char, C.c_char, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p,
                                 C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_int, C.c_int]),
    "eigx_dgemm_gather_dev": (C.c_int, [C.c_char, C.c_char, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p,
                                        C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_int, C.c_void_p,
                                        C.c_void_p]),
    "eigx_get_timers": (C.c_int, [_c_double_p]),
    "eigx_profile": (C.c_int, [C.c_int]),
    "eigx_profile_read": (C.c_int, [_c_double_p]),
    "eigx_profile_read_kinds": (C.c_int, [_c_double_p, C.c_int]),
    "eigx_tune": (C.c_int, [C.c_int, C.c_int]),
    "eigx_device_synchronize": (C.c_int, []),
    "eigx_malloc_dev": (C.c_void_p, [C.c_int64]),
    "eigx_free_dev": (C.c_int, [C.c_void_p]),
    "eigx_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "eigx_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
}

# The same for include/eigenexa_amd_gbatch.h (which eigenexa_amd.h includes) -- extension: many small symmetric-definite
# pencils in one call (csrc/gbatch.hip); b comes back as U.  A table of its own: SIGNATURES above is held fixed,
# name by name and in order, by tests/test_api_frontend.py.
GBATCH_SIGNATURES = {
    "eigx_gev_batch": (C.c_int, _GEV_BATCH),
    "eigx_gev_batch_dev": (C.c_int, _GEV_BATCH),
}

# The same for include/eigenexa_amd_hgbatch.h -- extension: many small Hermitian-definite pencils in one call
# (csrc/hgbatch.hip); a, b, z interleaved complex, b comes back as U.  The argument kinds are those of eigx_gev_batch.
HGBATCH_SIGNATURES = {
    "eigx_hgev_batch": (C.c_int, _GEV_BATCH),
    "eigx_hgev_batch_dev": (C.c_int, _GEV_BATCH),
}

# The same for include/eigenexa_amd_vbatch.h -- extension: ragged batches, every block with its own order (csrc/vbatch.hip,
# csrc/hvbatch.hip).  The six descriptor arrays (n, off_a, lda, off_w, off_z, ldz) are host arrays in both forms.
# batch, n, a, off_a, lda, w, off_w, z, off_z, ldz, mode, info
_VBATCH = [_INT, _PTR, _PTR, _PTR, _PTR, _PTR, _PTR, _PTR, _PTR, _PTR, C.c_char, _PTR]
VBATCH_SIGNATURES = {
    "eigx_s_vbatch": (C.c_int, _VBATCH),
    "eigx_s_vbatch_dev": (C.c_int, _VBATCH),
    "eigx_h_vbatch": (C.c_int, _VBATCH),
    "eigx_h_vbatch_dev": (C.c_int, _VBATCH),
    # batch, n, cutoff, top, order, counts6 (host arithmetic only)
    "eigx_vbatch_plan": (C.c_int, [_INT, _PTR, _INT, _INT, _PTR, _PTR]),
}

# The same for include/eigenexa_amd_gvbatch.h -- extension: ragged batches of pencils (csrc/gvbatch.hip, csrc/hgbatch.hip,
# DESIGN 8m).  The eight descriptor arrays (n, off_a, lda, off_b, ldb, off_w, off_z, ldz) are host arrays in both forms.
# batch, n, a, off_a, lda, b, off_b, ldb, w, off_w, z, off_z, ldz, mode, info
_GVBATCH = [_INT, _PTR, _PTR, _PTR, _PTR, _PTR, _PTR, _PTR, _PTR, _PTR, _PTR, _PTR, _PTR, C.c_char, _PTR]
GVBATCH_SIGNATURES = {
    "eigx_gev_vbatch": (C.c_int, _GVBATCH),
    "eigx_gev_vbatch_dev": (C.c_int, _GVBATCH),
    "eigx_hgev_vbatch": (C.c_int, _GVBATCH),
    "eigx_hgev_vbatch_dev": (C.c_int, _GVBATCH),
}

# The same for include/eigenexa_amd_batch_range.h -- extension: eigenpairs il .. iu of every matrix of a uniform batch
# (csrc/batch_range.hip), and what the last such call did (three host int pointers).
# n, batch, il, iu, a, lda, stride_a, w, ldw, z, ldz, stride_z, mode, info
_BATCH_RANGE = [_INT, _INT, _INT, _INT, _PTR, _INT, C.c_int64, _PTR, _INT, _PTR, _INT, C.c_int64, C.c_char, _PTR]
BATCH_RANGE_SIGNATURES = {
    "eigx_s_batch_range": (C.c_int, _BATCH_RANGE),
    "eigx_s_batch_range_dev": (C.c_int, _BATCH_RANGE),
    "eigx_batch_range_info": (C.c_int, [_c_int_p, _c_int_p, _c_int_p]),
}

# The same for include/eigenexa_amd_hbatch_range.h -- extension: the Hermitian sibling (csrc/hbatch_range.hip); a, z
# interleaved complex, the argument kinds those of eigx_s_batch_range.  eigx_batch_range_info above reports these calls too.
HBATCH_RANGE_SIGNATURES = {
    "eigx_h_batch_range": (C.c_int, _BATCH_RANGE),
    "eigx_h_batch_range_dev": (C.c_int, _BATCH_RANGE),
}

# The same for include/eigenexa_amd_gbatch_range.h -- extension: the pencil sibling (csrc/gbatch_range.hip); b comes
# back as U.  eigx_batch_range_info above reports these calls too.
# n, batch, il, iu, a, lda, stride_a, b, ldb, stride_b, w, ldw, z, ldz, stride_z, mode, info
_GEV_BATCH_RANGE = [_INT, _INT, _INT, _INT, _PTR, _INT, C.c_int64, _PTR, _INT, C.c_int64, _PTR, _INT, _PTR, _INT, C.c_int64,
                    C.c_char, _PTR]
GBATCH_RANGE_SIGNATURES = {
    "eigx_gev_batch_range": (C.c_int, _GEV_BATCH_RANGE),
    "eigx_gev_batch_range_dev": (C.c_int, _GEV_BATCH_RANGE),
}

# The same for include/eigenexa_amd_hgbatch_range.h -- extension: the complex pencil sibling (csrc/hgbatch_range.hip); a, b,
# z interleaved complex, b comes back as U.  The argument kinds are those of eigx_gev_batch_range.
HGBATCH_RANGE_SIGNATURES = {
    "eigx_hgev_batch_range": (C.c_int, _GEV_BATCH_RANGE),
    "eigx_hgev_batch_range_dev": (C.c_int, _GEV_BATCH_RANGE),
}

# The same for include/eigenexa_amd_gemm_lab.h, which eigenexa_amd.h does NOT include: a test interface to the GEMM dispatcher
# (csrc/gemm_lab.hip) for tests/test_gemm_paths.py; nothing in the package calls it.  Strides are int64_t; the table of
# eigx_dgemm_gather_table_dev is a host int64_t array.
LAB_SIGNATURES = {
    # opa, opb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc, tri_mode, px_n, px, py_n, py, batch, stride_a, stride_b, stride_c,
    # batch2, stride_a2, stride_b2, stride_c2, tn_lo, tn_hi, kmap_a, kmap_b
    "eigx_dgemm_ex_dev": (C.c_int, [C.c_char, C.c_char, _INT, _INT, _INT, C.c_double, _PTR, _INT, _PTR, _INT, C.c_double, _PTR,
                                    _INT, _INT, _INT, _INT, _INT, _INT, _INT, C.c_int64, C.c_int64, C.c_int64, _INT, C.c_int64,
                                    C.c_int64, C.c_int64, _INT, _INT, _PTR, _PTR]),
    # m, n, px_n, px, py_n, py, tn_lo, tn_hi (host arithmetic only)
    "eigx_dgemm_tri2_launch_tiles": (C.c_int, [_INT] * 8),
    # nbatch, entries, a, lda, b, ldb, c, ldc, kmap_a, kmap_b
    "eigx_dgemm_gather_table_dev": (C.c_int, [_INT, _PTR, _PTR, _INT, _PTR, _INT, _PTR, _INT, _PTR, _PTR]),
}

_lib = None


def load():
    """Load the shared library (building is __graft_entry__.build()'s job)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with tools/build_lib.sh (hipcc --offload-arch=gfx950). "
            "eigenexa_amd has no CPU fallback."
        )
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in {**SIGNATURES, **GBATCH_SIGNATURES, **HGBATCH_SIGNATURES, **VBATCH_SIGNATURES,
                               **GVBATCH_SIGNATURES, **BATCH_RANGE_SIGNATURES, **HBATCH_RANGE_SIGNATURES,
                               **GBATCH_RANGE_SIGNATURES, **HGBATCH_RANGE_SIGNATURES}.items():
        fn = getattr(lib, name)  # AttributeError = header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    # the test interface is no load requirement of the package: an earlier build of the library (EIGX_LIB, the A/B runs of
    # profiles/) has none; tests/test_gemm_paths.py holds this tree's build to the whole table
    for name, (res, args) in LAB_SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed with code {rc}")
