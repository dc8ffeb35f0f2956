"""Python mirror of the reference's public API (module eigen_libs_mod, src/eigen_libs.F:14-218).

Names, argument order, defaults and error behaviour follow the Fortran interface:

    call eigen_init([comm],[order])                      src/eigen_libs.F:70-104
    call eigen_get_matdims(n, nx, ny[, m_f, m_b, mode])  src/eigen_libs.F:106-148
    call eigen_sx(n, nvec, a, lda, w, z, ldz[, m_forward, m_backward, mode])   src/eigen_sx.F:30-308
    call eigen_s (n, nvec, a, lda, w, z, ldz[, m_forward, m_backward, mode])   src/eigen_libs.F:150-202
    call eigen_free()                                    src/eigen_libs.F:204-216

``a``, ``w``, ``z`` are either numpy arrays (host, Fortran order, as in the reference) or torch CUDA
tensors laid out column-major (device-resident: no PCIe traffic).  Like the reference the solvers have
no status argument: precondition failures print a warning and return; NaN/Inf input sets ``w`` to NaN
(src/eigen_sx.F:82-131, :151-155).  The last status code is kept in ``last_status`` for tests.
"""
import ctypes as C
import sys

import numpy as np

from . import _lib

# defaults of the reference (src/eigen_libs0.F:49-51)
eigen_NB_f = 48
eigen_NB_b = 128

_state = {"initialized": False, "comm": None, "last_status": 0}


def last_status():
    return _state["last_status"]


def _char(c, default):
    if c is None:
        c = default
    if isinstance(c, bytes):
        return c[:1]
    return str(c)[:1].encode()


def eigen_init(comm=None, order="C", device=None, dims=None):
    """eigen_init(comm, order): ``comm`` is None (single GPU) or an initialised ``torch.distributed``
    process group / True for the default group (one process per GPU; RCCL communicators are built from
    a unique id broadcast over it).  ``order`` 'R' or 'C' as in the reference (src/eigen_libs.F:88-97).
    ``dims`` = (Px, Py): explicit process grid, the counterpart of passing a 2-D cartesian communicator
    (src/eigen_libs0.F:579-715)."""
    lib = _lib.load()
    if dims is not None:
        _lib.check(lib.eigx_set_grid_dims(int(dims[0]), int(dims[1])), "eigx_set_grid_dims")
    rank, nranks = 0, 1
    dist = None
    if comm is not None and comm is not False:
        import torch.distributed as dist_mod

        dist = dist_mod
        group = None if comm is True else comm
        rank = dist.get_rank(group)
        nranks = dist.get_world_size(group)
    if device is None:
        import os

        device = int(os.environ.get("LOCAL_RANK", "0")) if nranks > 1 else 0
    if nranks == 1:
        rc = lib.eigx_init(int(device))
    else:
        import torch

        # the 128-byte session id (an ncclUniqueId when RCCL is installed) is made on rank 0 and broadcast over the
        # caller's process group; everything else -- the shared-memory board, the hipIpc window exchange, the RCCL
        # world / X / Y communicators -- happens inside eigx_init_multi
        group = None if comm is True else comm
        be = dist.get_backend(group)
        uid = (C.c_char * 128)()
        if rank == 0:
            _lib.check(lib.eigx_get_rccl_unique_id(uid), "eigx_get_rccl_unique_id")
        t = torch.tensor(list(bytes(uid)), dtype=torch.uint8)
        if be == "nccl":
            t = t.cuda(int(device))
        src = dist.get_global_rank(group, 0) if group is not None else 0
        dist.broadcast(t, src=src, group=group)
        raw = bytes(t.cpu().tolist())
        buf = C.create_string_buffer(raw, 128)
        rc = lib.eigx_init_multi(int(device), rank, nranks, buf, _char(order, "C"))
    _lib.check(rc, "eigen_init")
    _state["initialized"] = True
    _state["comm"] = comm
    return None


def eigen_comm_info():
    """transports chosen at eigen_init (per-step exchange, its wait, bulk collectives) and the init-time self-test's
    counts, as a dict (eigx_comm_info); {"ranks": 1} on one GPU"""
    import json

    lib = _lib.load()
    buf = C.create_string_buffer(2048)
    _lib.check(lib.eigx_comm_info(buf, 2048), "eigx_comm_info")
    return json.loads(buf.value.decode())


def eigen_free():
    lib = _lib.load()
    lib.eigx_free()
    _state["initialized"] = False


def eigen_get_matdims(n, m_forward=None, m_backward=None, mode="O"):
    """returns (nx, ny): extents of the local arrays a(nx,ny), z(nx,ny); (-1,-1) if too large."""
    lib = _lib.load()
    nx, ny = C.c_int(-1), C.c_int(-1)
    lib.eigx_get_matdims(int(n), C.byref(nx), C.byref(ny), int(m_forward or eigen_NB_f),
                         int(m_backward or eigen_NB_b), _char(mode, "O"))
    return nx.value, ny.value


def eigen_get_procs():
    lib = _lib.load()
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    _lib.check(lib.eigx_get_procs(C.byref(a), C.byref(b), C.byref(c)), "eigen_get_procs")
    return a.value, b.value, c.value


def eigen_get_id():
    lib = _lib.load()
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    _lib.check(lib.eigx_get_id(C.byref(a), C.byref(b), C.byref(c)), "eigen_get_id")
    return a.value, b.value, c.value


def eigen_get_version():
    lib = _lib.load()
    v = C.c_int()
    d = C.create_string_buffer(32)
    vc = C.create_string_buffer(32)
    lib.eigx_get_version(C.byref(v), d, vc)
    return v.value, d.value.decode(), vc.value.decode()


def eigen_get_errinfo():
    lib = _lib.load()
    v = C.c_int64()
    lib.eigx_get_errinfo(C.byref(v))
    return v.value


def eigen_memory_internal(n, lda, ldz, m1=None, m0=None):
    lib = _lib.load()
    return lib.eigx_memory_internal(int(n), int(lda), int(ldz), int(m1 or eigen_NB_f), int(m0 or eigen_NB_b))


def _grid_dim(grid):
    procs, xp, yp = eigen_get_procs()
    idn, xi, yi = eigen_get_id()
    g = str(grid)[:1].upper()
    if g == "X":
        return xp, xi
    if g == "Y":
        return yp, yi
    return procs, idn


def _index_helper(entry, i, grid):
    nnod, inod = _grid_dim(grid)
    return getattr(_lib.load(), entry)(int(i), nnod, inod)


# index helpers: (value, 'X'|'Y') like the reference (src/eigen_libs0.F:1744-2356); 1-based
def eigen_loop_start(istart, grid):
    return _index_helper("eigx_loop_start", istart, grid)


def eigen_loop_end(iend, grid):
    return _index_helper("eigx_loop_end", iend, grid)


def eigen_translate_l2g(ictr, grid):
    return _index_helper("eigx_translate_l2g", ictr, grid)


def eigen_translate_g2l(ictr, grid):
    return _index_helper("eigx_translate_g2l", ictr, grid)


def eigen_owner_node(ictr, grid):
    return _index_helper("eigx_owner_node", ictr, grid)


def eigen_owner_index(ictr, grid):
    return _index_helper("eigx_owner_index", ictr, grid)


# ---- the steps of a solver call: check the wrapper's own arguments, _begin, _addrs, the entry, _finish -----------------
# ``which`` names the family and with it the entry (eigx_<which>...), the name in the warnings and the dtype of a, b, z:
# float64 for 'sx', 's', 'gev', complex128 for 'h', 'hgev'; w is float64 everywhere.

_MIXED = "the arrays must all be host arrays or all be device tensors"


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _addr(x, name, dev, dtype, cplx):
    """address of the array argument ``x`` (None: null) of a host (``dev`` False) or a device call, after the checks of
    its dtype (``dtype``: 'float64' or 'complex128'), its side and, on the host, its order.  The real wrappers
    (``cplx`` False) judge a torch tensor by itself -- on the GPU, then its dtype -- before its side; the complex ones
    take a tensor that is not on the GPU for a host array."""
    if x is None:
        return None
    if _is_torch(x):
        import torch

        if not cplx and not x.is_cuda:
            raise ValueError(f"{name}: torch tensors must live on the GPU (use numpy for host arrays)")
        same_side = dev and x.is_cuda
        if cplx and not same_side:
            raise ValueError(_MIXED)
        if x.dtype != getattr(torch, dtype):
            raise ValueError(f"{name}: {dtype} required")
        if not same_side:
            raise ValueError(_MIXED)
        return x.data_ptr()
    if dev:
        raise ValueError(_MIXED)
    if x.dtype != getattr(np, dtype):
        raise ValueError(f"{name}: {dtype} required")
    if x.ndim == 2 and not x.flags.f_contiguous:
        raise ValueError(f"{name}: Fortran (column-major) order required, as in the reference")
    return x.ctypes.data


def _addrs(which, dev, **arrays):
    """addresses of the named array arguments of one call, checked in the order given"""
    cplx = which.startswith("h")
    return [_addr(x, name, dev, "complex128" if cplx and name != "w" else "float64", cplx) for name, x in arrays.items()]


def _begin(a):
    """(library, device flag) -- or None when eigen_init has not been called: the reference returns silently then
    (src/eigen_sx.F:82-86), here with status -1.  ``a`` decides the side of the call."""
    lib = _lib.load()
    if not _state["initialized"]:
        _state["last_status"] = -1
        return None
    dev = _is_torch(a)
    if dev:
        import torch

        torch.cuda.current_stream().synchronize()  # inputs written on torch's stream must be visible
    return lib, dev


def _entry(lib, name, dev):
    return getattr(lib, name + ("_dev" if dev else ""))


def _blocks(m_forward, m_backward):
    return eigen_NB_f if m_forward is None else int(m_forward), eigen_NB_b if m_backward is None else int(m_backward)


def _finish(name, rc, quiet=(0, -5)):
    _state["last_status"] = rc
    if rc not in quiet:
        print(f"Warning: {name} returned without computing (status {rc})", file=sys.stderr)


def _index_window(name, n, il, iu, z, mode):
    """checks of the index-range wrappers, made before the library is touched: the mode byte or None (status -2 =
    EIGX_ERR_BAD_ARG)"""
    md = _char(mode, "A").upper()
    try:
        ok = 1 <= int(il) <= int(iu) <= int(n) and md in (b"A", b"N") and not (md == b"A" and z is None)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        _state["last_status"] = -2
        print(f"Warning: {name}: invalid window / mode (n={n}, il={il}, iu={iu}, mode={mode!r})", file=sys.stderr)
        return None
    return md


def _value_window(name, n, vl, vu, w, z, mode, mmax):
    """checks of the value-window wrappers, made before the library is touched: (mode byte, mmax) or None (status -2)"""
    md = _char(mode, "A").upper()
    try:
        ok = int(n) > 0 and float(vl) < float(vu) and md in (b"A", b"N", b"C")   # a NaN bound fails the comparison
        if ok and md != b"C":
            if mmax is None:
                mmax = int(w.numel() if _is_torch(w) else w.size)
                if md == b"A" and z is not None and z.ndim == 2:
                    # columns of z: a torch tensor holds the column-major image, z[j, i] = Z(i, j)
                    mmax = min(mmax, int(z.shape[0] if _is_torch(z) else z.shape[1]))
            ok = int(mmax) >= 1 and w is not None and not (md == b"A" and z is None)
    except (TypeError, ValueError, AttributeError):
        ok = False
    if not ok:
        _state["last_status"] = -2
        print(f"Warning: {name}: invalid window / mode (n={n}, vl={vl}, vu={vu}, mmax={mmax}, mode={mode!r})", file=sys.stderr)
        return None
    return md, (0 if md == b"C" else int(mmax))


def _finish_value_call(name, rc, m, il, quiet):
    _finish(name, rc, quiet)
    return (m.value, il.value) if rc in (0, -9) else None


# ---- standard problem: 'sx', 's' (real symmetric), 'h' (complex Hermitian) --------------------------------------------
def _solve(which, n, nvec, a, lda, w, z, ldz, m_forward, m_backward, mode, nb=None):
    began = _begin(a)
    if began is None:
        return
    lib, dev = began
    pa, pw, pz = _addrs(which, dev, a=a, w=w, z=z)
    mf, mb = _blocks(m_forward, m_backward)
    if nb is None:
        rc = _entry(lib, f"eigx_{which}", dev)(int(n), int(nvec), pa, int(lda), pw, pz, int(ldz), mf, mb, _char(mode, "A"))
    else:
        rc = _entry(lib, "eigx_solve_bc", dev)(2 if which == "sx" else 1, int(n), int(nvec), pa, int(lda), pw, pz, int(ldz),
                                               int(nb), mf, mb, _char(mode, "A"))
    _finish(f"eigen_{which}", rc)


def eigen_sx(n, nvec, a, lda, w, z, ldz, m_forward=None, m_backward=None, mode="A"):
    """Pentadiagonal route (eigen_prd -> eigen_dcx -> trbakwy, src/eigen_sx.F:30-308)."""
    _solve("sx", n, nvec, a, lda, w, z, ldz, m_forward, m_backward, mode)


def eigen_s(n, nvec, a, lda, w, z, ldz, m_forward=None, m_backward=None, mode="A"):
    """Tridiagonal route (eigen_trd -> dc2 -> trbakwy, src/eigen_libs.F:150-202)."""
    _solve("s", n, nvec, a, lda, w, z, ldz, m_forward, m_backward, mode)


def eigen_h(n, nvec, a, lda, w, z, ldz, m_forward=None, m_backward=None, mode="A"):
    """Complex Hermitian solver (src/eigen_h.F:30-322: eigen_hrd -> dc2 -> eigen_hrbakwyx).  ``a``, ``z``: complex128,
    column-major (numpy, Fortran order) or GPU tensors holding the column-major image (``a[j, i] = A(i, j)``); upper
    triangle of ``a`` significant, ``a`` destroyed; ``w`` float64 ascending.  modes 'A', 'N', 'X'.  One GPU."""
    _solve("h", n, nvec, a, lda, w, z, ldz, m_forward, m_backward, mode)


def eigen_sx_bc(n, nvec, a, lda, w, z, ldz, nb, m_forward=None, m_backward=None, mode="A"):
    """eigen_sx on the local blocks of a 2-D block-cyclic (ScaLAPACK, MB = NB = nb) distribution over the process grid:
    no pdgemr2d redistribution into the cyclic layout is needed (manual 3.4).  ``z`` returns in the same distribution."""
    _solve("sx", n, nvec, a, lda, w, z, ldz, m_forward, m_backward, mode, nb=nb)


def eigen_s_bc(n, nvec, a, lda, w, z, ldz, nb, m_forward=None, m_backward=None, mode="A"):
    """eigen_s on block-cyclic local blocks (see eigen_sx_bc)."""
    _solve("s", n, nvec, a, lda, w, z, ldz, m_forward, m_backward, mode, nb=nb)


def numroc(n, nb, iproc, nprocs):
    """ScaLAPACK NUMROC with source process 0: local extent of n indices in blocks of nb on process iproc of nprocs"""
    return _lib.load().eigx_numroc(int(n), int(nb), int(iproc), int(nprocs))


def _solve_range(which, n, il, iu, a, lda, w, z, ldz, m_forward, m_backward, mode):
    name = f"eigen_{which}_range"
    md = _index_window(name, n, il, iu, z, mode)
    began = _begin(a) if md else None
    if began is None:
        return
    lib, dev = began
    pa, pw, pz = _addrs(which, dev, a=a, w=w, z=z)
    rc = _entry(lib, f"eigx_{which}_range", dev)(int(n), int(il), int(iu), pa, int(lda), pw, pz, int(ldz),
                                                 *_blocks(m_forward, m_backward), md)
    _finish(name, rc)


def eigen_sx_range(n, il, iu, a, lda, w, z, ldz, m_forward=None, m_backward=None, mode="A"):
    """EXTENSION (not in the reference): eigenpairs ``il .. iu`` (1-based, inclusive) of the ascending spectrum by the
    pentadiagonal route, one GPU.  ``w[:m]``, ``z[:, :m]`` with ``m = iu - il + 1``; modes 'A' and 'N'.  Work and memory
    after the reduction scale with ``m`` (Sturm multi-section on the window, inverse iteration, CholQR2 + Rayleigh-Ritz);
    ``range_info()`` tells whether that path or the full divide and conquer produced the result."""
    _solve_range("sx", n, il, iu, a, lda, w, z, ldz, m_forward, m_backward, mode)


def eigen_s_range(n, il, iu, a, lda, w, z, ldz, m_forward=None, m_backward=None, mode="A"):
    """EXTENSION: ``eigen_sx_range`` by the tridiagonal route."""
    _solve_range("s", n, il, iu, a, lda, w, z, ldz, m_forward, m_backward, mode)


def eigen_h_range(n, il, iu, a, lda, w, z, ldz, m_forward=None, m_backward=None, mode="A"):
    """EXTENSION (not in the reference): eigenpairs ``il .. iu`` (1-based, inclusive) of the ascending spectrum of a complex
    Hermitian matrix, one GPU.  Arrays as for ``eigen_h`` (``a``, ``z`` complex128, ``w`` float64); ``w[:m]``, ``z[:, :m]``
    with ``m = iu - il + 1``; modes 'A' and 'N' (``z`` may be None).  After eigen_h's reduction the work and the memory
    scale with ``m`` (multi-section on the window, inverse iteration, CholQR2 + Rayleigh-Ritz on the real tridiagonal
    matrix, back-transformation of ``m`` columns); ``range_info()`` tells whether that path or the full divide and conquer
    produced the result."""
    _solve_range("h", n, il, iu, a, lda, w, z, ldz, m_forward, m_backward, mode)


def _solve_range_v(which, n, vl, vu, a, lda, w, z, ldz, m_forward, m_backward, mode, mmax):
    name = f"eigen_{which}_range_v"
    chk = _value_window(name, n, vl, vu, w, z, mode, mmax)
    began = _begin(a) if chk else None
    if began is None:
        return None
    (md, mmax), (lib, dev) = chk, began
    pa, pw, pz = _addrs(which, dev, a=a, w=w, z=z)
    m, il = C.c_int(0), C.c_int(0)
    rc = _entry(lib, f"eigx_{which}_range_v", dev)(int(n), float(vl), float(vu), mmax, C.byref(m), C.byref(il), pa, int(lda),
                                                   pw, pz, int(ldz), *_blocks(m_forward, m_backward), md)
    return _finish_value_call(name, rc, m, il, (0, -5, -9))


def eigen_sx_range_v(n, vl, vu, a, lda, w, z, ldz, m_forward=None, m_backward=None, mode="A", mmax=None):
    """EXTENSION (not in the reference; LAPACK's range = 'V'): the eigenpairs with ``vl <= lambda < vu`` by the
    pentadiagonal route, one GPU.  Returns ``(m, il)``: ``m`` eigenvalues lie in the window, the first is number ``il``
    (1-based) of the ascending spectrum; ``w[:m]``, ``z[:, :m]`` as from ``eigen_sx_range(n, il, il + m - 1, ...)``, bit for
    bit.  The interval is half-open; an eigenvalue within rounding of an end point may fall on either side, as in LAPACK;
    ``-inf`` / ``inf`` are allowed.  ``mmax`` = room in ``w`` / ``z`` (default: the entries of ``w``, further limited by the
    columns of a 2-D ``z``): with ``m > mmax`` the status is -9, ``w`` and ``z`` are untouched and ``(m, il)`` is returned
    for a retry by index; ``m = 0`` is status 0 with ``w``, ``z`` untouched.  Modes 'A', 'N' (``z`` may be None) and 'C'
    (count only: ``w``, ``z`` may be None).  Returns None when nothing was resolved (any other status)."""
    return _solve_range_v("sx", n, vl, vu, a, lda, w, z, ldz, m_forward, m_backward, mode, mmax)


def eigen_s_range_v(n, vl, vu, a, lda, w, z, ldz, m_forward=None, m_backward=None, mode="A", mmax=None):
    """EXTENSION: ``eigen_sx_range_v`` by the tridiagonal route."""
    return _solve_range_v("s", n, vl, vu, a, lda, w, z, ldz, m_forward, m_backward, mode, mmax)


def eigen_h_range_v(n, vl, vu, a, lda, w, z, ldz, m_forward=None, m_backward=None, mode="A", mmax=None):
    """EXTENSION (not in the reference; LAPACK's range = 'V'): the eigenpairs of a complex Hermitian matrix with
    ``vl <= lambda < vu``, one GPU, at the cost of ONE reduction.  Arrays as for ``eigen_h``; window, ``mmax``, modes
    ('A', 'N', 'C'), statuses and the returned ``(m, il)`` as for ``eigen_sx_range_v``; ``w[:m]``, ``z[:, :m]`` as from
    ``eigen_h_range(n, il, il + m - 1, ...)``, bit for bit.  Returns None when nothing was resolved."""
    return _solve_range_v("h", n, vl, vu, a, lda, w, z, ldz, m_forward, m_backward, mode, mmax)


def _info_addr(info, dev, names):
    """address of the per-matrix status array of a batch call (None: null): int32, on the side of the other arrays"""
    if info is None:
        return None
    if dev != _is_torch(info):
        raise ValueError(f"{names} must all be host arrays or all be device tensors")
    if dev:
        import torch

        if not info.is_cuda or info.dtype != torch.int32:
            raise ValueError("info: int32 GPU tensor required")
    elif info.dtype != np.int32:
        raise ValueError("info: int32 required")
    return info.data_ptr() if dev else info.ctypes.data


def _solve_batch(which, n, batch, a, lda, w, z, ldz, mode, info, stride_a, ldw, stride_z, window=None, pencil=None):
    """the uniform-batch wrappers; window = (il, iu) for eigen_s_batch_range / eigen_h_batch_range / eigen_gev_batch_range / eigen_hgev_batch_range (z has m = iu - il + 1 columns and w has m entries per
    matrix, otherwise n), pencil = (b, ldb, stride_b) for the generalised families"""
    name = f"eigen_{which}_batch" + ("_range" if window else "")
    has_b = pencil is not None
    il, iu = window or (None, None)
    b, ldb, stride_b = pencil or (None, None, None)
    # the arguments are checked here, before the library is touched (status -2 = EIGX_ERR_BAD_ARG)
    md = _char(mode, "A").upper()
    try:
        n, batch, il, iu, lda, ldb = (int(x) if used else None for x, used in (
            (n, True), (batch, True), (il, window), (iu, window), (lda, True), (ldb, has_b)))   # (all of them, or none)
        m = iu - il + 1 if window else n
        ldw = m if ldw is None else int(ldw)
        ldz = int(ldz) if md == b"A" else (0 if ldz is None else int(ldz))
        stride_a = lda * n if stride_a is None else int(stride_a)
        if has_b:
            stride_b = ldb * n if stride_b is None else int(stride_b)
        stride_z = ldz * m if stride_z is None else int(stride_z)
        ok = n >= 1 and batch >= 0 and lda >= n and ldw >= m and md in (b"A", b"N") and a is not None and w is not None
        ok = ok and (not window or 1 <= il <= iu <= n) and (batch <= 1 or stride_a >= lda * n)
        ok = ok and (not has_b or (ldb >= n and b is not None and (batch <= 1 or stride_b >= ldb * n)))
        if md == b"A":
            ok = ok and z is not None and ldz >= n and (batch <= 1 or stride_z >= ldz * m)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        _state["last_status"] = -2
        shown = [("n", n), ("batch", batch)] + ([("il", il), ("iu", iu)] if window else []) + [("lda", lda)]
        shown += ([("ldb", ldb)] if has_b else []) + [("ldw", ldw), ("ldz", ldz), ("stride_a", stride_a)]
        shown += ([("stride_b", stride_b)] if has_b else []) + [("stride_z", stride_z)]
        print(f"Warning: {name}: invalid arguments ({', '.join(f'{key}={v}' for key, v in shown)}, mode={mode!r})", file=sys.stderr)
        return
    began = _begin(a)
    if began is None:
        return
    lib, dev = began
    if md != b"A":
        z = None
    arrays = dict(a=a, **(dict(b=b) if has_b else {}), w=w, z=z)
    for xname, x in arrays.items():
        if x is not None and not dev and not _is_torch(x) and x.ndim > 2 and not x.flags.f_contiguous:
            raise ValueError(f"{xname}: Fortran (column-major) order required, as in the reference")
    p = dict(zip(arrays, _addrs(which, dev, **arrays)))
    pi = _info_addr(info, dev, f"{', '.join(arrays)}, info")
    args = (n, batch) + ((il, iu) if window else ()) + (p["a"], lda, stride_a) + ((p["b"], ldb, stride_b) if has_b else ())
    rc = _entry(lib, name.replace("eigen_", "eigx_"), dev)(*args, p["w"], ldw, p["z"], ldz, stride_z, md, pi)
    _finish(name, rc, (0, -5, -6, -7) if has_b else (0, -5, -6))


def eigen_s_batch(n, batch, a, lda, w, z, ldz, mode="A", info=None, stride_a=None, ldw=None, stride_z=None):
    """EXTENSION (not in the reference): ``batch`` symmetric matrices of one size ``n`` in one call, one GPU.  ``a`` holds the
    matrices as ``a[lda, n, batch]`` (numpy, Fortran order) or a GPU tensor with the same memory image: matrix ``k`` starts at
    element ``k * stride_a``, upper triangle significant, destroyed.  ``w[ldw, batch]`` receives the ascending eigenvalues,
    ``z[ldz, n, batch]`` the eigenvectors (mode 'A'; mode 'N': eigenvalues only, ``z`` may be None).  Defaults:
    ``stride_a = lda * n``, ``stride_z = ldz * n``, ``ldw = n``.  ``info`` (optional, int32, ``batch`` entries, on the side of
    ``a``) receives the per-matrix status: 0, -5 (NaN / Inf in the matrix: its ``w`` is NaN, its ``z`` untouched) or -6;
    ``last_status()`` is 0 or the status of the first failed matrix.  For ``n <= 128`` one kernel launch solves the batch,
    one workgroup per matrix with the matrix in LDS; larger ``n`` runs ``eigen_s`` matrix by matrix."""
    _solve_batch("s", n, batch, a, lda, w, z, ldz, mode, info, stride_a, ldw, stride_z)


def eigen_h_batch(n, batch, a, lda, w, z, ldz, mode="A", info=None, stride_a=None, ldw=None, stride_z=None):
    """EXTENSION (not in the reference): ``batch`` complex Hermitian matrices of one size ``n`` in one call, one GPU -- the
    complex sibling of ``eigen_s_batch``.  ``a`` holds the matrices as ``a[lda, n, batch]`` (complex128 numpy, Fortran order)
    or a complex128 GPU tensor with the same memory image: matrix ``k`` starts at complex element ``k * stride_a``, upper
    triangle significant (of the diagonal the real parts only), destroyed.  ``w[ldw, batch]`` (float64) receives the ascending
    eigenvalues, ``z[ldz, n, batch]`` (complex128) the orthonormal eigenvectors (mode 'A'; mode 'N': eigenvalues only, ``z``
    may be None).  Defaults, ``info`` and ``last_status()`` as for ``eigen_s_batch``; leading dimensions and strides count
    complex elements.  For ``n <= 96`` one kernel launch solves the batch, one workgroup per matrix with the matrix in LDS;
    larger ``n`` runs ``eigen_h`` matrix by matrix."""
    _solve_batch("h", n, batch, a, lda, w, z, ldz, mode, info, stride_a, ldw, stride_z)


def eigen_s_batch_range(n, batch, il, iu, a, lda, w, z, ldz, mode="A", info=None, stride_a=None, ldw=None, stride_z=None):
    """EXTENSION (not in the reference): eigenpairs ``il .. iu`` (1-based, inclusive, the same window for every matrix) of
    ``batch`` symmetric matrices of one size ``n`` in one call, one GPU.  ``a`` as for ``eigen_s_batch``.  With
    ``m = iu - il + 1``: ``w[ldw, batch]`` receives ``w[:m, k]``, ascending; ``z[ldz, m, batch]`` the eigenvectors
    ``z[:n, :m, k]`` (mode 'A'; mode 'N': eigenvalues only, ``z`` may be None).  Defaults: ``stride_a = lda * n``,
    ``stride_z = ldz * m``, ``ldw = m``.  ``info`` and ``last_status()`` as for ``eigen_s_batch``.  For ``n <= 128`` either a
    window kernel (tridiagonalisation, Sturm-count bisection, inverse iteration and Rayleigh-Ritz in LDS, no QL sweep) or the
    kernel of ``eigen_s_batch`` with a slice solves the batch, by a measured rule (``eigx_tune`` key 26);
    ``batch_range_info()`` tells which.  Larger ``n`` runs ``eigen_s_range`` matrix by matrix."""
    _solve_batch("s", n, batch, a, lda, w, z, ldz, mode, info, stride_a, ldw, stride_z, window=(il, iu))


def eigen_h_batch_range(n, batch, il, iu, a, lda, w, z, ldz, mode="A", info=None, stride_a=None, ldw=None, stride_z=None):
    """EXTENSION (not in the reference): eigenpairs ``il .. iu`` (1-based, inclusive, the same window for every matrix) of
    ``batch`` complex Hermitian matrices of one size ``n`` in one call, one GPU -- the complex sibling of
    ``eigen_s_batch_range``.  ``a`` as for ``eigen_h_batch`` (complex128; leading dimensions and strides count complex
    elements).  With ``m = iu - il + 1``: ``w[ldw, batch]`` (float64) receives ``w[:m, k]``, ascending; ``z[ldz, m, batch]``
    (complex128) the orthonormal eigenvectors ``z[:n, :m, k]`` (mode 'A'; mode 'N': eigenvalues only, ``z`` may be None).
    Defaults: ``stride_a = lda * n``, ``stride_z = ldz * m``, ``ldw = m``.  ``info`` and ``last_status()`` as for
    ``eigen_s_batch``.  For ``n <= 96`` either a window kernel (Hermitian tridiagonalisation, then Sturm-count bisection,
    inverse iteration and Rayleigh-Ritz on the real tridiagonal matrix, all in LDS; mode 'A' for ``m <= 16`` and ``n <= 64``)
    or the kernel of ``eigen_h_batch`` with a slice solves the batch, by a measured rule (``eigx_tune`` key 26);
    ``batch_range_info()`` tells which.  Larger ``n`` runs ``eigen_h_range`` matrix by matrix."""
    _solve_batch("h", n, batch, a, lda, w, z, ldz, mode, info, stride_a, ldw, stride_z, window=(il, iu))


def eigen_gev_batch_range(n, batch, il, iu, a, lda, b, ldb, w, z, ldz, mode="A", info=None, stride_a=None, stride_b=None, ldw=None,
                          stride_z=None):
    """EXTENSION (not in the reference): eigenpairs ``il .. iu`` (1-based, inclusive, the same window for every pencil) of
    ``batch`` symmetric-definite pencils ``A x = lambda B x`` of one size ``n`` in one call, one GPU -- the pencil sibling of
    ``eigen_s_batch_range``.  ``a`` and ``b`` as for ``eigen_gev_batch``: upper triangles significant, ``a`` destroyed, ``b``
    returns ``U`` with ``B = U^T U`` in its upper triangle for every pencil that succeeded (bit for bit the ``U`` of
    ``eigen_gev_batch``; a failed pencil keeps its ``b``).  With ``m = iu - il + 1``: ``w[ldw, batch]`` receives ``w[:m, k]``,
    ascending; ``z[ldz, m, batch]`` the eigenvectors ``z[:n, :m, k]`` with ``z^T B z = I`` (mode 'A'; mode 'N': eigenvalues
    only, ``z`` may be None).  Defaults: ``stride_a = lda * n``, ``stride_b = ldb * n``, ``stride_z = ldz * m``, ``ldw = m``.
    ``info`` and ``last_status()`` as for ``eigen_gev_batch`` (0, -5, -6 or -7 per pencil).  For ``n <= 96`` either a window
    kernel (Cholesky, ``C = U^-T A U^-1``, tridiagonalisation, Sturm-count bisection, inverse iteration, Rayleigh-Ritz and
    ``Z = U^-1 V`` in LDS; mode 'A' for ``m <= 16`` and ``n <= 64``) or the kernel of ``eigen_gev_batch`` with a slice solves
    the batch, by a measured rule (``eigx_tune`` key 26); ``batch_range_info()`` tells which.  Larger ``n`` runs
    ``eigen_gev_range`` pencil by pencil."""
    _solve_batch("gev", n, batch, a, lda, w, z, ldz, mode, info, stride_a, ldw, stride_z, window=(il, iu), pencil=(b, ldb, stride_b))


def eigen_hgev_batch_range(n, batch, il, iu, a, lda, b, ldb, w, z, ldz, mode="A", info=None, stride_a=None, stride_b=None, ldw=None,
                           stride_z=None):
    """EXTENSION (not in the reference): eigenpairs ``il .. iu`` (1-based, inclusive, the same window for every pencil) of
    ``batch`` Hermitian-definite pencils ``A x = lambda B x`` of one size ``n`` in one call, one GPU -- the complex sibling of
    ``eigen_gev_batch_range``.  ``a`` and ``b`` as for ``eigen_hgev_batch`` (complex128; leading dimensions and strides count
    complex elements): upper triangles significant (of the diagonals the real parts), ``a`` destroyed, ``b`` returns ``U`` with
    ``B = U^H U`` and a real positive diagonal in its upper triangle for every pencil that succeeded (bit for bit the ``U`` of
    ``eigen_hgev_batch``; a failed pencil keeps its ``b``).  With ``m = iu - il + 1``: ``w[ldw, batch]`` (float64) receives
    ``w[:m, k]``, ascending; ``z[ldz, m, batch]`` (complex128) the eigenvectors ``z[:n, :m, k]`` with ``z^H B z = I`` (mode 'A';
    mode 'N': eigenvalues only, ``z`` may be None).  Defaults: ``stride_a = lda * n``, ``stride_b = ldb * n``,
    ``stride_z = ldz * m``, ``ldw = m``.  ``info`` and ``last_status()`` as for ``eigen_hgev_batch`` (0, -5, -6 or -7 per
    pencil).  For ``n <= 64`` either a window kernel (complex Cholesky, ``C = U^-H A U^-1``, Hermitian tridiagonalisation,
    Sturm-count bisection, inverse iteration, Rayleigh-Ritz and ``Z = U^-1 V`` in LDS; mode 'A' for ``m <= 16`` at ``n <= 32``
    and for ``m <= 8`` at ``33 <= n <= 64``, mode 'N' for any ``m``) or the kernel of ``eigen_hgev_batch`` with a slice solves
    the batch, by a measured rule (``eigx_tune`` key 26); ``batch_range_info()`` tells which.  Larger ``n`` runs
    ``KMATH_EIGEN_HGEV_RANGE`` pencil by pencil."""
    _solve_batch("hgev", n, batch, a, lda, w, z, ldz, mode, info, stride_a, ldw, stride_z, window=(il, iu), pencil=(b, ldb, stride_b))


def batch_range_info():
    """What the last ``eigen_s_batch_range``, ``eigen_h_batch_range``, ``eigen_gev_batch_range`` or ``eigen_hgev_batch_range``
    call did: ``route`` (1 the window kernel, 2 the full batch solve and a slice, 3 ``eigen_s_range`` / ``eigen_h_range`` /
    ``eigen_gev_range`` / ``KMATH_EIGEN_HGEV_RANGE`` matrix by matrix above the cutoff), ``m`` and ``redone`` (how many matrices
    the acceptance test of the window kernel sent to route 2)."""
    import collections

    lib = _lib.load()
    r, m, d = C.c_int(), C.c_int(), C.c_int()
    _lib.check(lib.eigx_batch_range_info(C.byref(r), C.byref(m), C.byref(d)), "eigx_batch_range_info")
    return collections.namedtuple("BatchRangeInfo", "route m redone")(r.value, m.value, d.value)


def _solve_vbatch(which, batch, n, a, off_a, lda, w, off_w, z, off_z, ldz, mode, info, pencil=None):
    """the ragged wrappers; pencil = (b, off_b, ldb) for the generalised families, which need all three in both modes"""
    name = f"eigen_{which}_vbatch"
    # the arguments are checked here, before the library is touched (status -2 = EIGX_ERR_BAD_ARG)
    md = _char(mode, "A").upper()
    want_vec = md == b"A"
    has_b = pencil is not None
    b, off_b, ldb = pencil if has_b else (None, None, None)
    desc = {}
    try:
        batch = int(batch)
        ok = batch >= 0 and md in (b"A", b"N") and (batch == 0 or (a is not None and w is not None))
        ok = ok and not (want_vec and batch > 0 and z is None) and not (has_b and batch > 0 and b is None)
        for key, x, dtype, needed in (("n", n, np.int32, True), ("off_a", off_a, np.int64, True), ("lda", lda, np.int32, True),
                                      ("off_b", off_b, np.int64, has_b), ("ldb", ldb, np.int32, has_b),
                                      ("off_w", off_w, np.int64, True), ("off_z", off_z, np.int64, want_vec),
                                      ("ldz", ldz, np.int32, want_vec)):
            if not ok:
                break
            if x is None or not needed:
                desc[key] = None
                ok = not needed or batch == 0
                continue
            v = np.asarray(x)
            ok = v.ndim == 1 and v.size == batch and (batch == 0 or v.dtype.kind in "iu")
            if ok:
                ok = batch == 0 or bool((v >= 0).all() and (v <= np.iinfo(dtype).max).all())
                desc[key] = np.ascontiguousarray(v, dtype=dtype)
        if ok and batch > 0:
            ok = bool((desc["lda"] >= desc["n"]).all()) and (not want_vec or bool((desc["ldz"] >= desc["n"]).all()))
            ok = ok and (not has_b or bool((desc["ldb"] >= desc["n"]).all()))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        _state["last_status"] = -2
        print(f"Warning: {name}: invalid arguments (batch={batch}, mode={mode!r}; n >= 0, lda >= n, {'ldb >= n, ' if has_b else ''}"
              f"offsets >= 0 and in mode 'A' "
              f"ldz >= n are required of every block, with {batch} entries per descriptor)", file=sys.stderr)
        return
    began = _begin(a)
    if began is None:
        return
    lib, dev = began
    if not want_vec:
        z = None
    pd = {key: (None if v is None else v.ctypes.data) for key, v in desc.items()}
    arrays = dict(a=a, **(dict(b=b) if has_b else {}), w=w, z=z)
    p = dict(zip(arrays, _addrs(which, dev, **arrays)))
    pi = _info_addr(info, dev, f"{', '.join(arrays)}, info")
    args = (batch, pd["n"], p["a"], pd["off_a"], pd["lda"]) + ((p["b"], pd["off_b"], pd["ldb"]) if has_b else ())
    rc = _entry(lib, f"eigx_{which}_vbatch", dev)(*args, p["w"], pd["off_w"], p["z"], pd["off_z"], pd["ldz"], md, pi)
    _finish(name, rc, (0, -5, -6, -7) if has_b else (0, -5, -6))


def eigen_s_vbatch(batch, n, a, off_a, lda, w, off_w, z, off_z, ldz, mode="A", info=None):
    """EXTENSION (not in the reference): ``batch`` symmetric matrices of differing orders in one call, one GPU -- the ragged
    sibling of ``eigen_s_batch``.  ``a``, ``w`` and ``z`` are flat arrays (numpy float64, host form) or GPU tensors (device form);
    ``n``, ``off_a``, ``lda``, ``off_w``, ``off_z``, ``ldz`` are integer sequences of ``batch`` entries, always on the host:
    block ``k`` of order ``n[k]`` starts at element ``off_a[k]`` of ``a``, column-major with the leading dimension ``lda[k]``,
    upper triangle significant, destroyed; its ascending eigenvalues go to ``w[off_w[k]:off_w[k] + n[k]]``, its eigenvectors to
    ``z`` from ``off_z[k]`` on with the leading dimension ``ldz[k]`` (mode 'A'; mode 'N': eigenvalues only, ``z``, ``off_z`` and
    ``ldz`` may be None).  ``layout.ragged_offsets`` packs a list of blocks.  Blocks must not overlap (not checked); ``n[k] = 0``
    is an empty block.  Nothing outside ``w(1:n_k)`` and ``z(1:n_k, 1:n_k)`` is written.  ``info`` (optional, int32, ``batch``
    entries, on the side of ``a``) receives the per-block status: 0, -5 (NaN / Inf in the block: its ``w`` is NaN, its ``z``
    untouched) or -6; ``last_status()`` is 0 or the status of the failed block with the lowest index.  Blocks with ``n <= 128``
    are solved by one kernel launch per size class, bit for bit as ``eigen_s_batch`` solves them; larger ones by ``eigen_s``."""
    _solve_vbatch("s", batch, n, a, off_a, lda, w, off_w, z, off_z, ldz, mode, info)


def eigen_h_vbatch(batch, n, a, off_a, lda, w, off_w, z, off_z, ldz, mode="A", info=None):
    """EXTENSION (not in the reference): ``batch`` complex Hermitian matrices of differing orders in one call, one GPU -- the
    ragged sibling of ``eigen_h_batch``, the arguments of ``eigen_s_vbatch``: ``a`` and ``z`` flat complex128 (numpy or GPU
    tensors), ``w`` float64; ``off_a``, ``lda``, ``off_z`` and ``ldz`` count complex elements, ``off_w`` doubles.  Of a block's
    diagonal only the real parts are read.  Blocks with ``n <= 96`` are solved by one kernel launch per size class, bit for bit
    as ``eigen_h_batch`` solves them; larger ones by ``eigen_h``."""
    _solve_vbatch("h", batch, n, a, off_a, lda, w, off_w, z, off_z, ldz, mode, info)


def eigen_gev_batch(n, batch, a, lda, b, ldb, w, z, ldz, mode="A", info=None, stride_a=None, stride_b=None, ldw=None, stride_z=None):
    """EXTENSION (not in the reference): ``batch`` symmetric-definite pencils ``A x = lambda B x`` of one size ``n`` in one call,
    one GPU.  ``a[lda, n, batch]`` and ``b[ldb, n, batch]`` (numpy, Fortran order, or GPU tensors with the same memory image:
    pencil ``k`` starts at elements ``k * stride_a`` / ``k * stride_b``) hold the upper triangles; ``a`` is destroyed, ``b``
    comes back with ``U`` (``B = U^T U``) in its upper triangle.  ``w[ldw, batch]`` receives the ascending eigenvalues,
    ``z[ldz, n, batch]`` the eigenvectors with ``z^T B z = I`` (mode 'A'; mode 'N': eigenvalues and ``U`` only, ``z`` may be
    None).  Defaults: ``stride_a = lda * n``, ``stride_b = ldb * n``, ``stride_z = ldz * n``, ``ldw = n``.  ``info`` (optional,
    int32, ``batch`` entries, on the side of ``a``) receives the per-pencil status: 0, -5 (NaN / Inf in A or B: its ``w`` is
    NaN, its ``z`` and ``b`` untouched), -7 (B not positive definite: ``w`` NaN, ``z`` untouched) or -6; ``last_status()`` is 0
    or the status of the first failed pencil.  For ``n <= 96`` one kernel launch solves the batch, one workgroup per pencil
    with both matrices in LDS; larger ``n`` runs ``KMATH_EIGEN_GEV_RANGE`` with ``il = 1, iu = n`` pencil by pencil."""
    _solve_batch("gev", n, batch, a, lda, w, z, ldz, mode, info, stride_a, ldw, stride_z, pencil=(b, ldb, stride_b))


def eigen_hgev_batch(n, batch, a, lda, b, ldb, w, z, ldz, mode="A", info=None, stride_a=None, stride_b=None, ldw=None, stride_z=None):
    """EXTENSION (not in the reference): ``batch`` Hermitian-definite pencils ``A x = lambda B x`` of one size ``n`` in one
    call, one GPU -- ``eigen_gev_batch`` over complex numbers, on the storage of ``eigen_h_batch``.  ``a[lda, n, batch]`` and
    ``b[ldb, n, batch]`` (complex128 numpy, Fortran order, or complex128 GPU tensors with the same memory image: pencil ``k``
    starts at complex elements ``k * stride_a`` / ``k * stride_b``) hold the upper triangles (of the diagonals the real parts
    only); ``a`` is destroyed, ``b`` comes back with ``U`` (``B = U^H U``, real positive diagonal) in its upper triangle.
    ``w[ldw, batch]`` (float64) receives the ascending eigenvalues, ``z[ldz, n, batch]`` (complex128) the eigenvectors with
    ``z^H B z = I`` (mode 'A'; mode 'N': eigenvalues and ``U`` only, ``z`` may be None).  Defaults, ``info`` and
    ``last_status()`` as for ``eigen_gev_batch``; leading dimensions and strides count complex elements.  For ``n <= 64`` one
    kernel launch solves the batch, one workgroup per pencil with both matrices in LDS; larger ``n`` runs
    ``KMATH_EIGEN_HGEV_RANGE`` with ``il = 1, iu = n`` pencil by pencil."""
    _solve_batch("hgev", n, batch, a, lda, w, z, ldz, mode, info, stride_a, ldw, stride_z, pencil=(b, ldb, stride_b))


def eigen_gev_vbatch(batch, n, a, off_a, lda, b, off_b, ldb, w, off_w, z, off_z, ldz, mode="A", info=None):
    """EXTENSION (not in the reference): ``batch`` symmetric-definite pencils ``A x = lambda B x`` of differing orders in one
    call, one GPU -- the ragged sibling of ``eigen_gev_batch``, in the storage of ``eigen_s_vbatch`` with ``b``, ``off_b`` and
    ``ldb`` added.  ``a``, ``b``, ``w`` and ``z`` are flat arrays (numpy float64, host form) or GPU tensors (device form);
    ``n``, ``off_a``, ``lda``, ``off_b``, ``ldb``, ``off_w``, ``off_z``, ``ldz`` are integer sequences of ``batch`` entries,
    always on the host: pencil ``k`` of order ``n[k]`` starts at elements ``off_a[k]`` of ``a`` and ``off_b[k]`` of ``b``,
    column-major with the leading dimensions ``lda[k]`` and ``ldb[k]``, upper triangles significant; ``a`` is destroyed, the block
    of ``b`` comes back with ``U`` (``B = U^T U``) in its upper triangle.  The ascending eigenvalues go to
    ``w[off_w[k]:off_w[k] + n[k]]``, the eigenvectors with ``z^T B z = I`` to ``z`` from ``off_z[k]`` on with the leading
    dimension ``ldz[k]`` (mode 'A'; mode 'N': eigenvalues and ``U`` only, ``z``, ``off_z`` and ``ldz`` may be None; ``b``,
    ``off_b`` and ``ldb`` are needed in both modes).  Packing a list of pencils with ``layout.ragged_offsets``::

        n = [A.shape[0] for A in As]
        off, total = layout.ragged_offsets(n)                    # tight blocks: lda = ldb = ldz = n[k]
        off_w, len_w = layout.ragged_offsets(n, ld=1)
        a = np.concatenate([A.T.reshape(-1) for A in As])        # column-major
        b = np.concatenate([B.T.reshape(-1) for B in Bs])
        w, z = np.empty(len_w), np.empty(total)
        eigen_gev_vbatch(len(n), n, a, off, n, b, off, n, w, off_w, z, off, n)

    Blocks must not overlap (not checked); ``n[k] = 0`` is an empty block.  ``info`` (optional, int32, ``batch`` entries, on the
    side of ``a``) receives the per-block status: 0, -5 (NaN / Inf in A or B: its ``w`` is NaN, its ``z`` and ``b`` untouched),
    -7 (B not positive definite: ``w`` NaN, ``z`` untouched) or -6; ``last_status()`` is 0 or the status of the failed block
    with the lowest index.  Blocks with ``n <= 96`` are solved by one kernel launch per size class, bit for bit as
    ``eigen_gev_batch`` solves them; larger ones by ``KMATH_EIGEN_GEV_RANGE`` with ``il = 1, iu = n``."""
    _solve_vbatch("gev", batch, n, a, off_a, lda, w, off_w, z, off_z, ldz, mode, info, pencil=(b, off_b, ldb))


def eigen_hgev_vbatch(batch, n, a, off_a, lda, b, off_b, ldb, w, off_w, z, off_z, ldz, mode="A", info=None):
    """EXTENSION (not in the reference): ``batch`` Hermitian-definite pencils of differing orders in one call, one GPU -- the
    ragged sibling of ``eigen_hgev_batch``, the arguments of ``eigen_gev_vbatch`` (packed in the same way with
    ``layout.ragged_offsets``): ``a``, ``b`` and ``z`` flat complex128 (numpy or GPU tensors), ``w`` float64; ``off_a``,
    ``lda``, ``off_b``, ``ldb``, ``off_z`` and ``ldz`` count complex elements, ``off_w`` doubles.  Of the diagonals only the real
    parts are read; ``U`` (``B = U^H U``) comes back with a real positive diagonal, ``z^H B z = I``.  Blocks with ``n <= 64`` are
    solved by one kernel launch per size class, bit for bit as ``eigen_hgev_batch`` solves them; larger ones by
    ``KMATH_EIGEN_HGEV_RANGE`` with ``il = 1, iu = n``."""
    _solve_vbatch("hgev", batch, n, a, off_a, lda, w, off_w, z, off_z, ldz, mode, info, pencil=(b, off_b, ldb))


def band_count(d, e, band, x):
    """EXTENSION, stage entry: ``cnt[p]`` = number of eigenvalues of the symmetric band matrix below ``x[p]``.  ``d`` (n),
    ``e`` (shape (2, lde) or flat with 2 lde entries, lde >= n, as ``eigx_band_reduce_dev`` writes it for either band) and
    ``x`` are float64 torch tensors on the GPU; returns an int32 tensor of ``x.numel()`` counts (-1 for a NaN point)."""
    import torch

    lib = _lib.load()
    n = int(d.numel())
    lde = int(e.shape[-1]) if e.ndim == 2 else int(e.numel()) // 2
    for t, name in ((d, "d"), (e, "e"), (x, "x")):
        if not (_is_torch(t) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
            raise ValueError(f"{name}: contiguous float64 GPU tensor required")
    if lde < n:
        raise ValueError("e: two rows of at least n entries required")
    cnt = torch.empty(x.numel(), dtype=torch.int32, device=x.device)
    torch.cuda.current_stream().synchronize()
    _lib.check(lib.eigx_band_count_dev(n, d.data_ptr(), e.data_ptr(), lde, int(band), int(x.numel()), x.data_ptr(),
                                       cnt.data_ptr()), "eigx_band_count_dev")
    return cnt.reshape(x.shape)


def range_info():
    """What the last range call did: ``path`` (1 subset path, 2 fell back to the full divide and conquer, 3 full divide
    and conquer by the size rule), ``m`` and ``cond`` (the conditioning estimate of the acceptance test)."""
    import collections

    lib = _lib.load()
    p, m, c = C.c_int(), C.c_int(), C.c_double()
    _lib.check(lib.eigx_range_info(C.byref(p), C.byref(m), C.byref(c)), "eigx_range_info")
    return collections.namedtuple("RangeInfo", "path m cond")(p.value, m.value, c.value)


# ---- generalised problem A x = lambda B x: 'gev' (real symmetric-definite), 'hgev' (complex Hermitian-definite) -------
def _gev(which, quiet, n, a, lda, b, ldb, w, z, ldz):
    began = _begin(a)
    if began is None:
        return
    lib, dev = began
    pa, pb, pw, pz = _addrs(which, dev, a=a, b=b, w=w, z=z)
    rc = _entry(lib, f"eigx_{which}", dev)(int(n), pa, int(lda), pb, int(ldb), pw, pz, int(ldz))
    _finish(f"KMATH_EIGEN_{which.upper()}", rc, quiet)


def _gev_range(which, n, il, iu, a, lda, b, ldb, w, z, ldz, mode):
    name = f"KMATH_EIGEN_{which.upper()}_RANGE"
    md = _index_window(name, n, il, iu, z, mode)
    began = _begin(a) if md else None
    if began is None:
        return
    lib, dev = began
    pa, pb, pw, pz = _addrs(which, dev, a=a, b=b, w=w, z=z)
    rc = _entry(lib, f"eigx_{which}_range", dev)(int(n), int(il), int(iu), pa, int(lda), pb, int(ldb), pw, pz, int(ldz), md)
    _finish(name, rc, (0, -5, -7))


def _gev_range_v(which, n, vl, vu, a, lda, b, ldb, w, z, ldz, mode, mmax):
    name = f"KMATH_EIGEN_{which.upper()}_RANGE_V"
    chk = _value_window(name, n, vl, vu, w, z, mode, mmax)
    began = _begin(a) if chk else None
    if began is None:
        return None
    (md, mmax), (lib, dev) = chk, began
    pa, pb, pw, pz = _addrs(which, dev, a=a, b=b, w=w, z=z)
    m, il = C.c_int(0), C.c_int(0)
    rc = _entry(lib, f"eigx_{which}_range_v", dev)(int(n), float(vl), float(vu), mmax, C.byref(m), C.byref(il), pa, int(lda),
                                                   pb, int(ldb), pw, pz, int(ldz), md)
    return _finish_value_call(name, rc, m, il, (0, -5, -7, -9))


def KMATH_EIGEN_GEV(n, a, lda, b, ldb, w, z, ldz):
    """Generalised symmetric-definite problem A x = lambda B x (src/KMATH_EIGEN_GEV.F:1-64): two eigen_s solves and
    three GEMMs.  Upper triangles of ``a``, ``b`` significant; ``w`` ascending, ``z`` B-orthonormal; ``a`` and ``b``
    are destroyed.  If B is not positive definite a message is printed and the call returns (status -7)."""
    _gev("gev", (0, -7), n, a, lda, b, ldb, w, z, ldz)


def KMATH_EIGEN_GEV_RANGE(n, il, iu, a, lda, b, ldb, w, z, ldz, mode="A"):
    """EXTENSION, not in the reference: eigenpairs ``il .. iu`` (1-based, inclusive) of A x = lambda B x by the Cholesky
    route (B = U^T U, C = U^-T A U^-1, ``eigen_sx_range`` of C, Z = U^-1 Y), one GPU.  ``w[:m]`` ascending, ``z[:, :m]``
    with ``z^T B z = I``, ``m = iu - il + 1``; modes 'A' and 'N' (``z`` may be None).  Upper triangles of ``a``, ``b``
    significant; ``a`` is destroyed, ``b`` holds U in its upper triangle.  Status -7 if B is not positive definite, -5
    (``w[:m]`` = NaN) for a non-finite entry of either triangle.  ``range_info()`` reports on the inner range solve."""
    _gev_range("gev", n, il, iu, a, lda, b, ldb, w, z, ldz, mode)


def KMATH_EIGEN_GEV_RANGE_V(n, vl, vu, a, lda, b, ldb, w, z, ldz, mode="A", mmax=None):
    """EXTENSION, not in the reference: the eigenpairs of A x = lambda B x with ``vl <= lambda < vu`` by the Cholesky route
    of ``KMATH_EIGEN_GEV_RANGE``, one GPU.  Window, ``mmax``, modes, statuses and the returned ``(m, il)`` as for
    ``eigen_sx_range_v``; ``z[:, :m]`` with ``z^T B z = I``.  ``a`` is destroyed and ``b`` holds U on status 0; on status -9
    host arrays are left as they were passed.  Status -7 if B is not positive definite."""
    return _gev_range_v("gev", n, vl, vu, a, lda, b, ldb, w, z, ldz, mode, mmax)


def KMATH_EIGEN_HGEV(n, a, lda, b, ldb, w, z, ldz):
    """EXTENSION, not in the reference (it has no complex generalised solver): the complex Hermitian-definite problem
    A x = lambda B x by the method of KMATH_EIGEN_GEV over complex numbers (two eigen_h solves, three complex products).
    ``a``, ``b``, ``z``: complex128, column-major (numpy, Fortran order) or GPU tensors holding the column-major image
    (``a[j, i] = A(i, j)``), leading dimensions in complex elements; ``w`` float64.  Upper triangles of ``a``, ``b``
    significant; ``w`` ascending, ``z^H B z = I``; on exit ``a`` holds Y and ``b`` holds F = U mu^-1/2, as in
    KMATH_EIGEN_GEV.  If B is not positive definite a message is printed and the call returns (status -7)."""
    _gev("hgev", (0, -5, -7), n, a, lda, b, ldb, w, z, ldz)


def KMATH_EIGEN_HGEV_RANGE(n, il, iu, a, lda, b, ldb, w, z, ldz, mode="A"):
    """EXTENSION, not in the reference: eigenpairs ``il .. iu`` (1-based, inclusive) of the complex Hermitian-definite
    problem A x = lambda B x by the Cholesky route (B = U^H U, C = U^-H A U^-1, ``eigen_h`` of C with nvec = iu,
    Z = U^-1 Y), one GPU.  ``a``, ``b``, ``z``: complex128, column-major (numpy, Fortran order) or GPU tensors holding the
    column-major image (``a[j, i] = A(i, j)``), leading dimensions in complex elements; ``w`` float64.  ``w[:m]``
    ascending, ``z[:, :m]`` with ``z^H B z = I``, ``m = iu - il + 1``; modes 'A' and 'N' (``z`` may be None).  Upper
    triangles of ``a``, ``b`` significant; ``a`` is destroyed, ``b`` holds U in its upper triangle.  Status -7 if B is
    not positive definite, -5 (``w[:m]`` = NaN) for a non-finite entry of either triangle."""
    _gev_range("hgev", n, il, iu, a, lda, b, ldb, w, z, ldz, mode)


def KMATH_EIGEN_HGEV_RANGE_V(n, vl, vu, a, lda, b, ldb, w, z, ldz, mode="A", mmax=None):
    """EXTENSION, not in the reference: the eigenpairs of the complex Hermitian-definite problem A x = lambda B x with
    ``vl <= lambda < vu`` by the Cholesky route of ``KMATH_EIGEN_HGEV_RANGE`` with ``eigen_h_range_v`` as the inner solve,
    one GPU.  Arrays as for ``KMATH_EIGEN_HGEV_RANGE``; window, ``mmax``, modes, statuses and the returned ``(m, il)`` as
    for ``eigen_sx_range_v``; ``z[:, :m]`` with ``z^H B z = I``.  ``a`` is destroyed and ``b`` holds U on status 0; on
    status -9 host arrays are left as they were passed.  Status -7 if B is not positive definite.  Agrees with
    ``KMATH_EIGEN_HGEV_RANGE`` on the resolved window to rounding, not bit for bit (the inner routes differ)."""
    return _gev_range_v("hgev", n, vl, vu, a, lda, b, ldb, w, z, ldz, mode, mmax)
