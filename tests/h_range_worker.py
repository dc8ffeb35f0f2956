"""Worker of the Hermitian range tests (tests/test_h_range.py), always a fresh process.
argv: noinit                 no eigen_init: all six entries return EIGX_ERR_NOT_INITIALIZED (-1)
      memory n m             one eigx_h_range_dev, window [1, m], on the subset path in a process that never ran another
                             solve; prints what the pool holds under "dc." and "h.Zri"
      ranks rank world port  `world` processes share GPU 0 (as in range_v_worker.py): the entries refuse more than one rank"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

what = sys.argv[1]
if what == "noinit":
    import eigenexa_amd as ee
    from eigenexa_amd import _lib, api

    lib = _lib.load()
    n = 16
    a = np.asfortranarray(np.eye(n, dtype=np.complex128))
    z = np.zeros((n, n), dtype=np.complex128, order="F")
    w = np.zeros(n)
    m, il = C.c_int(-3), C.c_int(-3)
    pa, pw, pz = a.ctypes.data, w.ctypes.data, z.ctypes.data
    for fn in (lib.eigx_h_range, lib.eigx_h_range_dev):
        assert fn(n, 1, n, pa, n, pw, pz, n, 48, 128, b"A") == -1
    for fn in (lib.eigx_h_range_v, lib.eigx_h_range_v_dev):
        assert fn(n, 0.0, 2.0, n, C.byref(m), C.byref(il), pa, n, pw, pz, n, 48, 128, b"A") == -1
    for fn in (lib.eigx_hgev_range_v, lib.eigx_hgev_range_v_dev):
        assert fn(n, 0.0, 2.0, n, C.byref(m), C.byref(il), pa, n, pa, n, pw, pz, n, b"A") == -1
    assert (m.value, il.value) == (-3, -3) and (w == 0).all() and (z == 0).all()
    ee.eigen_h_range(n, 1, n, a, n, w, z, n)
    assert api.last_status() == -1
    assert ee.eigen_h_range_v(n, 0.0, 2.0, a, n, w, z, n) is None and api.last_status() == -1
    assert ee.KMATH_EIGEN_HGEV_RANGE_V(n, 0.0, 2.0, a, n, a, n, w, z, n) is None and api.last_status() == -1
    print("OK noinit", flush=True)
    sys.exit(0)

if what == "memory":
    import eigenexa_amd as ee
    from eigenexa_amd import _lib, layout

    n, m = int(sys.argv[2]), int(sys.argv[3])
    ee.eigen_init()
    lib = _lib.load()
    lib.eigx_tune(17, 100)
    dev = torch.device("cuda:0")
    A = torch.from_numpy(layout.random_hermitian(n, seed=3)).to(dev)
    ld = n + 2
    a = torch.zeros(n, ld, dtype=torch.complex128, device=dev)
    a[:, :n] = A.T
    z = torch.zeros(m, ld, dtype=torch.complex128, device=dev)
    w = torch.zeros(m, dtype=torch.float64, device=dev)
    rc = lib.eigx_h_range_dev(n, 1, m, a.data_ptr(), ld, w.data_ptr(), z.data_ptr(), ld, 48, 128, b"A")
    assert rc == 0, rc
    info = ee.range_info()
    Z = z[:, :n].T
    eps = np.finfo(np.float64).eps
    res = torch.linalg.norm(A @ Z - Z * w.to(torch.complex128)[None, :]).item() / (n * eps * torch.linalg.norm(A).item())
    orth = torch.linalg.norm(Z.conj().T @ Z - torch.eye(m, dtype=torch.complex128, device=dev)).item() / (n * eps)
    assert res < 768 and orth < 8, (res, orth)
    print(f"MEMORY path={info.path} dc={lib.eigx_held_bytes_named(b'dc.')} zri={lib.eigx_held_bytes_named(b'h.Zri')} "
          f"held={lib.eigx_held_bytes()}", flush=True)
    ee.eigen_free()
    sys.exit(0)

import torch.distributed as dist

rank, world, port = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
os.environ.setdefault("EIGX_COMM_TIMEOUT_S", "60")
dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
import eigenexa_amd as ee
from eigenexa_amd import _lib, api

ee.eigen_init(comm=True, device=0)
lib = _lib.load()
n = 64
nx, ny = ee.eigen_get_matdims(n)
a = np.zeros((nx, ny), dtype=np.complex128, order="F")
z = np.zeros((nx, ny), dtype=np.complex128, order="F")
w = np.zeros(n)
ee.eigen_h_range(n, 1, 8, a, nx, w, z, nx)
assert api.last_status() == -2, api.last_status()
assert ee.eigen_h_range_v(n, 0.0, 1.0, a, nx, w, z, nx, mmax=8) is None and api.last_status() == -2
assert ee.KMATH_EIGEN_HGEV_RANGE_V(n, 0.0, 1.0, a, nx, a, nx, w, z, nx, mmax=8) is None and api.last_status() == -2
dev = torch.device("cuda:0")
ad = torch.zeros(ny, nx, dtype=torch.complex128, device=dev)
zd = torch.zeros(ny, nx, dtype=torch.complex128, device=dev)
wd = torch.zeros(n, dtype=torch.float64, device=dev)
m, il = C.c_int(-3), C.c_int(-3)
assert lib.eigx_h_range_dev(n, 1, 8, ad.data_ptr(), nx, wd.data_ptr(), zd.data_ptr(), nx, 48, 128, b"A") == -2
assert lib.eigx_h_range_v_dev(n, 0.0, 1.0, 8, C.byref(m), C.byref(il), ad.data_ptr(), nx, wd.data_ptr(), zd.data_ptr(), nx, 48,
                              128, b"A") == -2
assert lib.eigx_hgev_range_v_dev(n, 0.0, 1.0, 8, C.byref(m), C.byref(il), ad.data_ptr(), nx, ad.data_ptr(), nx, wd.data_ptr(),
                                 zd.data_ptr(), nx, b"A") == -2
assert (m.value, il.value) == (-3, -3)
dist.barrier()
ee.eigen_free()
dist.destroy_process_group()
print(f"OK rank {rank}/{world} Hermitian range entries refused", flush=True)
