"""Worker of the value-window tests (tests/test_range_v.py), always a fresh process.
argv: noinit                 no eigen_init: every value-window entry returns EIGX_ERR_NOT_INITIALIZED (-1)
      ranks rank world port  `world` processes share GPU 0 (as in range_worker.py): the entries refuse more than one rank"""
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
    a = np.asfortranarray(np.eye(n))
    z = np.zeros((n, n), order="F")
    w = np.zeros(n)
    m, il = C.c_int(-3), C.c_int(-3)
    for fn in (lib.eigx_sx_range_v, lib.eigx_s_range_v, lib.eigx_sx_range_v_dev, lib.eigx_s_range_v_dev):
        assert fn(n, 0.0, 2.0, n, C.byref(m), C.byref(il), a.ctypes.data, n, w.ctypes.data, z.ctypes.data, n, 48, 128, b"A") == -1
    for fn in (lib.eigx_gev_range_v, lib.eigx_gev_range_v_dev):
        assert fn(n, 0.0, 2.0, n, C.byref(m), C.byref(il), a.ctypes.data, n, a.ctypes.data, n, w.ctypes.data, z.ctypes.data, n,
                  b"A") == -1
    assert lib.eigx_band_count_dev(n, w.ctypes.data, z.ctypes.data, n, 1, 2, w.ctypes.data, None) == -1
    assert (m.value, il.value) == (-3, -3) and (w == 0).all() and (z == 0).all()
    for fn in (ee.eigen_sx_range_v, ee.eigen_s_range_v):
        assert fn(n, 0.0, 2.0, a, n, w, z, n) is None and api.last_status() == -1
    assert ee.KMATH_EIGEN_GEV_RANGE_V(n, 0.0, 2.0, a, n, a, n, w, z, n) is None and api.last_status() == -1
    print("OK noinit", flush=True)
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
a = np.zeros((nx, ny), order="F")
z = np.zeros((nx, ny), order="F")
w = np.zeros(n)
for fn in (ee.eigen_sx_range_v, ee.eigen_s_range_v):
    assert fn(n, 0.0, 1.0, a, nx, w, z, nx, mmax=8) is None
    assert api.last_status() == -2, api.last_status()
assert ee.KMATH_EIGEN_GEV_RANGE_V(n, 0.0, 1.0, a, nx, a, nx, w, z, nx, mmax=8) is None and api.last_status() == -2
dev = torch.device("cuda:0")
ad = torch.zeros(ny, nx, dtype=torch.float64, device=dev)
zd = torch.zeros(ny, nx, dtype=torch.float64, device=dev)
wd = torch.zeros(n, dtype=torch.float64, device=dev)
m, il = C.c_int(-3), C.c_int(-3)
for fn in (lib.eigx_sx_range_v_dev, lib.eigx_s_range_v_dev):
    assert fn(n, 0.0, 1.0, 8, C.byref(m), C.byref(il), ad.data_ptr(), nx, wd.data_ptr(), zd.data_ptr(), nx, 48, 128, b"A") == -2
assert lib.eigx_gev_range_v_dev(n, 0.0, 1.0, 8, C.byref(m), C.byref(il), ad.data_ptr(), nx, ad.data_ptr(), nx, wd.data_ptr(),
                                zd.data_ptr(), nx, b"A") == -2
assert (m.value, il.value) == (-3, -3)
dist.barrier()
ee.eigen_free()
dist.destroy_process_group()
print(f"OK rank {rank}/{world} value-window entries refused", flush=True)
