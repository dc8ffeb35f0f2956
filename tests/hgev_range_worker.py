"""Worker of the KMATH_EIGEN_HGEV_RANGE tests (an extension: the reference has no complex Cholesky-route generalised
solver), always a fresh process.
argv: uninit                 the entries before eigen_init: EIGX_ERR_NOT_INITIALIZED
      memory n m             one eigx_hgev_range_dev, window [1, m]; prints what the pool holds under "hgevr."
      ranks rank world port  `world` processes share GPU 0 (as in gev_range_worker.py): more than one rank is refused"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

what = sys.argv[1]
if what == "uninit":
    import eigenexa_amd as ee
    from eigenexa_amd import _lib, api

    lib = _lib.load()
    n = 8
    a = np.asfortranarray(np.eye(n, dtype=np.complex128))
    b = np.asfortranarray(np.eye(n, dtype=np.complex128))
    z = np.zeros((n, n), dtype=np.complex128, order="F")
    w = np.zeros(n)
    ee.KMATH_EIGEN_HGEV_RANGE(n, 1, n, a, n, b, n, w, z, n)
    assert api.last_status() == -1, api.last_status()
    assert lib.eigx_hgev_range(n, 1, n, a.ctypes.data, n, b.ctypes.data, n, w.ctypes.data, z.ctypes.data, n, b"A") == -1
    assert lib.eigx_hgev_range_dev(n, 1, n, None, n, None, n, None, None, n, b"A") == -1
    assert lib.eigx_zchol_dev(n, None, n) == -1
    assert lib.eigx_ztrsm_upper_dev(b"N", n, 1, None, n, None, n) == -1
    assert lib.eigx_hgev_reduce_dev(n, None, n, None, n) == -1
    print("OK uninit", flush=True)
    sys.exit(0)

if what == "memory":
    import eigenexa_amd as ee
    from eigenexa_amd import _lib, layout

    n, m = int(sys.argv[2]), int(sys.argv[3])
    ee.eigen_init()
    lib = _lib.load()
    dev = torch.device("cuda:0")
    A = torch.from_numpy(layout.random_hermitian(n, seed=3)).to(dev)
    B = torch.from_numpy(layout.random_hpd(n)).to(dev)
    ld = n + 2
    a = torch.zeros(n, ld, dtype=torch.complex128, device=dev)
    a[:, :n] = A.T
    b = torch.zeros(n, ld, dtype=torch.complex128, device=dev)
    b[:, :n] = B.T
    z = torch.zeros(m, ld, dtype=torch.complex128, device=dev)
    w = torch.zeros(m, dtype=torch.float64, device=dev)
    rc = lib.eigx_hgev_range_dev(n, 1, m, a.data_ptr(), ld, b.data_ptr(), ld, w.data_ptr(), z.data_ptr(), ld, b"A")
    assert rc == 0, rc
    Z = z[:, :n].T
    scale = max(1.0, w.abs().max().item())
    res = torch.linalg.norm(A @ Z - (B @ Z) * w.to(torch.complex128)[None, :]).item()
    orth = torch.linalg.norm(Z.conj().T @ B @ Z - torch.eye(m, dtype=torch.complex128, device=dev)).item()
    assert res < 1e-12 * scale * n and orth < 1e-12 * n, (res, orth)
    nb = lib.eigx_tune(20, 256)
    lib.eigx_tune(20, nb)
    print(f"MEMORY hgevr={lib.eigx_held_bytes_named(b'hgevr.')} held={lib.eigx_held_bytes()} nb={nb}", flush=True)
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
b = np.zeros((nx, ny), dtype=np.complex128, order="F")
z = np.zeros((nx, ny), dtype=np.complex128, order="F")
w = np.zeros(n)
ee.KMATH_EIGEN_HGEV_RANGE(n, 1, 8, a, nx, b, nx, w, z, nx)     # prints the one line
assert api.last_status() == -2, api.last_status()
# the stages answer EIGX_ERR_INTERNAL on more than one rank
dev = torch.device("cuda:0")
ad = torch.zeros(ny, nx, dtype=torch.complex128, device=dev)
assert lib.eigx_zchol_dev(nx, ad.data_ptr(), nx) == -6
dist.barrier()
ee.eigen_free()
dist.destroy_process_group()
print(f"OK rank {rank}/{world} generalised range entry refused", flush=True)
