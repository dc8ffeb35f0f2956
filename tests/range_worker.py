"""Worker of the index-range tests (an extension: the reference has no index-range interface), always a fresh process.
argv: memory n m           one eigx_sx_range_dev in a process that never ran a full solve; prints what the pool holds
      ranks rank world port  `world` processes share GPU 0 (as in mg_worker.py): the range entries refuse more than one rank"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

what = sys.argv[1]
if what == "memory":
    import eigenexa_amd as ee
    from eigenexa_amd import _lib, layout

    n, m = int(sys.argv[2]), int(sys.argv[3])
    ee.eigen_init()
    lib = _lib.load()
    lib.eigx_tune(17, 100)
    dev = torch.device("cuda:0")
    nx, ny = ee.eigen_get_matdims(n)
    A = layout.random_symmetric_torch(n, dev)
    a = torch.zeros(n, nx, dtype=torch.float64, device=dev)
    a[:, :n] = A.T
    z = torch.zeros(m, nx, dtype=torch.float64, device=dev)
    w = torch.zeros(m, dtype=torch.float64, device=dev)
    rc = lib.eigx_sx_range_dev(n, 1, m, a.data_ptr(), nx, w.data_ptr(), z.data_ptr(), nx, 128, 128, b"A")
    assert rc == 0, rc
    info = ee.range_info()
    Z = z[:, :n].T
    eps = np.finfo(np.float64).eps
    res = torch.linalg.norm(A @ Z - Z * w[None, :]).item() / (n * eps * torch.linalg.norm(A).item())
    orth = torch.linalg.norm(Z.T @ Z - torch.eye(m, dtype=torch.float64, device=dev)).item() / (n * eps)
    assert res < 768 and orth < 8, (res, orth)
    print(f"MEMORY path={info.path} dc={lib.eigx_held_bytes_named(b'dc.')} held={lib.eigx_held_bytes()} "
          f"internal={lib.eigx_memory_internal(n, nx, nx, 128, 128)}", flush=True)
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
a = np.zeros((nx, ny), order="F")
z = np.zeros((nx, ny), order="F")
w = np.zeros(n)
for fn in (ee.eigen_sx_range, ee.eigen_s_range):
    fn(n, 1, 8, a, nx, w, z, nx)
    assert api.last_status() == -2, api.last_status()
dev = torch.device("cuda:0")
ad = torch.zeros(ny, nx, dtype=torch.float64, device=dev)
zd = torch.zeros(ny, nx, dtype=torch.float64, device=dev)
wd = torch.zeros(n, dtype=torch.float64, device=dev)
for fn in (lib.eigx_sx_range_dev, lib.eigx_s_range_dev):
    assert fn(n, 1, 8, ad.data_ptr(), nx, wd.data_ptr(), zd.data_ptr(), nx, 48, 128, b"A") == -2
dist.barrier()
ee.eigen_free()
dist.destroy_process_group()
print(f"OK rank {rank}/{world} range entries refused", flush=True)
