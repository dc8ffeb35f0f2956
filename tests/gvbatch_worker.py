"""Worker of the ragged pencil-batch tests (tests/test_gvbatch.py), always a fresh process.
argv: ranks rank world port  `world` processes share GPU 0 (as in gbatch_worker.py): the entries of both families, host and
device form, refuse more than one rank and touch nothing"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.distributed as dist

assert sys.argv[1] == "ranks"
rank, world, port = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
os.environ.setdefault("EIGX_COMM_TIMEOUT_S", "60")
dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
import eigenexa_amd as ee
from eigenexa_amd import _lib, api, layout

ee.eigen_init(comm=True, device=0)
lib = _lib.load()
n = np.array([16, 3, 40], dtype=np.int32)
off_a, la = layout.ragged_offsets(n)
off_w, lw = layout.ragged_offsets(n, ld=1)
dev = torch.device("cuda:0")
for which, fn, dt, cs in (("gev", ee.eigen_gev_vbatch, np.float64, 1), ("hgev", ee.eigen_hgev_vbatch, np.complex128, 2)):
    a = np.zeros(la, dtype=dt)
    for k in range(3):
        a[off_a[k]:off_a[k] + n[k] * n[k]] = np.eye(n[k]).reshape(-1)
    b = a.copy()
    z = np.full(la, 7.0, dtype=dt)
    w = np.full(lw, 7.0)
    info = np.full(3, 77, dtype=np.int32)
    for mode in ("A", "N"):
        fn(3, n, a, off_a, n, b, off_a, n, w, off_w, z, off_a, n, mode=mode, info=info)
        assert api.last_status() == -2, api.last_status()
    assert (w == 7.0).all() and (z == 7.0).all() and (info == 77).all() and np.array_equal(a, b)
    ad = torch.zeros(cs * la, dtype=torch.float64, device=dev)
    bd = torch.full((cs * la,), 3.0, dtype=torch.float64, device=dev)
    zd = torch.full((cs * la,), 7.0, dtype=torch.float64, device=dev)
    wd = torch.full((lw,), 7.0, dtype=torch.float64, device=dev)
    idv = torch.full((3,), 77, dtype=torch.int32, device=dev)
    rc = getattr(lib, f"eigx_{which}_vbatch_dev")(3, n.ctypes.data, ad.data_ptr(), off_a.ctypes.data, n.ctypes.data, bd.data_ptr(),
                                                   off_a.ctypes.data, n.ctypes.data, wd.data_ptr(), off_w.ctypes.data,
                                                   zd.data_ptr(), off_a.ctypes.data, n.ctypes.data, b"A", idv.data_ptr())
    assert rc == -2, rc
    assert (wd == 7.0).all().item() and (zd == 7.0).all().item() and (idv == 77).all().item() and (bd == 3.0).all().item()
dist.barrier()
ee.eigen_free()
dist.destroy_process_group()
print(f"OK rank {rank}/{world} gvbatch entries refused", flush=True)
