"""Worker of the windowed batched complex generalised tests (tests/test_hgbatch_range.py), always a fresh process.
argv: ranks rank world port  `world` processes share GPU 0 (as in gbatch_range_worker.py): both entries refuse more than one rank"""
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
from eigenexa_amd import _lib, api

ee.eigen_init(comm=True, device=0)
lib = _lib.load()
n, nb, il, iu = 16, 4, 2, 5
m = iu - il + 1
eye = np.asfortranarray(np.broadcast_to(np.eye(n, dtype=np.complex128)[:, :, None], (n, n, nb)).copy())
a, b = eye.copy(order="F"), 2.0 * eye
z = np.full((n, m, nb), 7.0 + 0j, order="F")
w = np.full((m, nb), 7.0, order="F")
info = np.full(nb, 77, dtype=np.int32)
for mode in ("A", "N"):
    ee.eigen_hgev_batch_range(n, nb, il, iu, a, n, b, n, w, z, n, mode=mode, info=info)
    assert api.last_status() == -2, api.last_status()
assert (w == 7.0).all() and (z == 7.0).all() and (info == 77).all() and (b == 2.0 * eye).all()
dev = torch.device("cuda:0")
ad = torch.zeros(2 * nb * n * n, dtype=torch.float64, device=dev)
bd = torch.full((2 * nb * n * n,), 3.0, dtype=torch.float64, device=dev)
zd = torch.full((2 * nb * n * m,), 7.0, dtype=torch.float64, device=dev)
wd = torch.full((nb * m,), 7.0, dtype=torch.float64, device=dev)
idv = torch.full((nb,), 77, dtype=torch.int32, device=dev)
assert lib.eigx_hgev_batch_range_dev(n, nb, il, iu, ad.data_ptr(), n, n * n, bd.data_ptr(), n, n * n, wd.data_ptr(), m, zd.data_ptr(), n,
                                     n * m, b"A", idv.data_ptr()) == -2
assert (wd == 7.0).all().item() and (zd == 7.0).all().item() and (idv == 77).all().item() and (bd == 3.0).all().item()
dist.barrier()
ee.eigen_free()
dist.destroy_process_group()
print(f"OK rank {rank}/{world} windowed complex generalised batch entries refused", flush=True)
