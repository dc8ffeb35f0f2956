"""Worker of the multi-rank KMATH_EIGEN_HGEV test (an extension: the reference has no complex generalised solver):
`world` processes share GPU 0 as in mg_worker.py; cyclic blocks of A, B in, eigenvalues replicated, B-orthonormal
eigenvectors in cyclic blocks out.  gloo carries the session id and the test's own result gathering.
argv: rank world port n [PxxPy]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.distributed as dist

rank, world, port, n = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
dims = tuple(int(v) for v in sys.argv[5].split("x")) if len(sys.argv) > 5 and "x" in sys.argv[5] else None
os.environ.setdefault("EIGX_COMM_TIMEOUT_S", "60")
dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
import scipy.linalg

import eigenexa_amd as ee
from eigenexa_amd import _lib, api, layout

ee.eigen_init(comm=True, device=0, dims=dims)
procs, xp, yp = ee.eigen_get_procs()
_, xi, yi = ee.eigen_get_id()
rows = np.arange(xi - 1, n, xp)
cols = np.arange(yi - 1, n, yp)
nx, ny = ee.eigen_get_matdims(n)
low = rows[:, None] > cols[None, :]
diag = rows[:, None] == cols[None, :]


def blocks(M):
    """this rank's cyclic block of the upper triangle of M; NaN strictly below the diagonal and in Im of the diagonal"""
    loc = M[np.ix_(rows, cols)]
    loc = np.where(low, complex(np.nan, np.nan), loc)
    loc = np.where(diag, loc.real + 0j, loc)
    loc.imag[diag] = np.nan
    out = np.zeros((nx, ny), dtype=np.complex128, order="F")
    out[: len(rows), : len(cols)] = loc
    return out


def gather(x):
    xl = np.zeros(((n + xp - 1) // xp, (n + yp - 1) // yp), dtype=np.complex128)
    xl[: len(rows), : len(cols)] = x[: len(rows), : len(cols)]
    parts = [torch.zeros(xl.shape, dtype=torch.complex128) for _ in range(world)]
    dist.all_gather(parts, torch.from_numpy(np.ascontiguousarray(xl)))
    return layout.gather_cyclic([p.numpy() for p in parts], n, n, dims=dims)


A = layout.random_hermitian(n, seed=3)
B = layout.random_hpd(n, seed=n)
a, b = blocks(A), blocks(B)
z = np.zeros((nx, ny), dtype=np.complex128, order="F")
w = np.zeros(n)
ee.KMATH_EIGEN_HGEV(n, a, nx, b, nx, w, z, nx)
assert api.last_status() == 0, api.last_status()
# nothing gathered: planes of A, F, T and the transposes / C (8 n^2/P), the transposes' buffers, the SUMMA panels
held = _lib.load().eigx_held_bytes_named(b"hgev.")
assert 0 < held <= 8 * 12 * n * n // world + (1 << 20), (held, n, world)
if n >= 500:
    assert held < 0.7 * 8 * 8 * n * n, held
Z, F, Y = gather(z), gather(b), gather(a)
wr = scipy.linalg.eigh(A, B, eigvals_only=True)
scale = max(1.0, np.abs(wr).max())
assert np.abs(w - wr).max() < 1e-12 * scale, np.abs(w - wr).max()
assert np.linalg.norm(A @ Z - B @ Z * w) < 1e-12 * scale * n
assert np.linalg.norm(Z.conj().T @ B @ Z - np.eye(n)) < 1e-12 * n
assert np.linalg.norm(F.conj().T @ B @ F - np.eye(n)) < 1e-12 * n
assert np.linalg.norm(Y.conj().T @ Y - np.eye(n)) < 1e-12 * n
assert np.linalg.norm(F @ Y - Z) < 1e-12 * n * np.abs(F).max()
wt = torch.from_numpy(w.copy())
dist.broadcast(wt, src=0)
assert np.array_equal(wt.numpy(), w)
# an indefinite B: -7 on every rank
Bi = B - (np.linalg.eigvalsh(B)[0] + 1.0) * np.eye(n)
a, b = blocks(A), blocks(Bi)
ee.KMATH_EIGEN_HGEV(n, a, nx, b, nx, np.zeros(n), np.zeros((nx, ny), dtype=np.complex128, order="F"), nx)
assert api.last_status() == -7, api.last_status()
ee.eigen_free()
dist.barrier()
dist.destroy_process_group()
print(f"OK rank {rank}/{world} n={n} hgev", flush=True)
