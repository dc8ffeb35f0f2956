"""Timing of the batched small complex Hermitian eigensolve (an extension: eigx_h_batch_dev, csrc/hbatch.hip) on one GPU,
device API, against the two routes a caller had without it:
  (b) a loop of eigx_h_dev (nvec = n, the interface's default block sizes) over the matrices, and
  (c) for n <= 64, eigx_s_batch_dev on the real 2n x 2n embeddings [[X, -Y], [Y, X]] of the same matrices X + iY (every
      eigenvalue twice, 2n real vectors from which the caller would still have to pick n complex ones).
usage: gpu_hbatch_time.py [--repeats R] [--loop L] [--pool P] [n:batch ...]
(default 8:100000 16:50000 32:10000 64:4000 96:1000, modes 'A' and 'N')
The matrices are layout.random_hermitian(n, seed): P distinct ones (default 1000), repeated to fill the batch.  All routes run
in the same process, alternating, after one warm-up each.  The batch calls are timed whole (host clock around the call, which
returns after the result is complete); the loop is timed over the first L matrices of the same batch (default 200) and scaled
to the batch -- each of its calls ends in a host synchronisation, as a caller's loop does.  Printed: median and spread over
the repeats, the ratios, and the two gates (worst over the first L matrices of the batch call's result; mode 'N': the
eigenvalue error against LAPACK).  With eigx_tune key 22 below n the batch call is the loop itself; the tool leaves the key
at its default."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from eigenexa_amd import _lib, layout

args = sys.argv[1:]
repeats, nloop, npool = 5, 200, 1000
while args and args[0].startswith("--"):
    if args[0] == "--repeats":
        repeats = int(args[1])
    elif args[0] == "--loop":
        nloop = int(args[1])
    elif args[0] == "--pool":
        npool = int(args[1])
    else:
        raise SystemExit(f"unknown option {args[0]}")
    args = args[2:]
cases = [tuple(int(v) for v in s.split(":")) for s in args] or [(8, 100000), (16, 50000), (32, 10000), (64, 4000), (96, 1000)]
lib = _lib.load()
_lib.check(lib.eigx_init(0), "init")
dev = torch.device("cuda:0")
eps = np.finfo(np.float64).eps


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def cell(t):
    t = np.array(t) * 1e3
    return f"{np.median(t):>10.3f} [{t.min():>9.3f} .. {t.max():>9.3f}]"


print(f"{'n':>4} {'batch':>7} mode  {'(a) batch call ms':>34}  {'(b) loop of eigx_h_dev, scaled, ms':>34}  "
      f"{'(c) eigx_s_batch_dev on 2n x 2n, ms':>34}  {'b / a':>8}  {'c / a':>6}  {'us / matrix':>11}  gates (residual, orthogonality)",
      flush=True)
for n, batch in cases:
    P = min(npool, batch)
    pool = np.stack([layout.random_hermitian(n, seed=1000 * n + k) for k in range(P)])
    reps = -(-batch // P)
    M = torch.from_numpy(pool).to(dev)                   # M[k] = matrix k (row-major)
    # the column-major image of a Hermitian matrix is the row-major image of its transpose
    A0 = M.transpose(1, 2).contiguous().repeat(reps, 1, 1)[:batch].contiguous()
    a = torch.empty_like(A0)
    z = torch.zeros_like(A0)
    w = torch.zeros(batch, n, dtype=torch.float64, device=dev)
    info = torch.zeros(batch, dtype=torch.int32, device=dev)
    ar, zr = torch.view_as_real(a), torch.view_as_real(z)
    L = min(nloop, batch)
    embed = n <= 64
    if embed:
        X, Y = M.real, M.imag
        E = torch.cat([torch.cat([X, -Y], dim=2), torch.cat([Y, X], dim=2)], dim=1)   # symmetric: either image
        E0 = E.repeat(reps, 1, 1)[:batch].contiguous()
        ea = torch.empty_like(E0)
        ez = torch.zeros_like(E0)
        ew = torch.zeros(batch, 2 * n, dtype=torch.float64, device=dev)
        del E, X, Y

    def batch_call(mode):
        rc = lib.eigx_h_batch_dev(n, batch, ar.data_ptr(), n, n * n, w.data_ptr(), n, zr.data_ptr() if mode == b"A" else None, n,
                                  n * n, mode, info.data_ptr())
        _lib.check(rc, "eigx_h_batch_dev")

    def loop_call(mode):
        pa, pw, pz = ar.data_ptr(), w.data_ptr(), zr.data_ptr()
        for k in range(L):
            rc = lib.eigx_h_dev(n, n, pa + 16 * k * n * n, n, pw + 8 * k * n, (pz + 16 * k * n * n) if mode == b"A" else None, n, 48,
                                128, mode)
            _lib.check(rc, "eigx_h_dev")

    def embed_call(mode):
        m = 2 * n
        rc = lib.eigx_s_batch_dev(m, batch, ea.data_ptr(), m, m * m, ew.data_ptr(), m, ez.data_ptr() if mode == b"A" else None, m,
                                  m * m, mode, info.data_ptr())
        _lib.check(rc, "eigx_s_batch_dev")

    for mode in (b"A", b"N"):
        ta, tb, tc = [], [], []
        for rep in range(repeats + 1):   # rep 0 warms the kernels and the workspace pool of every route
            a.copy_(A0)
            dt = timed(lambda: loop_call(mode))
            if rep:
                tb.append(dt * batch / L)
            if embed:
                ea.copy_(E0)
                dt = timed(lambda: embed_call(mode))
                if rep:
                    tc.append(dt)
            a.copy_(A0)
            dt = timed(lambda: batch_call(mode))
            if rep:
                ta.append(dt)
        assert (info == 0).all().item()
        Ak = M[torch.arange(L, device=dev) % P]
        res = orth = float("nan")
        if mode == b"A":
            Z = z[:L].transpose(1, 2)    # Z[k][:, j] = eigenvector j of matrix k
            wc = w[:L, None, :].to(torch.complex128)
            res = (torch.linalg.norm(Ak @ Z - Z * wc, dim=(1, 2)) / (n * eps * torch.linalg.norm(Ak, dim=(1, 2)))).max().item()
            eye = torch.eye(n, dtype=torch.complex128, device=dev)
            orth = (torch.linalg.norm(Z.conj().transpose(1, 2) @ Z - eye, dim=(1, 2)) / (n * eps)).max().item()
        else:
            wl = torch.from_numpy(np.linalg.eigvalsh(pool[np.arange(L) % P])).to(dev)
            res = ((w[:L] - wl).abs().amax(dim=1) / wl.abs().amax(dim=1)).max().item()   # mode 'N': |w - w_lapack| / max|w|
        ma, mb = np.median(ta), np.median(tb)
        print(f"{n:>4} {batch:>7}  {mode.decode()}    {cell(ta)}  {cell(tb)}  {cell(tc) if embed else '-':>34}  {mb / ma:>8.1f}  "
              f"{(f'{np.median(tc) / ma:.2f}' if embed else '-'):>6}  {ma * 1e6 / batch:>11.3f}  {res:.2e} {orth:.2e}", flush=True)
    del A0, a, z, w, info, ar, zr, M
    if embed:
        del E0, ea, ez, ew
    torch.cuda.empty_cache()
lib.eigx_free()
