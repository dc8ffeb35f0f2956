"""Timing of the batched small symmetric eigensolve (an extension: eigx_s_batch_dev, csrc/batch.hip) on one GPU, device API,
against the route to the same answers without it: a loop of eigx_s_dev (nvec = n, the interface's default block sizes) over
the matrices.  usage: gpu_batch_time.py [--repeats R] [--loop L] [n:batch ...]
(default 8:100000 16:50000 32:10000 64:4000 96:2000 128:1000, modes 'A' and 'N')
Both run in the same process, alternating, after one warm-up each.  The batch call is timed whole (host clock around the
call, which returns after the result is complete); the loop is timed over the first L matrices of the same batch (default
200) and scaled to the batch -- each of its calls ends in a host synchronisation, as a caller's loop does.  Printed: median
and spread over the repeats, the ratio, and the two gates (worst over the first L matrices of the batch call's result).
With eigx_tune key 21 below n the batch call is the loop itself; the tool leaves the key at its default."""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from eigenexa_amd import _lib

args = sys.argv[1:]
repeats, nloop = 5, 200
while args and args[0].startswith("--"):
    if args[0] == "--repeats":
        repeats = int(args[1])
    elif args[0] == "--loop":
        nloop = int(args[1])
    else:
        raise SystemExit(f"unknown option {args[0]}")
    args = args[2:]
cases = [tuple(int(v) for v in s.split(":")) for s in args] or [(8, 100000), (16, 50000), (32, 10000), (64, 4000), (96, 2000),
                                                                 (128, 1000)]
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


print(f"{'n':>4} {'batch':>7} mode  {'batch call ms':>28}  {'loop of eigx_s_dev, scaled, ms':>34}  {'speed-up':>8}  "
      f"{'us / matrix':>11}  gates (residual, orthogonality)", flush=True)
for n, batch in cases:
    g = torch.Generator(device=dev)
    g.manual_seed(1000 + n)
    R = torch.rand(batch, n, n, dtype=torch.float64, device=dev, generator=g) - 0.5
    A0 = R + R.transpose(1, 2)       # symmetric: the row-major image of a matrix is its column-major image
    del R
    a = torch.empty_like(A0)
    z = torch.zeros_like(A0)
    w = torch.zeros(batch, n, dtype=torch.float64, device=dev)
    info = torch.zeros(batch, dtype=torch.int32, device=dev)
    L = min(nloop, batch)

    def batch_call(mode):
        rc = lib.eigx_s_batch_dev(n, batch, a.data_ptr(), n, n * n, w.data_ptr(), n, z.data_ptr() if mode == b"A" else None, n,
                                  n * n, mode, info.data_ptr())
        _lib.check(rc, "eigx_s_batch_dev")

    def loop_call(mode):
        pa, pw, pz = a.data_ptr(), w.data_ptr(), z.data_ptr()
        for k in range(L):
            rc = lib.eigx_s_dev(n, n, pa + 8 * k * n * n, n, pw + 8 * k * n, (pz + 8 * k * n * n) if mode == b"A" else None, n, 48,
                                128, mode)
            _lib.check(rc, "eigx_s_dev")

    for mode in (b"A", b"N"):
        tb, tl = [], []
        for rep in range(repeats + 1):   # rep 0 warms the kernels and the workspace pool of both
            a.copy_(A0)
            dt = timed(lambda: loop_call(mode))
            if rep:
                tl.append(dt * batch / L)
            a.copy_(A0)
            dt = timed(lambda: batch_call(mode))
            if rep:
                tb.append(dt)
        assert (info == 0).all().item()
        res = orth = float("nan")
        if mode == b"A":
            Z = z[:L].transpose(1, 2)    # Z[k][:, j] = eigenvector j of matrix k
            Ak = A0[:L]
            res = (torch.linalg.norm(Ak @ Z - Z * w[:L, None, :], dim=(1, 2)) / (n * eps * torch.linalg.norm(Ak, dim=(1, 2)))).max().item()
            orth = (torch.linalg.norm(Z.transpose(1, 2) @ Z - torch.eye(n, dtype=torch.float64, device=dev), dim=(1, 2)) / (n * eps)).max().item()
        else:
            wl = torch.linalg.eigvalsh(A0[:L])
            res = ((w[:L] - wl).abs().amax(dim=1) / wl.abs().amax(dim=1)).max().item()   # mode 'N': |w - w_lapack| / max|w|
        b, l = np.array(tb) * 1e3, np.array(tl) * 1e3
        print(f"{n:>4} {batch:>7}  {mode.decode()}    {np.median(b):>9.3f} [{b.min():>7.3f} .. {b.max():>8.3f}]  "
              f"{np.median(l):>12.1f} [{l.min():>9.1f} .. {l.max():>9.1f}]  {np.median(l) / np.median(b):>8.1f}  "
              f"{np.median(b) * 1e3 / batch:>11.3f}  {res:.2e} {orth:.2e}", flush=True)
    del A0, a, z, w, info
    torch.cuda.empty_cache()
lib.eigx_free()
