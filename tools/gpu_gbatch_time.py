"""Timing of the batched small generalised eigensolve (an extension: eigx_gev_batch_dev, csrc/gbatch.hip) on one GPU, device API:
  (a) the batch call;
  (b) the route to the same answers without it: a loop of eigx_gev_range_dev(n, 1, n, ...) over the pencils;
  (c) for orientation, eigx_s_batch_dev on the matrices A alone at the same (n, batch): (a) / (c) is what the Cholesky
      factorisation, the substitutions and the second LDS array cost.
usage: gpu_gbatch_time.py [--repeats R] [--loop L] [n:batch ...]
(default 8:100000 16:50000 32:10000 64:4000 96:1000, modes 'A' and 'N')
The pencils: A = R + R^T with R uniform in [-0.5, 0.5), B = G G^T / n + 0.1 I with G uniform in [-0.5, 0.5).  All routes run in
the same process, alternating, after one warm-up each.  The batch calls are timed whole (host clock around the call, which
returns after the result is complete); the loop is timed over the first L pencils of the same batch (default 200) and scaled
to the batch -- each of its calls ends in host synchronisations, as a caller's loop does.  Printed: median and spread over the
repeats, the ratios, and the gates of tests/test_gbatch.py in units of each gate (worst over the first L pencils of the batch
call's result, against scipy.linalg.eigh: eigenvalues, residual, B-orthogonality, factor; mode 'N': eigenvalues and factor).
With eigx_tune key 23 below n the batch call is the loop itself; the tool leaves the key at its default."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.linalg
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
cases = [tuple(int(v) for v in s.split(":")) for s in args] or [(8, 100000), (16, 50000), (32, 10000), (64, 4000), (96, 1000)]
lib = _lib.load()
_lib.check(lib.eigx_init(0), "init")
dev = torch.device("cuda:0")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def cell(t):
    return f"{np.median(t):>10.3f} [{t.min():>9.3f} .. {t.max():>9.3f}]"


print(f"{'n':>4} {'batch':>7} mode  {'(a) batch call ms':>34}  {'(b) loop of eigx_gev_range_dev, scaled':>38}  "
      f"{'(c) eigx_s_batch_dev on A, ms':>34}  {'b / a':>8}  {'a / c':>6}  {'us / pencil':>11}  "
      f"gates (w, residual, B-orthogonality, factor; 1 = the gate)", flush=True)
for n, batch in cases:
    g = torch.Generator(device=dev)
    g.manual_seed(1000 + n)
    R = torch.rand(batch, n, n, dtype=torch.float64, device=dev, generator=g) - 0.5
    A0 = R + R.transpose(1, 2)       # symmetric: the row-major image of a matrix is its column-major image
    R = torch.rand(batch, n, n, dtype=torch.float64, device=dev, generator=g) - 0.5
    B0 = R @ R.transpose(1, 2) / n + 0.1 * torch.eye(n, dtype=torch.float64, device=dev)
    B0 = 0.5 * (B0 + B0.transpose(1, 2))
    del R
    a, b = torch.empty_like(A0), torch.empty_like(B0)
    z = torch.zeros_like(A0)
    w = torch.zeros(batch, n, dtype=torch.float64, device=dev)
    info = torch.zeros(batch, dtype=torch.int32, device=dev)
    L = min(nloop, batch)
    Ah, Bh = A0[:L].cpu().numpy(), B0[:L].cpu().numpy()
    wref = torch.from_numpy(np.stack([scipy.linalg.eigh(Ah[k], Bh[k], eigvals_only=True) for k in range(L)])).to(dev)
    scale = wref.abs().amax(dim=1).clamp(min=1.0)
    eye = torch.eye(n, dtype=torch.float64, device=dev)

    def batch_call(mode):
        rc = lib.eigx_gev_batch_dev(n, batch, a.data_ptr(), n, n * n, b.data_ptr(), n, n * n, w.data_ptr(), n,
                                    z.data_ptr() if mode == b"A" else None, n, n * n, mode, info.data_ptr())
        _lib.check(rc, "eigx_gev_batch_dev")

    def loop_call(mode):
        pa, pb, pw, pz = a.data_ptr(), b.data_ptr(), w.data_ptr(), z.data_ptr()
        for k in range(L):
            rc = lib.eigx_gev_range_dev(n, 1, n, pa + 8 * k * n * n, n, pb + 8 * k * n * n, n, pw + 8 * k * n,
                                        (pz + 8 * k * n * n) if mode == b"A" else None, n, mode)
            _lib.check(rc, "eigx_gev_range_dev")

    def s_batch_call(mode):
        rc = lib.eigx_s_batch_dev(n, batch, a.data_ptr(), n, n * n, w.data_ptr(), n, z.data_ptr() if mode == b"A" else None, n, n * n,
                                  mode, info.data_ptr())
        _lib.check(rc, "eigx_s_batch_dev")

    # eigx_gev_range_dev wants even leading dimensions: at an odd n the loop is not a route a caller has without a copy
    loop_ok = n % 2 == 0
    for mode in (b"A", b"N"):
        ta, tb, tc = [], [], []
        for rep in range(repeats + 1):   # rep 0 warms the kernels and the workspace pool of every route
            if loop_ok:
                a.copy_(A0)
                b.copy_(B0)
                dt = timed(lambda: loop_call(mode))
                if rep:
                    tb.append(dt * batch / L)
            a.copy_(A0)
            dt = timed(lambda: s_batch_call(mode))
            if rep:
                tc.append(dt)
            a.copy_(A0)
            b.copy_(B0)
            dt = timed(lambda: batch_call(mode))
            if rep:
                ta.append(dt)
        assert (info == 0).all().item()
        U = torch.triu(b[:L].transpose(1, 2))
        Bk, Ak = B0[:L], A0[:L]
        gw = ((w[:L] - wref).abs().amax(dim=1) / (1e-12 * scale)).max().item()
        gf = (torch.linalg.norm(U.transpose(1, 2) @ U - Bk, dim=(1, 2)) / (1e-12 * n * torch.linalg.norm(Bk, dim=(1, 2)))).max().item()
        gr = go = float("nan")
        if mode == b"A":
            Z = z[:L].transpose(1, 2)    # Z[k][:, j] = eigenvector j of pencil k
            gr = (torch.linalg.norm(Ak @ Z - Bk @ Z * w[:L, None, :], dim=(1, 2)) / (1e-12 * scale * n)).max().item()
            go = (torch.linalg.norm(Z.transpose(1, 2) @ Bk @ Z - eye, dim=(1, 2)) / (1e-12 * n)).max().item()
        ta, tc = np.array(ta) * 1e3, np.array(tc) * 1e3
        tb = np.array(tb) * 1e3 if loop_ok else None
        ma = np.median(ta)
        print(f"{n:>4} {batch:>7}  {mode.decode()}    {cell(ta)}  {cell(tb) if loop_ok else '-':>38}  {cell(tc)}  "
              f"{(f'{np.median(tb) / ma:.1f}' if loop_ok else '-'):>8}  {ma / np.median(tc):>6.2f}  {ma * 1e3 / batch:>11.3f}  "
              f"{gw:.2e} {gr:.2e} {go:.2e} {gf:.2e}", flush=True)
    del A0, B0, a, b, z, w, info
    torch.cuda.empty_cache()
lib.eigx_free()
