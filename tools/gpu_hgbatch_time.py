"""Timing of the batched small complex generalised eigensolve (an extension: eigx_hgev_batch_dev, csrc/hgbatch.hip) on one GPU,
device API:
  (a) the batch call;
  (b) the route to the same answers without it: a loop of eigx_hgev_range_dev(n, 1, n, ...) over the pencils;
  (c) for n <= 48, eigx_gev_batch_dev on the real 2n x 2n embeddings [[X, -Y], [Y, X]] of both matrices X + iY (every eigenvalue
      twice, 2n real vectors from which the caller would still have to pick n complex ones);
  (d) for orientation, eigx_h_batch_dev on the matrices A alone at the same (n, batch): (a) / (d) is what the Cholesky
      factorisation, the substitutions and the second pair of LDS planes cost.
usage: gpu_hgbatch_time.py [--repeats R] [--loop L] [n:batch ...]
(default 8:100000 16:50000 32:10000 48:6000 64:4000, modes 'A' and 'N')
The pencils: A = R + R^H, B = G G^H / n + 0.1 I with the real and imaginary parts of R and G uniform in [-0.5, 0.5).  All routes
run in the same process, alternating, after one warm-up each.  The batch calls are timed whole (host clock around the call,
which returns after the result is complete); the loop is timed over the first L pencils of the same batch (default 200) and
scaled to the batch -- each of its calls ends in host synchronisations, as a caller's loop does.  Printed: median and spread
over the repeats, the ratios, and the gates of tests/test_hgbatch.py in units of each gate (worst over the first L pencils of
the batch call's result, against scipy.linalg.eigh: eigenvalues, residual, B-orthogonality, factor; mode 'N': eigenvalues and
factor).  With eigx_tune key 24 below n the batch call is the loop itself; the tool leaves the key at its default."""
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
cases = [tuple(int(v) for v in s.split(":")) for s in args] or [(8, 100000), (16, 50000), (32, 10000), (48, 6000), (64, 4000)]
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
    t = np.array(t) * 1e3
    return f"{np.median(t):>10.3f} [{t.min():>9.3f} .. {t.max():>9.3f}]"


def crand(g, batch, n):
    return torch.complex(torch.rand(batch, n, n, dtype=torch.float64, device=dev, generator=g) - 0.5,
                         torch.rand(batch, n, n, dtype=torch.float64, device=dev, generator=g) - 0.5)


def embedding(M):
    """the real symmetric 2n x 2n matrices [[X, -Y], [Y, X]] of the Hermitian M = X + iY (symmetric: either memory image)"""
    X, Y = M.real, M.imag
    return torch.cat([torch.cat([X, -Y], dim=2), torch.cat([Y, X], dim=2)], dim=1).contiguous()


print(f"{'n':>4} {'batch':>7} mode  {'(a) batch call ms':>34}  {'(b) loop of eigx_hgev_range_dev, scaled':>38}  "
      f"{'(c) eigx_gev_batch_dev on 2n x 2n, ms':>38}  {'(d) eigx_h_batch_dev on A, ms':>34}  {'b / a':>8}  {'c / a':>6}  {'a / d':>6}  "
      f"{'us / pencil':>11}  gates (w, residual, B-orthogonality, factor; 1 = the gate)", flush=True)
for n, batch in cases:
    g = torch.Generator(device=dev)
    g.manual_seed(2000 + n)
    R = crand(g, batch, n)
    Am = R + R.conj().transpose(1, 2)        # Am[k] = A of pencil k (row-major)
    R = crand(g, batch, n)
    Bm = R @ R.conj().transpose(1, 2) / n + 0.1 * torch.eye(n, dtype=torch.complex128, device=dev)
    Bm = 0.5 * (Bm + Bm.conj().transpose(1, 2))
    del R
    # the column-major image of a Hermitian matrix is the row-major image of its transpose
    A0, B0 = Am.transpose(1, 2).contiguous(), Bm.transpose(1, 2).contiguous()
    a, b = torch.empty_like(A0), torch.empty_like(B0)
    z = torch.zeros_like(A0)
    w = torch.zeros(batch, n, dtype=torch.float64, device=dev)
    info = torch.zeros(batch, dtype=torch.int32, device=dev)
    ar, br, zr = torch.view_as_real(a), torch.view_as_real(b), torch.view_as_real(z)
    L = min(nloop, batch)
    Ak, Bk = Am[:L].clone(), Bm[:L].clone()
    Ah, Bh = Ak.cpu().numpy(), Bk.cpu().numpy()
    wref = torch.from_numpy(np.stack([scipy.linalg.eigh(Ah[k], Bh[k], eigvals_only=True) for k in range(L)])).to(dev)
    scale = wref.abs().amax(dim=1).clamp(min=1.0)
    eye = torch.eye(n, dtype=torch.complex128, device=dev)
    embed = n <= 48
    if embed:
        EA0, EB0 = embedding(Am), embedding(Bm)
        ea, eb = torch.empty_like(EA0), torch.empty_like(EB0)
        ez = torch.zeros_like(EA0)
        ew = torch.zeros(batch, 2 * n, dtype=torch.float64, device=dev)
    del Am, Bm

    def batch_call(mode):
        rc = lib.eigx_hgev_batch_dev(n, batch, ar.data_ptr(), n, n * n, br.data_ptr(), n, n * n, w.data_ptr(), n,
                                     zr.data_ptr() if mode == b"A" else None, n, n * n, mode, info.data_ptr())
        _lib.check(rc, "eigx_hgev_batch_dev")

    def loop_call(mode):
        pa, pb, pw, pz = ar.data_ptr(), br.data_ptr(), w.data_ptr(), zr.data_ptr()
        for k in range(L):
            rc = lib.eigx_hgev_range_dev(n, 1, n, pa + 16 * k * n * n, n, pb + 16 * k * n * n, n, pw + 8 * k * n,
                                         (pz + 16 * k * n * n) if mode == b"A" else None, n, mode)
            _lib.check(rc, "eigx_hgev_range_dev")

    def embed_call(mode):
        m = 2 * n
        rc = lib.eigx_gev_batch_dev(m, batch, ea.data_ptr(), m, m * m, eb.data_ptr(), m, m * m, ew.data_ptr(), m,
                                    ez.data_ptr() if mode == b"A" else None, m, m * m, mode, info.data_ptr())
        _lib.check(rc, "eigx_gev_batch_dev")

    def h_batch_call(mode):
        rc = lib.eigx_h_batch_dev(n, batch, ar.data_ptr(), n, n * n, w.data_ptr(), n, zr.data_ptr() if mode == b"A" else None, n,
                                  n * n, mode, info.data_ptr())
        _lib.check(rc, "eigx_h_batch_dev")

    for mode in (b"A", b"N"):
        ta, tb, tc, td = [], [], [], []
        for rep in range(repeats + 1):   # rep 0 warms the kernels and the workspace pool of every route
            a.copy_(A0)
            b.copy_(B0)
            dt = timed(lambda: loop_call(mode))
            if rep:
                tb.append(dt * batch / L)
            if embed:
                ea.copy_(EA0)
                eb.copy_(EB0)
                dt = timed(lambda: embed_call(mode))
                if rep:
                    tc.append(dt)
            a.copy_(A0)
            dt = timed(lambda: h_batch_call(mode))
            if rep:
                td.append(dt)
            a.copy_(A0)
            b.copy_(B0)
            dt = timed(lambda: batch_call(mode))
            if rep:
                ta.append(dt)
        assert (info == 0).all().item()
        U = torch.triu(b[:L].transpose(1, 2))
        gw = ((w[:L] - wref).abs().amax(dim=1) / (1e-12 * scale)).max().item()
        gf = (torch.linalg.norm(U.conj().transpose(1, 2) @ U - Bk, dim=(1, 2)) / (1e-12 * n * torch.linalg.norm(Bk, dim=(1, 2)))).max().item()
        gr = go = float("nan")
        if mode == b"A":
            Z = z[:L].transpose(1, 2)    # Z[k][:, j] = eigenvector j of pencil k
            wc = w[:L, None, :].to(torch.complex128)
            gr = (torch.linalg.norm(Ak @ Z - Bk @ Z * wc, dim=(1, 2)) / (1e-12 * scale * n)).max().item()
            go = (torch.linalg.norm(Z.conj().transpose(1, 2) @ Bk @ Z - eye, dim=(1, 2)) / (1e-12 * n)).max().item()
        ma = np.median(ta)
        print(f"{n:>4} {batch:>7}  {mode.decode()}    {cell(ta)}  {cell(tb):>38}  {cell(tc) if embed else '-':>38}  {cell(td)}  "
              f"{np.median(tb) / ma:>8.1f}  {(f'{np.median(tc) / ma:.2f}' if embed else '-'):>6}  {ma / np.median(td):>6.2f}  "
              f"{ma * 1e6 / batch:>11.3f}  {gw:.2e} {gr:.2e} {go:.2e} {gf:.2e}", flush=True)
    del A0, B0, a, b, z, w, info, ar, br, zr, Ak, Bk
    if embed:
        del EA0, EB0, ea, eb, ez, ew
    torch.cuda.empty_cache()
lib.eigx_free()
