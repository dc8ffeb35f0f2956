"""Timing of the windowed batched complex generalised eigensolve (an extension: eigx_hgev_batch_range_dev, csrc/hgbatch_range.hip)
on one GPU, device API, complex pencils after tools/gpu_gbatch_range_time.py (A = R + R^H, B = G G^H / n + 0.1 I with complex
Gaussian R and G), the lowest m pairs: for every cell (n, batch, mode, m) the window kernel (route 1: eigx_tune key 26 = 1), the
full batch solve with a slice (route 2: key 26 = 2, the baseline: the kernel of eigx_hgev_batch and a gather) and the plain
eigx_hgev_batch_dev full solve, the yardstick.
usage: gpu_hgbatch_range_time.py [--repeats R] [--check L] [n:batch ...]
(default 8:100000 16:50000 32:10000 48:4000 64:4000; windows: the lowest m of {1, 4, 16} at n <= 32 and of {1, 4, 8} above, the
widest the n-class serves in mode 'A'; modes 'A' and 'N', mode 'N' also with m = n)
The three alternate in one process after one warm-up each; every call is timed whole (host clock around the call, which returns
after the result is complete).  Printed: the medians and the spread over the repeats, the ratio route 2 / route 1 (above 1:
route 1 is faster), what the automatic rule (key 26 = 0) takes for the cell, the pencils sent to the redo, and the gates on the
first L pencils of route 1's result (mode 'A': ||A Z - B Z W||_F / (scale n) and ||Z^H B Z - I||_F / n in units of 1e-12, the gates
of tests/test_hgbatch.py; mode 'N': |w - w_ref| / scale in the same unit, w_ref from torch's Cholesky and eigvalsh;
scale = max(1, max|w_ref|)).  One n:batch row per run keeps every row under a time limit of its own."""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from eigenexa_amd import _lib

args = sys.argv[1:]
repeats, ncheck = 5, 200
while args and args[0].startswith("--"):
    if args[0] == "--repeats":
        repeats = int(args[1])
    elif args[0] == "--check":
        ncheck = int(args[1])
    else:
        raise SystemExit(f"unknown option {args[0]}")
    args = args[2:]
cases = [tuple(int(v) for v in s.split(":")) for s in args] or [(8, 100000), (16, 50000), (32, 10000), (48, 4000), (64, 4000)]
lib = _lib.load()
_lib.check(lib.eigx_init(0), "init")
dev = torch.device("cuda:0")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def info_of_last_call():
    r, m, d = C.c_int(), C.c_int(), C.c_int()
    _lib.check(lib.eigx_batch_range_info(C.byref(r), C.byref(m), C.byref(d)), "eigx_batch_range_info")
    return r.value, m.value, d.value


def cgauss(batch, n, g):
    return torch.complex(torch.randn(batch, n, n, dtype=torch.float64, device=dev, generator=g),
                         torch.randn(batch, n, n, dtype=torch.float64, device=dev, generator=g))


print(f"{'n':>4} {'batch':>7} mode {'m':>4}  {'route 1 ms':>28}  {'route 2 ms':>28}  {'eigx_hgev_batch_dev ms':>28}  {'r2 / r1':>7}  "
      f"{'full / r1':>9}  auto  redone  gates", flush=True)
for n, batch in cases:
    g = torch.Generator(device=dev)
    g.manual_seed(1000 + n)
    R = cgauss(batch, n, g)
    A0 = R + R.mH
    R = cgauss(batch, n, g)
    B0 = R @ R.mH / n + 0.1 * torch.eye(n, dtype=torch.complex128, device=dev)
    B0 = 0.5 * (B0 + B0.mH)
    del R
    aimg = A0.transpose(1, 2).contiguous()   # the column-major image of A0[k]: aimg[k][j][i] = A0[k][i][j], interleaved complex
    bimg = B0.transpose(1, 2).contiguous()
    a = torch.empty_like(aimg)
    b = torch.empty_like(bimg)
    zf = torch.zeros_like(aimg)
    wf = torch.zeros(batch, n, dtype=torch.float64, device=dev)
    info = torch.zeros(batch, dtype=torch.int32, device=dev)
    L = min(ncheck, batch)
    Lc = torch.linalg.cholesky(B0[:L])
    X = torch.linalg.solve_triangular(Lc, A0[:L], upper=False)
    wl = torch.linalg.eigvalsh(torch.linalg.solve_triangular(Lc, X.mH, upper=False))
    scale = wl.abs().amax(dim=1).clamp(min=1.0)
    del Lc, X
    wide = 16 if n <= 32 else 8              # the widest window of mode 'A' in the n-class
    for mode in (b"A", b"N"):
        widths = sorted({1, min(n, 4), min(n, wide)} | ({n} if mode == b"N" else set()))
        for m in widths:
            z = torch.zeros(batch, m, n, dtype=torch.complex128, device=dev)
            w = torch.zeros(batch, m, dtype=torch.float64, device=dev)

            def window_call(route):
                old = lib.eigx_tune(26, route)
                rc = lib.eigx_hgev_batch_range_dev(n, batch, 1, m, a.data_ptr(), n, n * n, b.data_ptr(), n, n * n, w.data_ptr(), m,
                                                   z.data_ptr() if mode == b"A" else None, n, n * m, mode, info.data_ptr())
                lib.eigx_tune(26, old)
                _lib.check(rc, "eigx_hgev_batch_range_dev")

            def full_call():
                rc = lib.eigx_hgev_batch_dev(n, batch, a.data_ptr(), n, n * n, b.data_ptr(), n, n * n, wf.data_ptr(), n,
                                             zf.data_ptr() if mode == b"A" else None, n, n * n, mode, info.data_ptr())
                _lib.check(rc, "eigx_hgev_batch_dev")

            a.copy_(aimg)
            b.copy_(bimg)
            window_call(0)                   # what the automatic rule takes for this cell
            auto = info_of_last_call()[0]
            t1, t2, tf = [], [], []
            for rep in range(repeats + 1):   # rep 0 warms the kernels and the workspace pool of all three
                for fn, acc in ((lambda: window_call(2), t2), (full_call, tf), (lambda: window_call(1), t1)):
                    a.copy_(aimg)
                    b.copy_(bimg)
                    dt = timed(fn)
                    if rep:
                        acc.append(dt)
            route, mm, redone = info_of_last_call()      # (route 1 ran last: w and z hold its result)
            assert route == 1 and mm == m and (info == 0).all().item()
            if mode == b"A":
                Z = z[:L].transpose(1, 2)    # Z[k][:, j] = eigenvector j of the window of pencil k
                Ak, Bk = A0[:L], B0[:L]
                res = (torch.linalg.norm(Ak @ Z - (Bk @ Z) * w[:L, None, :], dim=(1, 2)) / (scale * n)).max().item() * 1e12
                orth = (torch.linalg.norm(Z.mH @ Bk @ Z - torch.eye(m, dtype=torch.complex128, device=dev), dim=(1, 2))
                        / n).max().item() * 1e12
                gates = f"{res:.2e} {orth:.2e}"
                assert res < 1.0 and orth < 1.0
            else:
                werr = ((w[:L] - wl[:, :m]).abs().amax(dim=1) / scale).max().item() * 1e12
                gates = f"{werr:.2e}"
                assert werr < 1.0
            b1, b2, bf = np.array(t1) * 1e3, np.array(t2) * 1e3, np.array(tf) * 1e3
            print(f"{n:>4} {batch:>7}  {mode.decode()}   {m:>4}  {np.median(b1):>9.3f} [{b1.min():>7.3f} .. {b1.max():>8.3f}]  "
                  f"{np.median(b2):>9.3f} [{b2.min():>7.3f} .. {b2.max():>8.3f}]  {np.median(bf):>9.3f} [{bf.min():>7.3f} .. {bf.max():>8.3f}]  "
                  f"{np.median(b2) / np.median(b1):>7.2f}  {np.median(bf) / np.median(b1):>9.2f}  {auto:>4}  {redone:>6}  {gates}", flush=True)
            del z, w
    del A0, B0, aimg, bimg, a, b, zf, wf, info
    torch.cuda.empty_cache()
lib.eigx_free()
