"""Timing of the ragged batched generalised eigensolves (an extension: eigx_gev_vbatch_dev, eigx_hgev_vbatch_dev;
csrc/gvbatch.hip, csrc/hgbatch.hip) on one GPU, device API, against the routes a caller has without them.
usage: gpu_gvbatch_time.py [--repeats R] [--loop L] [--gate G]
Size distributions (pencils packed tightly, lda = ldb = ldz = n; A random symmetric / Hermitian, B random and diagonally
dominant with the diagonal n):
  uniform   4096 pencils, n uniform in 1 .. top (top = 96 for _gev_, 64 for _hgev_)
  sectors   min(C(12, j), top), j = 0 .. 12, repeated 250 times (3250 pencils): a few sizes at the cutoff dominate
  n = 64    4000 pencils of n = 64
  n = 1     4000 pencils of n = 1: next to no arithmetic, so (a) against (d) shows what the schedule and the descriptors cost
for eigx_gev_vbatch in modes 'A' and 'N' and for eigx_hgev_vbatch in mode 'A'.  Routes, alternating in one process after one
warm-up each, median and [min .. max] over R repeats (default 5):
  (a)  the ragged call
  (b)  a loop of eigx_*gev_batch_dev(n_k, 1, ...) on the pencils in place, timed over the first L pencils (default 512) and scaled
  (c)  caller-side grouping: per distinct n device gathers of its blocks of a and of b into strided buffers, one
       eigx_*gev_batch_dev call, and device scatters of w and z back (U is left in the gathered buffer: scattering it back as
       well would add to this route); the index tensors are made beforehand, the copies are timed
  (d)  on the two one-size rows only: eigx_*gev_batch_dev itself on the same buffers
and the gates of tests/test_gbatch.py in units of each gate (eigenvalues against scipy.linalg.eigh, residual, B-orthogonality;
mode 'N': eigenvalues only), worst over the first G pencils (default 200) of route (a)."""
import os
import sys
import time
from math import comb

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.linalg
import torch

from eigenexa_amd import _lib, layout

args = sys.argv[1:]
repeats, nloop, ngate = 5, 512, 200
while args:
    if args[0] == "--repeats":
        repeats = int(args[1])
    elif args[0] == "--loop":
        nloop = int(args[1])
    elif args[0] == "--gate":
        ngate = int(args[1])
    else:
        raise SystemExit(f"unknown option {args[0]}")
    args = args[2:]
lib = _lib.load()
_lib.check(lib.eigx_init(0), "init")
dev = torch.device("cuda:0")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def sizes_of(dist, top):
    if dist == "uniform":
        return np.random.default_rng(top).integers(1, top + 1, 4096).astype(np.int32)
    if dist == "sectors":
        return np.tile(np.array([min(comb(12, j), top) for j in range(13)], dtype=np.int32), 250)
    return np.full(4000, int(dist.split("=")[1]), dtype=np.int32)   # "n = 64", "n = 1"


def show(t):
    t = np.array(t) * 1e3
    return f"{np.median(t):>9.2f} [{t.min():>8.2f} .. {t.max():>8.2f}]"


def block(buf, off, v, cs):
    """block of order v at element `off` of a host image as a Hermitian matrix built from its upper triangle"""
    blk = buf[cs * off:cs * (off + v * v)].reshape(v, v, cs)
    U = np.triu((blk[:, :, 0] + (1j * blk[:, :, 1] if cs == 2 else 0.0)).T, 1)
    return U + U.conj().T + np.diag(np.diag(blk[:, :, 0]))


print(f"{'entry':>6} mode {'sizes':>8} {'blocks':>6}  {'(a) ragged call ms':>31}  {'(b) loop, scaled, ms':>31}  "
      f"{'(c) grouping ms':>31}  {'(d) uniform ms':>31}  {'b/a':>6} {'c/a':>6} {'a/d':>6}  a < b, c  gates (w, residual, B-orth)", flush=True)
for which, cs, top, modes in (("gev", 1, 96, (b"A", b"N")), ("hgev", 2, 64, (b"A",))):
    vcall = getattr(lib, f"eigx_{which}_vbatch_dev")
    ucall = getattr(lib, f"eigx_{which}_batch_dev")
    for dist in ("uniform", "sectors", "n = 64", "n = 1"):
        n = sizes_of(dist, top)
        nb = len(n)
        off_a, la = layout.ragged_offsets(n)
        off_w, lw = layout.ragged_offsets(n, ld=1)
        g = torch.Generator(device=dev)
        g.manual_seed(7 + top)
        a0 = torch.rand(cs * la, dtype=torch.float64, device=dev, generator=g) - 0.5   # only the upper triangles are read
        b0 = torch.rand(cs * la, dtype=torch.float64, device=dev, generator=g) - 0.5
        # the diagonal of B: n (its real part), which dominates the at most n - 1 off-diagonal entries of modulus < 0.71 of a row
        n64 = n.astype(np.int64)
        idiag = np.concatenate([off_a[k] + np.arange(n64[k]) * (n64[k] + 1) for k in range(nb)])
        b0[torch.from_numpy(cs * idiag).to(dev)] = torch.from_numpy(np.repeat(n, n).astype(np.float64)).to(dev)
        a, b = torch.empty_like(a0), torch.empty_like(b0)
        z = torch.zeros_like(a0)
        w = torch.zeros(lw, dtype=torch.float64, device=dev)
        info = torch.zeros(nb, dtype=torch.int32, device=dev)
        L = min(nloop, nb)
        # route (c): per distinct n the places of its blocks' elements in a / b / z (doubles) and in w, made beforehand
        groups = []
        for v in np.unique(n):
            ks = np.nonzero(n == v)[0]
            ia = torch.from_numpy(cs * off_a[ks][:, None] + np.arange(cs * int(v) * int(v))[None, :]).to(dev).reshape(-1)
            iw = torch.from_numpy(off_w[ks][:, None] + np.arange(int(v))[None, :]).to(dev).reshape(-1)
            groups.append((int(v), len(ks), ia, iw))

        def ragged(mode):
            want = mode == b"A"
            rc = vcall(nb, n.ctypes.data, a.data_ptr(), off_a.ctypes.data, n.ctypes.data, b.data_ptr(), off_a.ctypes.data,
                       n.ctypes.data, w.data_ptr(), off_w.ctypes.data, z.data_ptr() if want else None,
                       off_a.ctypes.data if want else None, n.ctypes.data if want else None, mode, info.data_ptr())
            _lib.check(rc, "gvbatch")

        def loop(mode):
            pa, pb, pw, pz = a.data_ptr(), b.data_ptr(), w.data_ptr(), z.data_ptr()
            for k in range(L):
                v, o = int(n[k]), 8 * cs * int(off_a[k])
                rc = ucall(v, 1, pa + o, v, 0, pb + o, v, 0, pw + 8 * int(off_w[k]), v, (pz + o) if mode == b"A" else None, v, 0, mode,
                           None)
                _lib.check(rc, "batch, one pencil")

        def grouped(mode):
            for v, cnt, ia, iw in groups:
                ab, bb = a.take(ia), b.take(ia)
                wb = torch.empty(cnt * v, dtype=torch.float64, device=dev)
                zb = torch.empty_like(ab) if mode == b"A" else None
                rc = ucall(v, cnt, ab.data_ptr(), v, v * v, bb.data_ptr(), v, v * v, wb.data_ptr(), v,
                           zb.data_ptr() if zb is not None else None, v, v * v, mode, None)
                _lib.check(rc, "batch, one size")
                w.put_(iw, wb)
                if zb is not None:
                    z.put_(ia, zb)

        def uniform(mode):
            v = int(n[0])
            rc = ucall(v, nb, a.data_ptr(), v, v * v, b.data_ptr(), v, v * v, w.data_ptr(), v, z.data_ptr() if mode == b"A" else None,
                       v, v * v, mode, info.data_ptr())
            _lib.check(rc, "batch")

        routes = [("b", loop), ("c", grouped)] + ([("d", uniform)] if dist.startswith("n =") else []) + [("a", ragged)]
        for mode in modes:
            t = {name: [] for name, _ in routes}
            for rep in range(repeats + 1):   # rep 0 warms the kernels and the workspace pool of every route
                for name, fn in routes:      # (a) last: the gates below are taken from its result
                    a.copy_(a0)
                    b.copy_(b0)
                    dt = timed(lambda: fn(mode))
                    if rep:
                        t[name].append(dt * (nb / L if name == "b" else 1.0))
            assert (info == 0).all().item()
            G = min(ngate, nb)
            wh, zh, ah, bh = w.cpu().numpy(), z.cpu().numpy(), a0.cpu().numpy(), b0.cpu().numpy()
            gw = gres = gorth = 0.0
            for k in range(G):
                v = int(n[k])
                A, B = block(ah, off_a[k], v, cs), block(bh, off_a[k], v, cs)
                wk = wh[off_w[k]:off_w[k] + v]
                wref = scipy.linalg.eigh(A, B, eigvals_only=True)
                scale = max(1.0, np.abs(wref).max())
                gw = max(gw, np.abs(wk - wref).max() / (1e-12 * scale))
                if mode == b"A":
                    zz = zh[cs * off_a[k]:cs * (off_a[k] + v * v)].reshape(v, v, cs)
                    Z = (zz[:, :, 0] + (1j * zz[:, :, 1] if cs == 2 else 0.0)).T
                    gres = max(gres, np.linalg.norm(A @ Z - B @ Z * wk) / (1e-12 * scale * v))
                    gorth = max(gorth, np.linalg.norm(Z.conj().T @ B @ Z - np.eye(v)) / (1e-12 * v))
                else:
                    gres = gorth = float("nan")
            med = {name: np.median(v) for name, v in t.items()}
            wins = max(t["a"]) < min(t["b"]) and max(t["a"]) < min(t["c"])
            print(f"{which:>6}  {mode.decode()}   {dist:>8} {nb:>6}  {show(t['a'])}  {show(t['b'])}  {show(t['c'])}  "
                  f"{show(t['d']) if 'd' in t else '':>31}  {med['b'] / med['a']:>6.1f} {med['c'] / med['a']:>6.1f} "
                  f"{(med['a'] / med['d']) if 'd' in t else float('nan'):>6.3f}  {str(wins):>8}  {gw:.2e} {gres:.2e} {gorth:.2e}", flush=True)
        del a0, b0, a, b, z, w, info, groups
        torch.cuda.empty_cache()
lib.eigx_free()
