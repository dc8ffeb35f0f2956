"""Timing of KMATH_EIGEN_HGEV_RANGE (an extension: the Cholesky-route complex generalised range solver) against
KMATH_EIGEN_HGEV in the same process on the same pencil, one GPU, device API.
usage: gpu_hgev_range_time.py [N ...]          (default 4096 8192) the table: eigx_hgev_dev and eigx_hgev_range_dev with the
                                               windows [1, n] and [1, n/10] (mode 'A') and [1, n] mode 'N' alternate; one
                                               warm-up, then the median of REPS timed repeats, min .. max logged
       gpu_hgev_range_time.py --one N          a single full-window call and nothing else (for a kernel trace)
Timers of both solvers: [0] total [1] factorisation / eigen_h(B) [2] forming C [3] the inner eigen_h [4] back-substitution /
Z = F Y."""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from eigenexa_amd import _lib

REPS = 5
args = sys.argv[1:]
one = args[:1] == ["--one"]
sizes = [int(v) for v in (args[1:] if one else args)] or [4096, 8192]
lib = _lib.load()
_lib.check(lib.eigx_init(0), "init")
dev = torch.device("cuda:0")
tm = np.zeros(16)
tp = tm.ctypes.data_as(C.POINTER(C.c_double))


def pencil(n):
    g = torch.Generator(device=dev)
    g.manual_seed(n)
    S = torch.randn(n, n, dtype=torch.complex128, device=dev, generator=g)
    A = (S + S.conj().T) / 2
    X = torch.randn(n, n, dtype=torch.complex128, device=dev, generator=g)
    B = X @ X.conj().T / n + torch.eye(n, dtype=torch.complex128, device=dev)
    return A, (B + B.conj().T) / 2


class Bench:
    def __init__(self, n):
        self.n, self.ld = n, n + 2
        self.A, self.B = pencil(n)
        self.a = torch.zeros(n, self.ld, dtype=torch.complex128, device=dev)
        self.b = torch.zeros(n, self.ld, dtype=torch.complex128, device=dev)
        self.z = torch.zeros(n, self.ld, dtype=torch.complex128, device=dev)
        self.w = torch.zeros(n, dtype=torch.float64, device=dev)

    def call(self, what, iu=None, mode=b"A"):
        n, ld = self.n, self.ld
        self.a[:, :n] = self.A.T
        self.b[:, :n] = self.B.T
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if what == "hgev":
            rc = lib.eigx_hgev_dev(n, self.a.data_ptr(), ld, self.b.data_ptr(), ld, self.w.data_ptr(), self.z.data_ptr(), ld)
        else:
            rc = lib.eigx_hgev_range_dev(n, 1, iu, self.a.data_ptr(), ld, self.b.data_ptr(), ld, self.w.data_ptr(),
                                         self.z.data_ptr(), ld, mode)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        _lib.check(rc, what)
        lib.eigx_get_timers(tp)
        return dt, tm[:5].copy()

    def gates(self, m):
        n = self.n
        Z, w = self.z[:m, :n].T, self.w[:m]
        scale = max(1.0, w.abs().max().item())
        res = torch.linalg.norm(self.A @ Z - (self.B @ Z) * w.to(torch.complex128)[None, :]).item() / (scale * n)
        orth = torch.linalg.norm(Z.conj().T @ self.B @ Z - torch.eye(m, dtype=torch.complex128, device=dev)).item() / n
        return res, orth


def row(label, samples):
    wall = np.array([s[0] for s in samples]) * 1e3
    t = np.array([s[1] for s in samples]) * 1e3
    med, lo, hi = np.median(t, axis=0), t.min(axis=0), t.max(axis=0)
    print(f"  {label:<30s} total {med[0]:8.1f} ms ({lo[0]:.1f} .. {hi[0]:.1f})  wall {np.median(wall):8.1f}  stages " +
          "  ".join(f"{med[q]:7.1f}" for q in range(1, 5)), flush=True)
    return med


if one:
    bn = Bench(sizes[0])
    dt, t = bn.call("hgevr", bn.n)
    print(f"single eigx_hgev_range_dev n={bn.n} [1, n]: wall {dt * 1e3:.1f} ms, timers " + " ".join(f"{v * 1e3:.1f}" for v in t))
    lib.eigx_free()
    sys.exit(0)

for n in sizes:
    bn = Bench(n)
    cases = [("eigx_hgev_dev", ("hgev",)), ("eigx_hgev_range_dev [1, n]", ("hgevr", n)),
             ("eigx_hgev_range_dev [1, n/10]", ("hgevr", n // 10)), ("eigx_hgev_range_dev 'N' [1, n]", ("hgevr", n, b"N"))]
    for _, c in cases:      # warm-up: workspace pool, kernels, clocks
        bn.call(*c)
    samples = {k: [] for k, _ in cases}
    for rep in range(REPS):  # the solvers alternate
        for k, c in cases:
            samples[k].append(bn.call(*c))
            if rep == 0 and c[0] == "hgevr" and len(c) == 2:
                res, orth = bn.gates(c[1])
                print(f"  gates n={n} [1, {c[1]}]: |AZ - BZW|_F / (scale n) = {res:.2e}  |Z^H B Z - I|_F / n = {orth:.2e}  (< 1e-12)")
    nb = lib.eigx_tune(20, 256)
    lib.eigx_tune(20, nb)
    print(f"n = {n}, ld = {bn.ld}, NB = {nb}: median of {REPS} (min .. max); stages = "
          "factor B | form C | inner solve | back-substitution")
    med = {k: row(k, samples[k]) for k, _ in cases}
    g, r = med["eigx_hgev_dev"], med["eigx_hgev_range_dev [1, n]"]
    print(f"  whole call [1, n] / eigx_hgev_dev: {r[0] / g[0]:.3f}   triangular stages 1+2+4: {r[1] + r[2] + r[4]:.1f} ms "
          f"against eigen_h(B) + products {g[1] + g[2] + g[4]:.1f} ms", flush=True)
    del bn
    torch.cuda.empty_cache()
lib.eigx_free()
