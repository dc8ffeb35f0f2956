"""Timing of KMATH_EIGEN_HGEV (an extension: the complex Hermitian generalised problem) on one GPU, device API, with
KMATH_EIGEN_GEV and eigen_h at the same N for comparison.  usage: gpu_hgev_time.py [N ...]   (default 4096 8192)
Prints the five timers (total, eigen_h(B), forming C, eigen_h(C), Z = F Y), the complex-GEMM rate of the three products
(8 n^3 per full complex product, 4 n^3 for the upper-tile product C = F^H T) and the residual gates."""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from eigenexa_amd import _lib

sizes = [int(v) for v in sys.argv[1:]] or [4096, 8192]
lib = _lib.load()
_lib.check(lib.eigx_init(0), "init")
dev = torch.device("cuda:0")
tm = np.zeros(16)
tp = tm.ctypes.data_as(C.POINTER(C.c_double))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    lib.eigx_get_timers(tp)
    return rc, dt, tm.copy()


for n in sizes:
    g = torch.Generator(device=dev)
    g.manual_seed(n)
    S = torch.randn(n, n, dtype=torch.complex128, device=dev, generator=g)
    A = (S + S.conj().T) / 2
    X = torch.randn(n, n, dtype=torch.complex128, device=dev, generator=g)
    B = X @ X.conj().T / n + torch.eye(n, dtype=torch.complex128, device=dev)
    B = (B + B.conj().T) / 2
    del S, X
    for rep in range(2):   # rep 0 warms the workspace pool and the kernels
        a, b = A.T.contiguous(), B.T.contiguous()
        z = torch.zeros(n, n, dtype=torch.complex128, device=dev)
        w = torch.zeros(n, dtype=torch.float64, device=dev)
        rc, dt, t = timed(lambda: lib.eigx_hgev_dev(n, a.data_ptr(), n, b.data_ptr(), n, w.data_ptr(), z.data_ptr(), n))
        _lib.check(rc, "hgev")
    del a, b
    prod = t[2] + t[4]
    print(f"KMATH_EIGEN_HGEV n={n}: total {t[0]*1e3:.1f} ms (wall {dt*1e3:.1f})  eigen_h(B) {t[1]*1e3:.1f}  form C {t[2]*1e3:.1f}  "
          f"eigen_h(C) {t[3]*1e3:.1f}  Z=FY {t[4]*1e3:.1f}  | products {prod*1e3:.1f} ms, {20.0*n**3/prod/1e12:.1f} TFLOP/s "
          f"(20 n^3), Z=FY alone {8.0*n**3/t[4]/1e12:.1f} TFLOP/s", flush=True)
    Z = z.T
    wc = w.to(torch.complex128)
    scale = max(1.0, w.abs().max().item())
    res = torch.linalg.norm(A @ Z - (B @ Z) * wc[None, :]).item() / (scale * n)
    orth = torch.linalg.norm(Z.conj().T @ B @ Z - torch.eye(n, dtype=torch.complex128, device=dev)).item() / n
    print(f"  gates: |AZ - BZW|_F / (scale n) = {res:.2e} (< 1e-12)   |Z^H B Z - I|_F / n = {orth:.2e} (< 1e-12)", flush=True)
    del z, Z
    # the same N through eigen_h (A alone) and KMATH_EIGEN_GEV (real symmetric A, B)
    for rep in range(2):
        a = A.T.contiguous()
        z = torch.zeros(n, n, dtype=torch.complex128, device=dev)
        rc, dt, t = timed(lambda: lib.eigx_h_dev(n, n, a.data_ptr(), n, w.data_ptr(), z.data_ptr(), n, 48, 128, b"X"))
        _lib.check(rc, "eigen_h")
    print(f"eigen_h (mode X) n={n}: total {t[0]*1e3:.1f} ms (wall {dt*1e3:.1f})", flush=True)
    del a, z, A, B
    Ar, Br = torch.randn(n, n, dtype=torch.float64, device=dev, generator=g), torch.randn(n, n, dtype=torch.float64, device=dev, generator=g)
    Ar = (Ar + Ar.T) / 2
    Br = Br @ Br.T / n + torch.eye(n, dtype=torch.float64, device=dev)
    for rep in range(2):
        a, b = Ar.T.contiguous(), ((Br + Br.T) / 2).T.contiguous()
        z = torch.zeros(n, n, dtype=torch.float64, device=dev)
        rc, dt, t = timed(lambda: lib.eigx_gev_dev(n, a.data_ptr(), n, b.data_ptr(), n, w.data_ptr(), z.data_ptr(), n))
        _lib.check(rc, "gev")
    print(f"KMATH_EIGEN_GEV n={n}: total {t[0]*1e3:.1f} ms (wall {dt*1e3:.1f})  eigen_s(B) {t[1]*1e3:.1f}  form C {t[2]*1e3:.1f}  "
          f"eigen_s(C) {t[3]*1e3:.1f}  Z=FY {t[4]*1e3:.1f}", flush=True)
    del a, b, z, Ar, Br
    torch.cuda.empty_cache()
lib.eigx_free()
