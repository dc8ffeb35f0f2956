"""Timing of the Hermitian range solves (an extension: eigen_h_range / eigen_h_range_v / KMATH_EIGEN_HGEV_RANGE_V) on one
GPU, device API, against the routes to the same answers without them.  One process per configuration: the driver starts a
fresh child for each and relays its lines; in a child every call alternates with the one it is compared with, after one
warm-up each, and the median of the repeats is printed with min .. max.
usage: gpu_h_range_time.py [--repeats R] [--kinds index,value,hgev] [--m M,M,..] [N ...]     (default 8192 16384; m = 64, 512, n/10)
       gpu_h_range_time.py --one KIND N M WHERE R     a single configuration (what the driver starts); WHERE = low | mid
  index  eigx_h_range_dev on the window [1, m] (low) or [n/2, n/2 + m - 1] (mid), once with eigx_tune key 17 = 100 (subset
         path) and once with key 17 = 0 (full D&C, the window a pointer offset), against eigx_h_dev with nvec = iu; the path
         taken and the stage split (bisection, inverse iteration, orthonormalisation + Rayleigh-Ritz or D&C,
         back-transformation; the reduction is the rest) are printed.
  value  eigx_h_range_v_dev (automatic key 17) against the pair it replaces: eigx_h_dev mode 'N' followed by eigx_h_dev with
         nvec = iu.  The bounds are mid-gap points of a first mode-'N' solve; m and il are checked.
  hgev   eigx_hgev_range_v_dev against eigx_hgev_range_dev on the same window (the index entry runs eigen_h with nvec = iu)."""
import ctypes as C
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

args = sys.argv[1:]
if args[:1] != ["--one"]:
    repeats, kinds, ms = 3, ["index", "value", "hgev"], None
    while args and args[0].startswith("--"):
        if args[0] == "--repeats":
            repeats = int(args[1])
        elif args[0] == "--kinds":
            kinds = args[1].split(",")
        elif args[0] == "--m":
            ms = [int(v) for v in args[1].split(",")]
        else:
            raise SystemExit(f"unknown option {args[0]}")
        args = args[2:]
    for n in [int(v) for v in args] or [8192, 16384]:
        for kind in kinds:
            for m in ms or [64, 512, n // 10]:
                for where in ("low", "mid"):
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", kind, str(n), str(m), where, str(repeats)])
                    if r.returncode != 0:     # nothing more is started on the GPU after a failure
                        raise SystemExit(f"configuration {kind} n={n} m={m} {where} ended with status {r.returncode}")
    sys.exit(0)

import numpy as np
import torch

from eigenexa_amd import _lib

kind, n, m, where, repeats = args[1], int(args[2]), int(args[3]), args[4], int(args[5])
il = 1 if where == "low" else n // 2
iu = il + m - 1
lib = _lib.load()
_lib.check(lib.eigx_init(0), "init")
dev = torch.device("cuda:0")
t4 = np.zeros(4)
t4p = t4.ctypes.data_as(C.POINTER(C.c_double))
eps = np.finfo(np.float64).eps
MF, MB = 48, 128
ld = n + 2
g = torch.Generator(device=dev)
g.manual_seed(n)
S = torch.randn(n, n, dtype=torch.complex128, device=dev, generator=g)
A = (S + S.conj().T) / 2
del S
a = torch.zeros(n, ld, dtype=torch.complex128, device=dev)
z = torch.zeros(iu, ld, dtype=torch.complex128, device=dev)
w = torch.zeros(n, dtype=torch.float64, device=dev)
wr = torch.zeros(m, dtype=torch.float64, device=dev)
mv, ilv = C.c_int(), C.c_int()


def timed(fn, fill=None):
    (fill or load_a)()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = fn()
    torch.cuda.synchronize()
    _lib.check(rc, "solve")
    return time.perf_counter() - t0


def load_a():
    a[:, :n] = A.T


def ms_(ts):
    t = np.array(ts) * 1e3
    return np.median(t), f"{np.median(t):.1f} ms [{t.min():.1f} .. {t.max():.1f}]"


def info():
    path, mm, cond = C.c_int(), C.c_int(), C.c_double()
    lib.eigx_range_info(C.byref(path), C.byref(mm), C.byref(cond))
    lib.eigx_range_timers(t4p)
    return path.value, cond.value, t4.copy()


def gates(Zt, wv):
    Z = Zt[:, :n].T
    res = torch.linalg.norm(A @ Z - Z * wv.to(torch.complex128)[None, :]).item() / (n * eps * torch.linalg.norm(A).item())
    orth = torch.linalg.norm(Z.conj().T @ Z - torch.eye(Z.shape[1], dtype=torch.complex128, device=dev)).item() / (n * eps)
    return f"residual {res:.2e} unitarity {orth:.2e}"


def full(nvec, mode):
    return lambda: lib.eigx_h_dev(n, nvec, a.data_ptr(), ld, w.data_ptr(), z.data_ptr(), ld, MF, MB, mode)


def rng():
    return lib.eigx_h_range_dev(n, il, iu, a.data_ptr(), ld, wr.data_ptr(), z.data_ptr(), ld, MF, MB, b"A")


head = f"{kind} n={n} [{il}, {iu}] m={m}"
if kind == "index":
    tf, tr, st = [], {100: [], 0: []}, {100: [], 0: []}
    note = {}
    for rep in range(repeats + 1):   # rep 0 warms the workspace pool and the kernels of all three
        dt = timed(full(iu, b"A"))
        if rep:
            tf.append(dt)
        for key17 in (100, 0):
            old = lib.eigx_tune(17, key17)
            dt = timed(rng)
            lib.eigx_tune(17, old)
            path, cond, t = info()
            if rep:
                tr[key17].append(dt)
                st[key17].append(t)
            else:
                note[key17] = f"path {path} cond(L) {cond:.3g} {gates(z[:m], wr)}"
    f, fs = ms_(tf)
    print(f"{head}: eigx_h_dev nvec=iu {fs}  held {lib.eigx_held_bytes() / 2**20:.0f} MiB", flush=True)
    for key17, name in ((100, "subset"), (0, "full D&C")):
        r, rs = ms_(tr[key17])
        s = np.median(np.array(st[key17]), axis=0) * 1e3
        print(f"{head}: eigx_h_range_dev {name} {rs}  ratio {r / f:.2f}  | {note[key17]}  bisection {s[0]:.1f}  inverse iteration "
              f"{s[1]:.1f}  orth + Rayleigh-Ritz / D&C {s[2]:.1f}  back-transformation {s[3]:.1f}", flush=True)
elif kind == "value":
    timed(full(n, b"N"))
    wh = w.cpu().numpy()
    vl = float(wh[0] - (wh[-1] - wh[0])) if il == 1 else float(0.5 * (wh[il - 2] + wh[il - 1]))
    vu = float(0.5 * (wh[iu - 1] + wh[iu]))
    tp, tv = [], []
    for rep in range(repeats + 1):
        dt = timed(full(n, b"N")) + timed(full(iu, b"A"))
        if rep:
            tp.append(dt)
        dt = timed(lambda: lib.eigx_h_range_v_dev(n, vl, vu, m, C.byref(mv), C.byref(ilv), a.data_ptr(), ld, wr.data_ptr(),
                                                   z.data_ptr(), ld, MF, MB, b"A"))
        assert (mv.value, ilv.value) == (m, il), (mv.value, ilv.value)
        if rep:
            tv.append(dt)
    path, cond, _ = info()
    p, ps = ms_(tp)
    v, vs = ms_(tv)
    print(f"{head}: 'N' solve + nvec=iu solve {ps}  eigx_h_range_v_dev {vs}  ratio {v / p:.2f}  | path {path} {gates(z[:m], wr)}",
          flush=True)
elif kind == "hgev":
    X = torch.randn(n, n, dtype=torch.complex128, device=dev, generator=g)
    B = X @ X.conj().T / n + torch.eye(n, dtype=torch.complex128, device=dev)
    B = (B + B.conj().T) / 2
    del X
    b = torch.zeros(n, ld, dtype=torch.complex128, device=dev)

    def load_ab():
        a[:, :n] = A.T
        b[:, :n] = B.T

    def by_index(lo, hi, mode):
        return lambda: lib.eigx_hgev_range_dev(n, lo, hi, a.data_ptr(), ld, b.data_ptr(), ld, w.data_ptr(), z.data_ptr(), ld, mode)

    timed(by_index(1, n, b"N"), load_ab)
    wh = w.cpu().numpy()
    vl = float(wh[0] - (wh[-1] - wh[0])) if il == 1 else float(0.5 * (wh[il - 2] + wh[il - 1]))
    vu = float(0.5 * (wh[iu - 1] + wh[iu]))
    ti, tv = [], []
    for rep in range(repeats + 1):
        dt = timed(by_index(il, iu, b"A"), load_ab)
        if rep:
            ti.append(dt)
        dt = timed(lambda: lib.eigx_hgev_range_v_dev(n, vl, vu, m, C.byref(mv), C.byref(ilv), a.data_ptr(), ld, b.data_ptr(), ld,
                                                      wr.data_ptr(), z.data_ptr(), ld, b"A"), load_ab)
        assert (mv.value, ilv.value) == (m, il), (mv.value, ilv.value)
        if rep:
            tv.append(dt)
    path, cond, _ = info()
    Z = z[:m, :n].T
    scale = max(1.0, wr.abs().max().item())
    res = torch.linalg.norm(A @ Z - (B @ Z) * wr.to(torch.complex128)[None, :]).item() / (scale * n)
    orth = torch.linalg.norm(Z.conj().T @ B @ Z - torch.eye(m, dtype=torch.complex128, device=dev)).item() / n
    i, is_ = ms_(ti)
    v, vs = ms_(tv)
    print(f"{head}: eigx_hgev_range_dev {is_}  eigx_hgev_range_v_dev {vs}  ratio {v / i:.2f}  | inner path {path}  "
          f"|AZ - BZW|_F / (scale n) = {res:.2e}  |Z^H B Z - I|_F / n = {orth:.2e}  (< 1e-12)", flush=True)
else:
    raise SystemExit(f"unknown kind {kind}")
lib.eigx_free()
