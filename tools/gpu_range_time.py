"""Timing of the index-range solves (an extension: eigen_sx_range / eigen_s_range) on one GPU, device API, against the
route to the same answer without them: eigx_sx_dev / eigx_s_dev with nvec = m (the lowest m pairs; the full divide and
conquer, trimmed back-transformation).  usage: gpu_range_time.py [--repeats R] [--m M,M,..] [N ...]   (default 8192 32768)
Both run in the same process, alternating, after one warm-up each; the spread over the repeats is printed, and for the
range call the path taken, the stage split (bisection, inverse iteration, orthonormalisation + Rayleigh-Ritz,
back-transformation; the reduction is the rest) and eigx_held_bytes().  The size rule (eigx_tune key 17) is switched off
here so that every window takes the subset path.
--by-value: each window is also timed through the value-window entries (eigx_sx_range_v_dev / eigx_s_range_v_dev).  The
bounds are mid-gap points around the window in the eigenvalues of a first mode-'N' solve, so both calls solve the same
window (checked: m, il and bit-identical w); the line gains the value call's time and its difference to the index call.
--count: after each size's timings, eigx_band_count_dev alone on the band matrix of that size, both bands, npts = 2 (what a
value call adds) and 4096 (a density-of-states histogram), median of 20 calls.
--no-full: the nvec = m route is not timed (A/B runs of the range entries against another build, EIGX_LIB)."""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from eigenexa_amd import _lib, layout

args = sys.argv[1:]
repeats, ms = 3, [64, 512, 4096]
by_value = count_stage = no_full = False
while args and args[0].startswith("--"):
    if args[0] in ("--by-value", "--count", "--no-full"):
        by_value, count_stage, no_full = (by_value or args[0] == "--by-value", count_stage or args[0] == "--count",
                                          no_full or args[0] == "--no-full")
        args = args[1:]
        continue
    if args[0] == "--repeats":
        repeats = int(args[1])
    elif args[0] == "--m":
        ms = [int(v) for v in args[1].split(",")]
    else:
        raise SystemExit(f"unknown option {args[0]}")
    args = args[2:]
sizes = [int(v) for v in args] or [8192, 32768]
lib = _lib.load()
_lib.check(lib.eigx_init(0), "init")
lib.eigx_tune(17, 100)
dev = torch.device("cuda:0")
t4 = np.zeros(4)
t4p = t4.ctypes.data_as(C.POINTER(C.c_double))
eps = np.finfo(np.float64).eps


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = fn()
    torch.cuda.synchronize()
    _lib.check(rc, "solve")
    return time.perf_counter() - t0


for n in sizes:
    nx, ny = C.c_int(), C.c_int()
    lib.eigx_get_matdims(n, C.byref(nx), C.byref(ny), 48, 128, b"O")
    ld = nx.value
    A = layout.random_symmetric_torch(n, dev)
    a = torch.zeros(n, ld, dtype=torch.float64, device=dev)
    anorm = torch.linalg.norm(A).item()
    for route in ("sx", "s"):
        full = lib.eigx_sx_dev if route == "sx" else lib.eigx_s_dev
        rng = lib.eigx_sx_range_dev if route == "sx" else lib.eigx_s_range_dev
        rngv = lib.eigx_sx_range_v_dev if route == "sx" else lib.eigx_s_range_v_dev
        if by_value:   # all eigenvalues once: the bounds of every window come from them
            wall = torch.zeros(n, dtype=torch.float64, device=dev)
            a[:, :n] = A.T
            timed(lambda: full(n, n, a.data_ptr(), ld, wall.data_ptr(), None, ld, 128, 128, b"N"))
            wh = wall.cpu().numpy()
        for m in ms:
            if m > n:
                continue
            z = torch.zeros(m, ld, dtype=torch.float64, device=dev)
            w = torch.zeros(n, dtype=torch.float64, device=dev)
            tf, tr, tv, stages = [], [], [], []
            if by_value:   # [vl, vu) around eigenvalues 1 .. m: a finite point below the spectrum, a mid-gap point above w(m)
                vl = float(wh[0] - (wh[-1] - wh[0]))
                vu = float(0.5 * (wh[m - 1] + wh[m])) if m < n else float(wh[-1] + (wh[-1] - wh[0]))
                wv = torch.zeros(m, dtype=torch.float64, device=dev)
                mv, ilv = C.c_int(), C.c_int()
            for rep in range(repeats + 1):   # rep 0 warms the workspace pool and the kernels of both
                if not no_full:
                    a[:, :n] = A.T
                    dt = timed(lambda: full(n, m, a.data_ptr(), ld, w.data_ptr(), z.data_ptr(), ld, 128, 128, b"A"))
                    if rep:
                        tf.append(dt)
                if by_value:
                    a[:, :n] = A.T
                    dt = timed(lambda: rngv(n, vl, vu, m, C.byref(mv), C.byref(ilv), a.data_ptr(), ld, wv.data_ptr(), z.data_ptr(),
                                            ld, 128, 128, b"A"))
                    assert (mv.value, ilv.value) == (m, 1), (mv.value, ilv.value)
                    if rep:
                        tv.append(dt)
                a[:, :n] = A.T
                dt = timed(lambda: rng(n, 1, m, a.data_ptr(), ld, w.data_ptr(), z.data_ptr(), ld, 128, 128, b"A"))
                if rep:
                    tr.append(dt)
                    lib.eigx_range_timers(t4p)
                    stages.append(t4.copy())
            path, mm, cond = C.c_int(), C.c_int(), C.c_double()
            lib.eigx_range_info(C.byref(path), C.byref(mm), C.byref(cond))
            Z = z[:, :n].T
            res = torch.linalg.norm(A @ Z - Z * w[None, :m]).item() / (n * eps * anorm)
            orth = torch.linalg.norm(Z.T @ Z - torch.eye(m, dtype=torch.float64, device=dev)).item() / (n * eps)
            st = np.median(np.array(stages), axis=0) * 1e3
            f, r = np.array(tf if tf else [float("nan")]) * 1e3, np.array(tr) * 1e3
            if by_value:
                assert (wv == w[:m]).all()   # the same window, the same code after the counts
                v = np.array(tv) * 1e3
                print(f"eigen_{route} n={n} m={m}: index call {np.median(r):.2f} ms [{r.min():.2f} .. {r.max():.2f}]  value call "
                      f"{np.median(v):.2f} ms [{v.min():.2f} .. {v.max():.2f}]  value - index {np.median(v) - np.median(r):+.2f} ms",
                      flush=True)
            print(f"eigen_{route} n={n} m={m}: nvec=m route {np.median(f):.1f} ms [{f.min():.1f} .. {f.max():.1f}]  range call "
                  f"{np.median(r):.1f} ms [{r.min():.1f} .. {r.max():.1f}]  ratio {np.median(r) / np.median(f):.2f}  | path {path.value} "
                  f"cond(L) {cond.value:.3g}  bisection {st[0]:.1f}  inverse iteration {st[1]:.1f}  orth + Rayleigh-Ritz {st[2]:.1f}  "
                  f"back-transformation {st[3]:.1f}  | held {lib.eigx_held_bytes() / 2**20:.0f} MiB  | gates: residual {res:.2e} "
                  f"orthogonality {orth:.2e}", flush=True)
            del z, w, Z
    if count_stage:
        d = torch.zeros(n, dtype=torch.float64, device=dev)
        e = torch.zeros(2 * n, dtype=torch.float64, device=dev)
        for band in (1, 2):
            a[:, :n] = A.T
            _lib.check(lib.eigx_band_reduce_dev(n, a.data_ptr(), ld, d.data_ptr(), e.data_ptr(), n, 128, band), "band_reduce")
            lo, hi = (d - 2 * e.abs().max()).min().item(), (d + 2 * e.abs().max()).max().item()
            for npts in (2, 4096):
                x = torch.linspace(lo, hi, npts + 2, dtype=torch.float64, device=dev)[1:-1].contiguous()
                cnt = torch.zeros(npts, dtype=torch.int32, device=dev)
                ts = [timed(lambda: lib.eigx_band_count_dev(n, d.data_ptr(), e.data_ptr(), n, band, npts, x.data_ptr(),
                                                            cnt.data_ptr())) for _ in range(21)][1:]
                t = np.array(ts) * 1e3
                print(f"eigx_band_count_dev n={n} band={band} npts={npts}: {np.median(t):.3f} ms [{t.min():.3f} .. {t.max():.3f}]  "
                      f"counts {cnt.min().item()} .. {cnt.max().item()}", flush=True)
    del A, a
    torch.cuda.empty_cache()
lib.eigx_free()
