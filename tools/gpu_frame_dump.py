"""Bit-for-bit record of what the whole-solve drivers return, for comparing two builds of the library.
usage: [EIGX_LIB=other/libeigenexa_amd.so] gpu_frame_dump.py OUTDIR [--quick]

Runs a fixed list of seeded calls of eigen_sx / eigen_s, the index-range solves and eigen_h (device and host entry
points; every mode, panel widths, nvec < n, odd leading dimensions, scaled and non-finite inputs) and writes for each
call  NNN_label.{rc,w,z,flops}.npy : the returned status, w, z (the columns the call owns) and a(1,1) (the flop count;
the seconds in a(2,1) differ from run to run and are left out).  Then the complex generalised solvers eigx_hgev_dev and
eigx_hgev_range_dev and their stages (Cholesky, triangular solves, reduction; eigx_tune key 20 = 64 and the default):
the status, w, z and the arrays a / b as the call leaves them.  An array above 8 MiB is stored as its SHA-256.
The library is deterministic, so two builds that compute the same leave directories that `cmp` finds equal:
    for f in A/*; do cmp $f B/$(basename $f); done
Run each build in a fresh process.  --quick leaves out n >= 2048."""
import ctypes as C
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from eigenexa_amd import _lib

out = sys.argv[1]
quick = "--quick" in sys.argv[2:]
os.makedirs(out, exist_ok=True)
lib = _lib.load()
_lib.check(lib.eigx_init(0), "init")
dev = torch.device("cuda:0")
count = [0]


def save(label, **arrays):
    idx = count[0]
    count[0] += 1
    for key, v in arrays.items():
        v = np.ascontiguousarray(v)
        if v.nbytes > (8 << 20):
            v = np.frombuffer(hashlib.sha256(v.tobytes()).digest(), dtype=np.uint8)
        np.save(os.path.join(out, f"{idx:03d}_{label}.{key}.npy"), v)
    print(f"{idx:03d} {label} rc={int(arrays['rc'])} flops={float(arrays.get('flops', 0.0)):.6e}", flush=True)


_sym = {}


def sym(n):
    if n not in _sym:
        B = np.random.default_rng(1000 + n).standard_normal((n, n))
        _sym[n] = (B + B.T) / 2
    return _sym[n]


def herm(n):
    g = np.random.default_rng(2000 + n)
    B = g.standard_normal((n, n)) + 1j * g.standard_normal((n, n))
    return (B + B.conj().T) / 2


def real_dev(fn, label, A, nvec, mode, ld=None, mf=128, mb=128):
    """fn = eigx_sx_dev / eigx_s_dev; a[j, i] = A(i, j) with leading dimension ld"""
    n = A.shape[0]
    ld = ld or n
    a = torch.zeros(n, ld, dtype=torch.float64, device=dev)
    a[:, :n] = torch.from_numpy(np.ascontiguousarray(A.T)).to(dev)
    z = torch.zeros(n, ld, dtype=torch.float64, device=dev)
    w = torch.zeros(n, dtype=torch.float64, device=dev)
    rc = fn(n, nvec, a.data_ptr(), ld, w.data_ptr(), z.data_ptr(), ld, mf, mb, mode.encode())
    torch.cuda.synchronize()
    save(label, rc=np.int64(rc), w=w.cpu().numpy(), z=z[:max(nvec, 0), :n].cpu().numpy(), flops=a[0, 0].item())


def range_dev(fn, label, A, il, iu, mode):
    n = A.shape[0]
    m = iu - il + 1
    a = torch.from_numpy(np.ascontiguousarray(A.T)).to(dev)
    z = torch.zeros(m, n, dtype=torch.float64, device=dev)
    w = torch.zeros(m, dtype=torch.float64, device=dev)   # w holds m entries only
    rc = fn(n, il, iu, a.data_ptr(), n, w.data_ptr(), z.data_ptr(), n, 128, 128, mode.encode())
    torch.cuda.synchronize()
    path, mm, cond = C.c_int(0), C.c_int(0), C.c_double(0.0)
    lib.eigx_range_info(C.byref(path), C.byref(mm), C.byref(cond))
    save(f"{label}_path{path.value if rc == 0 else 0}", rc=np.int64(rc), w=w.cpu().numpy(), z=z.cpu().numpy(),
         flops=a[0, 0].item())


def herm_dev(label, A, nvec, mode, mf):
    n = A.shape[0]
    at = torch.from_numpy(np.ascontiguousarray(A.T)).to(dev)   # at[j, i] = A(i, j)
    z = torch.zeros(n, n, dtype=torch.complex128, device=dev)
    w = torch.zeros(n, dtype=torch.float64, device=dev)
    rc = lib.eigx_h_dev(n, nvec, at.data_ptr(), n, w.data_ptr(), z.data_ptr(), n, mf, 128, mode.encode())
    torch.cuda.synchronize()
    save(label, rc=np.int64(rc), w=w.cpu().numpy(), z=z[:nvec].cpu().numpy(), flops=at[0, 0].real.item())


routes = (("sx", lib.eigx_sx_dev), ("s", lib.eigx_s_dev))
# ---- eigen_sx / eigen_s on device arrays: every size, mode and nvec in {n, n / 3} ------------------------------------
for n in (1, 2, 3, 130, 1000) + (() if quick else (4096,)):
    for name, fn in routes:
        for mode in "ANXSCTR":
            for nvec in sorted({n, max(1, n // 3)}) if mode != "N" else (n,):
                real_dev(fn, f"{name}_n{n}_{mode}_v{nvec}", sym(n), nvec, mode)
for name, fn in routes:
    real_dev(fn, f"{name}_oddld", sym(130), 130, "A", ld=131)
    real_dev(fn, f"{name}_big", sym(130) * 1e120, 130, "A")
    real_dev(fn, f"{name}_tiny", sym(130) * 1e-120, 130, "A")
    bad = sym(130).copy()
    bad[5, 7] = bad[7, 5] = np.nan
    real_dev(fn, f"{name}_nan", bad, 130, "A")

# ---- the host entry points, once each -----------------------------------------------------------------------------------
n = 130
a = np.asfortranarray(sym(n).copy())
z = np.zeros((n, n), order="F")
w = np.zeros(n)
rc = lib.eigx_sx(n, n, a.ctypes.data, n, w.ctypes.data, z.ctypes.data, n, 128, 128, b"A")
save("host_sx", rc=np.int64(rc), w=w, z=z, flops=a[0, 0])
n = 100
a = np.asfortranarray(herm(n))
z = np.zeros((n, n), dtype=np.complex128, order="F")
w = np.zeros(n)
rc = lib.eigx_h(n, n, a.ctypes.data, n, w.ctypes.data, z.ctypes.data, n, 48, 128, b"A")
save("host_h", rc=np.int64(rc), w=w, z=z, flops=a[0, 0].real)

# ---- index-range solves: the subset path (1) and the full divide and conquer (3) by key 17, key 18, mode N, NaN ----------
n = 1000
for name, fn in (("sxr", lib.eigx_sx_range_dev), ("sr", lib.eigx_s_range_dev)):
    for pct in (100, 0):
        lib.eigx_tune(17, pct)
        range_dev(fn, f"{name}_pct{pct}_A", sym(n), 101, 140, "A")
    lib.eigx_tune(17, 100)
    range_dev(fn, f"{name}_N", sym(n), 101, 140, "N")
    bad = sym(n).copy()
    bad[5, 7] = bad[7, 5] = np.nan
    range_dev(fn, f"{name}_nan", bad, 101, 140, "A")
for name, fn in routes:
    for optin in (1, 0):
        lib.eigx_tune(18, optin)
        real_dev(fn, f"{name}_key18_{optin}", sym(n), 40, "A")
lib.eigx_tune(17, -1)

# ---- eigen_h on device arrays -------------------------------------------------------------------------------------------
for n in (1, 2, 3, 200, 1000) + (() if quick else (2048,)):
    A = herm(n)
    for mode in "ANXS":
        for mf in (32, 48):
            for nvec in sorted({n, max(1, n // 3)}) if mode != "N" else (n,):
                herm_dev(f"h_n{n}_{mode}_mf{mf}_v{nvec}", A, nvec, mode, mf)
herm_dev("h_big", herm(200) * 1e120, 200, "A", 48)
herm_dev("h_tiny", herm(200) * 1e-120, 200, "X", 48)

# ---- the complex generalised solvers and their stages (split planes: zplanes.hip) ----------------------------------------
def pencil(n):
    g = np.random.default_rng(3000 + n)
    X = g.standard_normal((n, n)) + 1j * g.standard_normal((n, n))
    B = X @ X.conj().T / n + np.eye(n)
    return herm(n), (B + B.conj().T) / 2


def cdev(M, ld):
    """t[j, i] = M(i, j) with leading dimension ld (complex elements), the padding zero"""
    t = torch.zeros(M.shape[1], ld, dtype=torch.complex128, device=dev)
    t[:, :M.shape[0]] = torch.from_numpy(np.ascontiguousarray(M.T)).to(dev)
    return t


def hgev_dev(label, n, il=None, iu=None, mode="A"):
    A, B = pencil(n)
    ld = n + 2
    a, b = cdev(A, ld), cdev(B, ld)
    m = n if il is None else iu - il + 1
    z = torch.zeros(m, ld, dtype=torch.complex128, device=dev)
    w = torch.zeros(m, dtype=torch.float64, device=dev)
    if il is None:
        rc = lib.eigx_hgev_dev(n, a.data_ptr(), ld, b.data_ptr(), ld, w.data_ptr(), z.data_ptr(), ld)
    else:
        rc = lib.eigx_hgev_range_dev(n, il, iu, a.data_ptr(), ld, b.data_ptr(), ld, w.data_ptr(), z.data_ptr(), ld,
                                     mode.encode())
    torch.cuda.synchronize()
    save(label, rc=np.int64(rc), w=w.cpu().numpy(), z=z.cpu().numpy(), a=a.cpu().numpy(), b=b.cpu().numpy())


for n in (5, 130, 517):
    hgev_dev(f"hgev_n{n}", n)
for n in (130, 517):
    for il, iu in ((1, n), (n // 3, n // 3 + 39)):
        for mode in "AN":
            hgev_dev(f"hgevr_n{n}_{il}_{iu}_{mode}", n, il, iu, mode)
nb_default = lib.eigx_tune(20, 64)
for nb in (64, nb_default):
    lib.eigx_tune(20, nb)
    for n in (65, 517):
        A, B = pencil(n)
        ld = n + 2
        b = cdev(B, ld)
        rc = lib.eigx_zchol_dev(n, b.data_ptr(), ld)
        torch.cuda.synchronize()
        save(f"zchol_n{n}_nb{nb}", rc=np.int64(rc), b=b.cpu().numpy())
        for trans in "NC":
            x = cdev(A[:, :n // 2 + 1], ld)
            rc = lib.eigx_ztrsm_upper_dev(trans.encode(), n, n // 2 + 1, b.data_ptr(), ld, x.data_ptr(), ld)
            torch.cuda.synchronize()
            save(f"ztrsm_n{n}_nb{nb}_{trans}", rc=np.int64(rc), z=x.cpu().numpy())
        a = cdev(A, ld)
        rc = lib.eigx_hgev_reduce_dev(n, a.data_ptr(), ld, b.data_ptr(), ld)
        torch.cuda.synchronize()
        save(f"hgev_reduce_n{n}_nb{nb}", rc=np.int64(rc), a=a.cpu().numpy())
lib.eigx_free()
print(f"DUMPED {count[0]} calls into {out}", flush=True)
