"""Where the spectral route of eigx_gev_dev gains or loses accuracy on an ill-conditioned B: the driver as
it is, then its stages replaced one at a time.  With the GPU's own F = Z_B W_B^-1/2 (left in b) and C = F^T A F formed in
longdouble, the inner solve is done by LAPACK (syevd), by eigen_s and by eigen_sx on the GPU, once with F's columns in ascending
order of w_B ("asc": C graded with its large entries at the top left) and once reversed ("desc": what gev_dev feeds its inner
solve).  Every result is judged as a pencil (hard_dense.pencil_metrics: E_w, E_r, E_o in eps cond(B)) and C as a standard
problem against a longdouble reference of that C (hard_dense.metrics, in eps |C|_2).  One GPU.

usage: gpu_gev_order_probe.py                  the four pencils of profiles/dense_pencil_accuracy.log
       EIGX_LIB=<another build's libeigenexa_amd.so> gpu_gev_order_probe.py     the same against that library's driver"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hard_dense as hd  # noqa: E402
import eigenexa_amd as ee  # noqa: E402
from eigenexa_amd import _lib, api  # noqa: E402

CASES = ((130, "glued_rot", 4), (130, "random", 4), (65, "glued_rot", 4), (130, "glued_rot", 0))
LD = hd.LD
ee.eigen_init()
lib = _lib.load()
dev = torch.device("cuda:0")


def to_dev(M, ld):
    """column-major image of M with leading dimension ld: tensor (cols, ld), t[j, i] = M(i, j)"""
    t = torch.zeros(M.shape[1], ld, dtype=torch.float64, device=dev)
    t[:, :M.shape[0]] = torch.from_numpy(np.ascontiguousarray(M.T)).to(dev)
    return t


def from_dev(t, rows):
    return np.ascontiguousarray(t[:, :rows].T.cpu().numpy())


def driver(pc):
    """eigx_gev_dev on the upper triangles: w, Z and the F left in b"""
    n = pc.n
    ld = n + 2 + (n & 1)
    a, b = to_dev(hd.nan_lower(pc.A), ld), to_dev(hd.nan_lower(pc.B), ld)
    z = torch.zeros(n, ld, dtype=torch.float64, device=dev)
    w = torch.zeros(n, dtype=torch.float64, device=dev)
    rc = lib.eigx_gev_dev(n, a.data_ptr(), ld, b.data_ptr(), ld, w.data_ptr(), z.data_ptr(), ld)
    assert rc == 0, rc
    return w.cpu().numpy(), from_dev(z, n), from_dev(b, n)


def gpu_eig(which, Cm):
    """eigen_s / eigen_sx, mode 'X', on the upper triangle of Cm"""
    n = Cm.shape[0]
    ld = n + 2 + (n & 1)
    a = to_dev(hd.nan_lower(Cm), ld)
    z = torch.zeros(n, ld, dtype=torch.float64, device=dev)
    w = torch.zeros(n, dtype=torch.float64, device=dev)
    (ee.eigen_s if which == "s" else ee.eigen_sx)(n, n, a, ld, w, z, ld, mode="X")
    assert api.last_status() == 0
    return w.cpu().numpy(), from_dev(z, n)


class Standard:
    """C with its longdouble reference eigenvalues, as hard_dense.metrics reads a case"""

    def __init__(self, Cm):
        self.A = Cm
        self.lam = hd.reference_eigenvalues(Cm)
        self.anorm = float(np.abs(self.lam).max())


def show(tag, pc, w, Z, cs=None, Y=None):
    m = hd.pencil_metrics(pc, w, Z, None)[:3]
    line = f"LOC {tag}: pencil E_w={m[0]:.3f} E_r={m[1]:.3f} E_o={m[2]:.3f}"
    if cs is not None:
        s = hd.metrics(cs, w, Y)
        line += f" | C as a standard problem (eps |C|_2): E_w={s[0]:.3f} E_r={s[1]:.3f} E_o={s[2]:.3f}"
    print(line, flush=True)


print(f"library: {_lib.LIB_PATH}")
for n, fam, c in CASES:
    pc = hd.pencil("gev", n, fam, c)
    w, Z, F = driver(pc)
    show(f"n={n} {fam} c={c} eigx_gev_dev", pc, w, Z)
    Fl = F.astype(LD)
    Cl = Fl.T @ pc.A.astype(LD) @ Fl
    for order in ("asc", "desc"):
        P = np.arange(n) if order == "asc" else np.arange(n)[::-1]
        Fo = F[:, P]
        Cp = Cl[np.ix_(P, P)]
        Cm = np.asarray((Cp + Cp.T) / 2, dtype=np.float64)
        cs = Standard(Cm)
        wl, Yl = np.linalg.eigh(Cm)
        show(f"  {order} LAPACK syevd on C", pc, wl, Fo @ Yl, cs, Yl)
        for which in ("s", "sx"):
            wg, Yg = gpu_eig(which, Cm)
            show(f"  {order} eigen_{which} on C", pc, wg, Fo @ Yg, cs, Yg)
ee.eigen_free()
