"""Bit-for-bit record of what the whole-solve drivers return, for comparing two builds of the library.
usage: [EIGX_LIB=other/libeigenexa_amd.so] gpu_frame_dump.py OUTDIR [--quick | --batch | --range]

Runs a fixed list of seeded calls of eigen_sx / eigen_s, the index-range solves and eigen_h (device and host entry
points; every mode, panel widths, nvec < n, odd leading dimensions, scaled and non-finite inputs) and writes for each
call  NNN_label.{rc,w,z,flops}.npy : the returned status, w, z (the columns the call owns) and a(1,1) (the flop count;
the seconds in a(2,1) differ from run to run and are left out).  Then the complex generalised solvers eigx_hgev_dev and
eigx_hgev_range_dev and their stages (Cholesky, triangular solves, reduction; eigx_tune key 20 = 64 and the default):
the status, w, z and the arrays a / b as the call leaves them.  Then the real generalised solvers eigx_gev[_range][_dev],
the value-window solves (m and il as well), the host forms of all four generalised solvers and their statuses (non-finite
A or B, B not positive definite, a bad window, ldb < n) from sentinel-filled w and z.  An array above 8 MiB is stored as
its SHA-256.  Last the twelve batched families -- the uniform eigx_{s,h,gev,hgev}_batch, the ragged eigx_{s,h,gev,hgev}_vbatch
and the windowed eigx_{s,h,gev,hgev}_batch_range, host and device forms (batch_section below); --batch runs that section alone
(about a minute).  --range runs range_section below alone instead (under a minute): every range entry of the five families, which the
list above covers only in part; its .held files (bytes in the workspace pool) depend on the build, the others do not.
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


def batch_section():
    """eigx_{s,h,gev,hgev}_batch[_dev], modes A and N and mode A with info = NULL, at n = 1, 2, 17, 33, 64 (s, h, gev: 96, s: 128
    too) and, with the cutoff key lowered to 32, at n = 40 through the full-size solvers (gev: odd and even leading dimensions).
    A batch is the families of the family's test file, the first of them scaled by 1e-200 and by 1e+200, one matrix with a NaN
    and (gev, hgev) one pencil with an indefinite B.  Padded leading dimensions and strides, NaN outside the upper triangles,
    w / z / info prefilled; recorded: the status, the whole buffers w, z, info and (gev, hgev) b as the call leaves them, errinfo
    and the timers with entry 0 (the seconds of the call) set to zero.  Then the four ragged entries (ragged below) and the four
    windowed entries eigx_{s,h,gev,hgev}_batch_range[_dev] (window below) at one n below each class edge of the family's window
    kernel (s: 17, 64, 80, 100; h, gev: 17, 64, 80; hgev: 17, 64) with the windows (1, 1), (2, 5), (n - 3, n), each with key 26 = 1,
    key 26 = 2 and keys 26 = 1, 27 = 101, and at n = 40 with the family's cutoff key (21 to 24) lowered to 32; of these also b
    (gev, hgev) and eigx_batch_range_info."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import test_batch
    import test_gbatch
    import test_gvbatch
    import test_hbatch
    import test_hgbatch
    import test_vbatch

    def image(mats, ld, stride, cplx):
        """upper triangles (complex: interleaved, Im of the diagonal NaN); NaN in the lower triangles, the padding and the gaps"""
        n, c = mats[0].shape[0], 2 if cplx else 1
        buf = np.full(c * stride * len(mats), np.nan)
        upper = np.tri(n, dtype=bool)   # [j, i]: i <= j
        for k, M in enumerate(mats):
            v = buf[c * k * stride:c * (k * stride + ld * n)].reshape(n, ld, c)   # v[j, i] = m(i, j)
            v[:, :n, 0] = np.where(upper, M.T.real, np.nan)
            if cplx:
                v[:, :n, 1] = np.where(upper & ~np.eye(n, dtype=bool), M.T.imag, np.nan)
        return buf

    def frame_record(window=False):
        """what the frame leaves beside the arrays: errinfo, the timers without the seconds of the call and, of the windowed
        entry, (route, m, redone)"""
        err, t = C.c_int64(0), (C.c_double * 16)()
        lib.eigx_get_errinfo(C.byref(err))
        lib.eigx_get_timers(t)
        rec = dict(errinfo=np.int64(err.value), timers=np.array([0.0] + t[1:]))
        if window:
            r, m, d = C.c_int(-1), C.c_int(-1), C.c_int(-1)
            lib.eigx_batch_range_info(C.byref(r), C.byref(m), C.byref(d))
            rec["brinfo"] = np.array([r.value, m.value, d.value], dtype=np.int64)
        return rec

    def one(fam, n, even, tag):
        cplx, gev = fam in ("h", "hgev"), fam in ("gev", "hgev")
        mats = (test_hbatch if cplx else test_batch)._families(n)
        bad = mats[0].copy()
        bad[0, n - 1] = bad[n - 1, 0] = np.nan
        mats = mats + [mats[0] * 1e-200, mats[0] * 1e200, bad]
        nb = len(mats) + gev
        lda, ldb, ldz, ldw = (n + 4, n + 2, n + 2, n + 2) if even else (n + 3, n + 2, n + 1, n + 2)
        sa, sb, sz = lda * n + 5, ldb * n + 3, ldz * n + 7
        if gev:
            ov = (test_hgbatch if cplx else test_gbatch)._overlaps(n)
            indef = ov[0].copy()
            indef[n // 2, n // 2] = -1.0
            mats, bs = mats + [mats[1]], [ov[k % len(ov)] for k in range(nb - 1)] + [indef]
        a0 = image(mats, lda, sa, cplx)
        b0 = image(bs, ldb, sb, cplx) if gev else None
        c = 2 if cplx else 1
        for form in ("dev", "host"):
            fn = getattr(lib, f"eigx_{fam}_batch" + ("_dev" if form == "dev" else ""))
            for mode, with_info in (("A", True), ("N", True), ("A", False)):
                w, z = np.full(ldw * nb, SENT_B), np.full(c * sz * nb, SENT_B)
                info = np.full(nb, 77, dtype=np.int32)
                arrs = dict(a=a0.copy(), w=w, z=z, info=info, **(dict(b=b0.copy()) if gev else {}))
                if form == "dev":
                    arrs = {k: torch.from_numpy(v).to(dev) for k, v in arrs.items()}
                    ptr = {k: v.data_ptr() for k, v in arrs.items()}
                else:
                    ptr = {k: v.ctypes.data for k, v in arrs.items()}
                args = (n, nb, ptr["a"], lda, sa) + ((ptr["b"], ldb, sb) if gev else ()) + (
                    ptr["w"], ldw, ptr["z"] if mode == "A" else None, ldz, sz, mode.encode(), ptr["info"] if with_info else None)
                rc = fn(*args)
                if form == "dev":
                    torch.cuda.synchronize()
                    arrs = {k: v.cpu().numpy() for k, v in arrs.items()}
                del arrs["a"]
                save(f"{fam}batch_{form}_n{n}{tag}_{mode}{'' if with_info else '_noinfo'}", rc=np.int64(rc), **arrs, **frame_record())

    for fam, key, sizes in (("s", 21, (1, 2, 17, 33, 64, 96, 128)), ("h", 22, (1, 2, 17, 33, 64, 96)), ("gev", 23, (1, 2, 17, 33, 64, 96)),
                            ("hgev", 24, (1, 2, 17, 33, 64))):
        for n in sizes:
            one(fam, n, False, "")
        cutoff = lib.eigx_tune(key, 32)
        one(fam, 40, False, "_loop")
        if fam == "gev":
            one(fam, 40, True, "_loop_evenld")
        lib.eigx_tune(key, cutoff)

    def ragged(fam, pencil):
        """One call per form and mode of a ragged entry, in the buffers of the family's test file (gaps in front of every block,
        NaN outside the upper triangles, guards in w, z and info): orders 0, 1, 2, 17, 33, 64, `mid` and the largest the kernels
        serve, with the cutoff key lowered to `mid` -- an order of the top class, so every class is launched and the largest block
        alone goes through the full-size solver -- then a block with a NaN and (pencil families) one with an indefinite B."""
        mid = {128: 100, 96: 80, 64: 40}[fam.top]
        orders = [n for n in (0, 1, 2, 17, 33, 64) if n < mid] + [mid, fam.top]
        dt = np.float64 if fam.cs == 1 else np.complex128

        def pick(n, k):
            """member k of the family's matrices of order n: (A,) or (A, B)"""
            lists = fam.mixed(n) if pencil else (fam.families(n),)
            return tuple(x[k % len(x)] for x in lists)

        blocks = [pick(n, k) if n else (np.zeros((0, 0), dtype=dt),) * (1 + pencil) for k, n in enumerate(orders)]
        bad = pick(17, 0)[0].copy()
        bad[0, 16] = bad[16, 0] = np.nan
        blocks.append((bad,) + pick(17, 0)[1:])
        if pencil:
            indef = pick(33, 1)[1].copy()
            indef[16, 16] = -1.0
            blocks.append((pick(33, 1)[0], indef))
        lists = [list(x) for x in zip(*blocks)]
        cutoff = lib.eigx_tune(fam.key, mid)
        for form in ("dev", "host"):
            for mode, with_info in (("A", True), ("N", True), ("A", False)):
                R = (test_gvbatch.RaggedPencils if pencil else test_vbatch.Ragged)(fam, *lists, device=form == "dev")
                rc = R.run(lib, mode=mode.encode(), info=with_info, z=mode == "A", host=form == "host")
                if form == "dev":
                    torch.cuda.synchronize()
                img = R.images(host=form == "host")
                arrs = dict(zip(("w", "z", "b", "info") if pencil else ("w", "z", "info"), img))
                save(f"{fam.name}vbatch_{form}_{mode}{'' if with_info else '_noinfo'}", rc=np.int64(rc), **arrs, **frame_record())
        lib.eigx_tune(fam.key, cutoff)

    for fam, pencil in ((test_vbatch.S, False), (test_vbatch.H, False), (test_gvbatch.G, True), (test_gvbatch.HG, True)):
        ragged(fam, pencil)

    def window(fam, n, il, iu, tag):
        """eigx_{fam}_batch_range[_dev], modes A and N, on the batch of one(fam, ...) (a NaN matrix; gev, hgev: an indefinite B
        too): z with m columns per matrix"""
        cplx, gev = fam in ("h", "hgev"), fam in ("gev", "hgev")
        m, c = iu - il + 1, 2 if cplx else 1
        mats = (test_hbatch if cplx else test_batch)._families(n)
        bad = mats[0].copy()
        bad[0, n - 1] = bad[n - 1, 0] = np.nan
        mats = mats + [mats[0] * 1e-200, mats[0] * 1e200, bad]
        nb = len(mats) + gev
        lda, ldb, ldz, ldw = n + 3, n + 2, n + 1, m + 2
        sa, sb, sz = lda * n + 5, ldb * n + 3, ldz * m + 7
        if gev:
            ov = (test_hgbatch if cplx else test_gbatch)._overlaps(n)
            indef = ov[0].copy()
            indef[n // 2, n // 2] = -1.0
            mats, bs = mats + [mats[1]], [ov[k % len(ov)] for k in range(nb - 1)] + [indef]
        a0 = image(mats, lda, sa, cplx)
        b0 = image(bs, ldb, sb, cplx) if gev else None
        for form in ("dev", "host"):
            fn = getattr(lib, f"eigx_{fam}_batch_range" + ("_dev" if form == "dev" else ""))
            for mode in "AN":
                arrs = dict(a=a0.copy(), w=np.full(ldw * nb, SENT_B), z=np.full(c * sz * nb, SENT_B), info=np.full(nb, 77, dtype=np.int32),
                            **(dict(b=b0.copy()) if gev else {}))
                if form == "dev":
                    arrs = {k: torch.from_numpy(v).to(dev) for k, v in arrs.items()}
                    ptr = {k: v.data_ptr() for k, v in arrs.items()}
                else:
                    ptr = {k: v.ctypes.data for k, v in arrs.items()}
                rc = fn(n, nb, il, iu, ptr["a"], lda, sa, *((ptr["b"], ldb, sb) if gev else ()), ptr["w"], ldw,
                        ptr["z"] if mode == "A" else None, ldz, sz, mode.encode(), ptr["info"])
                if form == "dev":
                    torch.cuda.synchronize()
                    arrs = {k: v.cpu().numpy() for k, v in arrs.items()}
                del arrs["a"]
                save(f"{fam}brange_{form}_n{n}_{il}_{iu}{tag}_{mode}", rc=np.int64(rc), **arrs, **frame_record(window=True))

    # per family: an order below each class edge of its window kernel, then n = 40 above the cutoff key lowered to 32
    for fam, key, sizes in (("s", 21, (17, 64, 80, 100)), ("h", 22, (17, 64, 80)), ("gev", 23, (17, 64, 80)), ("hgev", 24, (17, 64))):
        for n in sizes:
            for il, iu in ((1, 1), (2, 5), (n - 3, n)):
                for route in (1, 2):
                    old = lib.eigx_tune(26, route)
                    window(fam, n, il, iu, f"_route{route}")
                    lib.eigx_tune(26, old)
                old, accept = lib.eigx_tune(26, 1), lib.eigx_tune(27, 101)   # the window kernel refuses every matrix: all are redone
                window(fam, n, il, iu, "_refused")
                lib.eigx_tune(26, old)
                lib.eigx_tune(27, accept)
        cutoff = lib.eigx_tune(key, 32)
        for il, iu in ((1, 1), (2, 5), (37, 40)):
            window(fam, 40, il, iu, "_loop")
        lib.eigx_tune(key, cutoff)


def range_section():
    """The range solves of the five families (sx, s, h, gev, hgev), by index and by value, device and host forms, at n = 5, 65,
    130 with a window that begins at the first eigenvalue and one that does not: mode A with key 17 = 100 and 0 (paths 1 and 3)
    and with key 19 = 0 (the acceptance test refuses: path 2); modes N and, by value, C; by value also an empty window, one that
    overflows mmax and infinite bounds; a NaN in A; A scaled by 1e+200 and 1e-200; and key 18 = 1 through eigx_sx_dev.
    Recorded: the status, w, z, *m, *il, a (its seconds a(2,1) zeroed) and b as the call leaves them, eigx_range_info, errinfo, the
    timers without their seconds (entries 0 .. 4), and, in a file of its own kind (.held), eigx_held_bytes()."""

    def problem(fam, n):
        cplx, pencil = fam in ("h", "hgev"), fam in ("gev", "hgev")
        g = np.random.default_rng(5000 + n)
        S = g.standard_normal((n, n)) + (1j * g.standard_normal((n, n)) if cplx else 0.0)
        X = g.standard_normal((n, n)) + (1j * g.standard_normal((n, n)) if cplx else 0.0)
        A = (S + S.conj().T) / 2
        if not pencil:
            return A, None, np.linalg.eigvalsh(A)
        B = X @ X.conj().T / n + np.eye(n)
        B = (B + B.conj().T) / 2
        L = np.linalg.cholesky(B)
        Cm = np.linalg.solve(L, np.linalg.solve(L, A).conj().T).conj().T
        return A, B, np.linalg.eigvalsh((Cm + Cm.conj().T) / 2)

    def image(M, ld, form):
        if form == "host":
            return np.asfortranarray(M.copy())
        t = torch.zeros(M.shape[1], ld, dtype=torch.complex128 if np.iscomplexobj(M) else torch.float64, device=dev)
        t[:, :M.shape[0]] = torch.from_numpy(np.ascontiguousarray(M.T)).to(dev)
        return t

    def one(label, fam, form, A, B, win, mode):
        """win = (il, iu) or (vl, vu, mmax); w has two entries and z one column more than the call may write"""
        n = A.shape[0]
        by_value = len(win) == 3
        cap = max(win[2] if by_value else win[1] - win[0] + 1, 0)
        ld = n if form == "host" else n + (n & 1)
        a, b = image(A, ld, form), None if B is None else image(B, ld, form)
        if form == "host":
            w, z = np.full(cap + 2, SENT_B), np.full((n, cap + 1), SENT_B, dtype=A.dtype, order="F")
            ptr = lambda x: x.ctypes.data
        else:
            w = torch.full((cap + 2,), SENT_B, dtype=torch.float64, device=dev)
            z = torch.full((cap + 1, ld), SENT_B, dtype=a.dtype, device=dev)
            ptr = lambda x: x.data_ptr()
        m, il = C.c_int(-77), C.c_int(-77)
        fn = getattr(lib, f"eigx_{fam}_range" + ("_v" if by_value else "") + ("_dev" if form == "dev" else ""))
        head = (n, float(win[0]), float(win[1]), win[2], C.byref(m), C.byref(il)) if by_value else (n, win[0], win[1])
        mats = (ptr(a), ld) + (() if B is None else (ptr(b), ld))
        rc = fn(*head, *mats, ptr(w), ptr(z), ld, *((0, 0) if B is None else ()), mode.encode())
        if form == "dev":
            torch.cuda.synchronize()
            w, z, a = w.cpu().numpy(), z.cpu().numpy(), a.cpu().numpy().T.copy()
            b = None if b is None else b.cpu().numpy()
        if B is None and rc == 0 and n > 1:
            a[1, 0] = 0.0   # the seconds of the call
        finish(f"{fam}_{form}_n{n}_{label}", rc, w=w, z=z, a=a, m=np.int64(m.value), il=np.int64(il.value),
               **({} if b is None else dict(b=b)))

    def finish(label, rc, **arrays):
        path, mm, cond = C.c_int(0), C.c_int(0), C.c_double(0.0)
        lib.eigx_range_info(C.byref(path), C.byref(mm), C.byref(cond))
        err, t = C.c_int64(0), (C.c_double * 16)()
        lib.eigx_get_errinfo(C.byref(err))
        lib.eigx_get_timers(t)
        save(f"{label}_path{path.value}", rc=np.int64(rc), rinfo=np.array([path.value, mm.value, cond.value]), errinfo=np.int64(err.value),
             timers=np.array([0.0] * 5 + t[5:]), held=np.int64(lib.eigx_held_bytes()), **arrays)

    def mid(lam, k):
        """between the eigenvalues k and k + 1 (1-based); k = 0: below all"""
        return lam[0] - 1.0 if k == 0 else 0.5 * (lam[k - 1] + lam[k])

    for n in (5, 65, 130):
        wins = ((1, 3), (2, 4)) if n == 5 else ((1, 10), (n // 3, n // 3 + 9))
        for fam in ("sx", "s", "h", "gev", "hgev"):
            A, B, lam = problem(fam, n)
            bad = A.copy()
            bad[1, 3] = bad[3, 1] = np.nan
            for form in ("dev", "host"):
                for il, iu in wins:
                    m = iu - il + 1
                    vl, vu = mid(lam, il - 1), mid(lam, iu)
                    for tag, k17, k19 in (("p1", 100, None), ("p3", 0, None), ("p2", 100, 0)):
                        old17 = lib.eigx_tune(17, k17)
                        old19 = lib.eigx_tune(19, k19) if k19 is not None else None
                        one(f"{il}_{iu}_{tag}_A", fam, form, A, B, (il, iu), "A")
                        one(f"v{il}_{iu}_{tag}_A", fam, form, A, B, (vl, vu, m + 1), "A")
                        lib.eigx_tune(17, old17)
                        if old19 is not None:
                            lib.eigx_tune(19, old19)
                    one(f"{il}_{iu}_N", fam, form, A, B, (il, iu), "N")
                    one(f"v{il}_{iu}_N", fam, form, A, B, (vl, vu, m + 1), "N")
                    one(f"v{il}_{iu}_C", fam, form, A, B, (vl, vu, 0), "C")
                    one(f"v{il}_{iu}_small", fam, form, A, B, (vl, vu, m - 1), "A")
                    one(f"{il}_{iu}_nan", fam, form, bad, B, (il, iu), "A")
                    one(f"v{il}_{iu}_nan", fam, form, bad, B, (vl, vu, m + 1), "A")
                    for tag, s in (("big", 1e200), ("tiny", 1e-200)):
                        one(f"{il}_{iu}_{tag}", fam, form, A * s, B, (il, iu), "A")
                        one(f"v{il}_{iu}_{tag}", fam, form, A * s, B, (vl * s, vu * s, m + 1), "A")
                il = wins[1][0]
                gap = lam[il - 1] - lam[il - 2]
                one("v_empty", fam, form, A, B, (lam[il - 2] + 0.25 * gap, lam[il - 2] + 0.75 * gap, 4), "A")
                one("v_all", fam, form, A, B, (-np.inf, np.inf, n), "A")
                one("v_upper", fam, form, A, B, (mid(lam, n - 3), np.inf, 4), "A")
        # the opt-in route of eigx_sx_dev: the lowest nvec pairs by the range path, w filled up by bisection
        A = problem("sx", n)[0]
        nvec = 3 if n == 5 else 10
        old18 = lib.eigx_tune(18, 1)
        a = image(A, n + (n & 1), "dev")
        z = torch.full((nvec + 1, n + (n & 1)), SENT_B, dtype=torch.float64, device=dev)
        w = torch.full((n + 2,), SENT_B, dtype=torch.float64, device=dev)
        rc = lib.eigx_sx_dev(n, nvec, a.data_ptr(), n + (n & 1), w.data_ptr(), z.data_ptr(), n + (n & 1), 128, 128, b"A")
        torch.cuda.synchronize()
        lib.eigx_tune(18, old18)
        a = a.cpu().numpy().T.copy()
        a[1, 0] = 0.0
        finish(f"sx_dev_n{n}_key18", rc, w=w.cpu().numpy(), z=z.cpu().numpy(), a=a)


SENT_B = -7.25   # what w and z of the batch and range sections start from
_sym = {}


if "--range" in sys.argv[2:]:
    range_section()
    lib.eigx_free()
    print(f"DUMPED {count[0]} calls into {out}", flush=True)
    sys.exit(0)
if "--batch" in sys.argv[2:]:
    batch_section()
    lib.eigx_free()
    print(f"DUMPED {count[0]} calls into {out}", flush=True)
    sys.exit(0)


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

# ---- the real generalised solvers (gev.hip), the value-window solves, and the host forms of all four ---------------------
SENT = 12345.678   # w and z start from it where "not written" is to show in the dump


def rpencil(n):
    X = np.random.default_rng(4000 + n).standard_normal((n, n))
    B = X @ X.T / n + np.eye(n)
    return sym(n), (B + B.T) / 2


def rdev(M, ld, ncols=None, fill=0.0):
    """t[j, i] = M(i, j) with leading dimension ld, the padding `fill` (M None: all `fill`)"""
    t = torch.full((ncols if M is None else M.shape[1], ld), fill, dtype=torch.float64, device=dev)
    if M is not None:
        t[:, :M.shape[0]] = torch.from_numpy(np.ascontiguousarray(M.T)).to(dev)
    return t


def gen_eigs(A, B):
    L = np.linalg.cholesky(B)
    Y = np.linalg.solve(L, A)
    return np.linalg.eigvalsh(np.linalg.solve(L, Y.T).T)


def mid(lam, k):
    """between the eigenvalues k and k + 1 (1-based); k = 0 / n: below / above all"""
    if k == 0:
        return lam[0] - 1.0
    return lam[-1] + 1.0 if k == len(lam) else 0.5 * (lam[k - 1] + lam[k])


def gen_dev(label, fn, A, B, win=None, mode="A", ld=None, ldb=None, cplx=False, fill=0.0):
    """One device call of a generalised solver: win None (eigx_gev_dev / eigx_hgev_dev), (il, iu), or (vl, vu, mmax)"""
    n = A.shape[0]
    ld = ld or n + (n & 1)
    mk = cdev if cplx else rdev
    a, b = mk(A, ld), mk(B, ld)
    cap = n if win is None else (win[2] if len(win) == 3 else max(win[1] - win[0] + 1, 1))
    z = torch.full((max(cap, 1), ld), fill, dtype=torch.complex128 if cplx else torch.float64, device=dev)
    w = torch.full((max(cap, 1),), fill, dtype=torch.float64, device=dev)
    extra = {}
    pa, pb, pw, pz = a.data_ptr(), b.data_ptr(), w.data_ptr(), z.data_ptr()
    if win is None:
        rc = fn(n, pa, ld, pb, ldb or ld, pw, pz, ld)
    elif len(win) == 2:
        rc = fn(n, win[0], win[1], pa, ld, pb, ldb or ld, pw, pz, ld, mode.encode())
    else:
        m, il = C.c_int(-1), C.c_int(-1)
        rc = fn(n, win[0], win[1], win[2], C.byref(m), C.byref(il), pa, ld, pb, ldb or ld, pw, pz, ld, mode.encode())
        extra = dict(m=np.int64(m.value), il=np.int64(il.value))
    torch.cuda.synchronize()
    if win is None and rc == -7:
        b[0, 1] = 0.0   # B not positive definite: b is what eigen_s / eigen_h of B left, its b(2,1) the seconds of that solve
    save(label, rc=np.int64(rc), w=w.cpu().numpy(), z=z.cpu().numpy(), a=a.cpu().numpy(), b=b.cpu().numpy(), **extra)


def gen_host(label, fn, A, B, win=None, mode="A", ldb=None, fill=0.0):
    """The same through a host entry point (Fortran-ordered arrays; complex by A's dtype)"""
    n = A.shape[0]
    a, b = np.asfortranarray(A.copy()), np.asfortranarray(B.copy())
    cap = n if win is None else (win[2] if len(win) == 3 else max(win[1] - win[0] + 1, 1))
    z = np.full((n, max(cap, 1)), fill, dtype=A.dtype, order="F")
    w = np.full(max(cap, 1), fill)
    extra = {}
    pa, pb, pw, pz = a.ctypes.data, b.ctypes.data, w.ctypes.data, z.ctypes.data
    if win is None:
        rc = fn(n, pa, n, pb, ldb or n, pw, pz, n)
    elif len(win) == 2:
        rc = fn(n, win[0], win[1], pa, n, pb, ldb or n, pw, pz, n, mode.encode())
    else:
        m, il = C.c_int(-1), C.c_int(-1)
        rc = fn(n, win[0], win[1], win[2], C.byref(m), C.byref(il), pa, n, pb, ldb or n, pw, pz, n, mode.encode())
        extra = dict(m=np.int64(m.value), il=np.int64(il.value))
    save(label, rc=np.int64(rc), w=w, z=z, a=a, b=b, **extra)


for n in (5, 130, 517):
    gen_dev(f"gev_n{n}", lib.eigx_gev_dev, *rpencil(n))
gen_host("gev_host_n130", lib.eigx_gev, *rpencil(130))
n = 517
A, B = rpencil(n)
for pct in (100, 0):
    lib.eigx_tune(17, pct)
    for il, iu in ((1, n), (n // 3, n // 3 + 39)):
        for mode in "AN":
            gen_dev(f"gevr_pct{pct}_{il}_{iu}_{mode}", lib.eigx_gev_range_dev, A, B, (il, iu), mode)
lib.eigx_tune(17, -1)
gen_host("gevr_host", lib.eigx_gev_range, A, B, (n // 3, n // 3 + 39))

# by value: vl, vu midway between neighbouring eigenvalues, so that no count depends on rounding
k0 = n // 3
for name, fn, lam in (("sxrv", lib.eigx_sx_range_v_dev, np.linalg.eigvalsh(A)), ("srv", lib.eigx_s_range_v_dev, np.linalg.eigvalsh(A)),
                      ("gevrv", lib.eigx_gev_range_v_dev, gen_eigs(A, B))):
    gap = lam[k0] - lam[k0 - 1]
    cases = (("w40", mid(lam, k0), mid(lam, k0 + 40), 64, "A"), ("empty", lam[k0 - 1] + 0.25 * gap, lam[k0 - 1] + 0.75 * gap, 64, "A"),
             ("small", mid(lam, k0), mid(lam, k0 + 40), 10, "A"), ("count", mid(lam, k0), mid(lam, k0 + 40), 0, "C"),
             ("all", -np.inf, np.inf, n, "A"), ("w40N", mid(lam, k0), mid(lam, k0 + 40), 64, "N"))
    for cname, vl, vu, mmax, mode in cases:
        if name == "gevrv":
            gen_dev(f"{name}_{cname}", fn, A, B, (vl, vu, mmax), mode, fill=SENT)
        else:
            a = rdev(A, n + 1)
            z = torch.full((max(mmax, 1), n + 1), SENT, dtype=torch.float64, device=dev)
            w = torch.full((max(mmax, 1),), SENT, dtype=torch.float64, device=dev)
            m, il = C.c_int(-1), C.c_int(-1)
            rc = fn(n, vl, vu, mmax, C.byref(m), C.byref(il), a.data_ptr(), n + 1, w.data_ptr(), z.data_ptr(), n + 1, 128, 128,
                    mode.encode())
            torch.cuda.synchronize()
            save(f"{name}_{cname}", rc=np.int64(rc), w=w.cpu().numpy(), z=z.cpu().numpy(), flops=a[0, 0].item(),
                 m=np.int64(m.value), il=np.int64(il.value))
lam = np.linalg.eigvalsh(A)
a = np.asfortranarray(A.copy())
z = np.full((n, 64), SENT, order="F")
w = np.full(64, SENT)
m, il = C.c_int(-1), C.c_int(-1)
rc = lib.eigx_sx_range_v(n, mid(lam, k0), mid(lam, k0 + 40), 64, C.byref(m), C.byref(il), a.ctypes.data, n, w.ctypes.data,
                         z.ctypes.data, n, 128, 128, b"A")
save("sxrv_host", rc=np.int64(rc), w=w, z=z, flops=a[0, 0], m=np.int64(m.value), il=np.int64(il.value))
lam = gen_eigs(A, B)
gen_host("gevrv_host", lib.eigx_gev_range_v, A, B, (mid(lam, k0), mid(lam, k0 + 40), 64), fill=SENT)

n = 130
gen_host("hgev_host_n130", lib.eigx_hgev, *pencil(n))
gen_host("hgevr_host_n130", lib.eigx_hgev_range, *pencil(n), (n // 3, n // 3 + 39))

# statuses of the four generalised solvers, device and host form: w and z start from the sentinel
n = 65
for fam, cplx, pen in (("gev", False, rpencil(n)), ("hgev", True, pencil(n))):
    A, B = pen
    nanA, nanB, indef = A.copy(), B.copy(), B.copy()
    nanA[3, 9] = nanA[9, 3] = np.nan
    nanB[3, 9] = nanB[9, 3] = np.nan
    indef[7, 7] = -1.0
    full, rng = getattr(lib, f"eigx_{fam}"), getattr(lib, f"eigx_{fam}_range")
    full_d, rng_d = getattr(lib, f"eigx_{fam}_dev"), getattr(lib, f"eigx_{fam}_range_dev")
    for cname, Ax, Bx, win, ldb in (("nanA", nanA, B, (5, 20), None), ("nanB", A, nanB, (5, 20), None),
                                    ("notspd", A, indef, (5, 20), None), ("badwin", A, B, (20, 5), None),
                                    ("ldb", A, B, (5, 20), n - 1)):
        if cname != "badwin":
            gen_dev(f"st_{fam}_dev_{cname}", full_d, Ax, Bx, None, cplx=cplx, ldb=ldb, fill=SENT)
            gen_host(f"st_{fam}_host_{cname}", full, Ax, Bx, None, ldb=ldb, fill=SENT)
        gen_dev(f"st_{fam}r_dev_{cname}", rng_d, Ax, Bx, win, cplx=cplx, ldb=ldb, fill=SENT)
        gen_host(f"st_{fam}r_host_{cname}", rng, Ax, Bx, win, ldb=ldb, fill=SENT)
batch_section()
lib.eigx_free()
print(f"DUMPED {count[0]} calls into {out}", flush=True)
