"""CPU tests of the host logic: C-ABI library loads and exports every declared symbol (no compute without a
GPU), index helpers, cyclic layout round trips, grid rule, and the N>1 plumbing under gloo (world_size 2)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    txt = open(os.path.join(ROOT, "include", "eigenexa_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(eigx_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    import ctypes

    from eigenexa_amd import _lib

    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared_symbols()
    assert len(names) >= 30
    for name in names:
        assert hasattr(lib, name), f"{name} declared in include/eigenexa_amd.h but not exported"
    # and the ctypes table covers the header one to one
    assert set(names) == set(_lib.SIGNATURES.keys())


def test_product_does_not_touch_the_oracle():
    """the shipped package must not import, link or call anything under oracle/"""
    for dirpath, _, files in os.walk(os.path.join(ROOT, "eigenexa_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".F90")):
                src = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "oracle" not in src.replace("orchestr", ""), f"{f} mentions the oracle"
    out = subprocess.run(["nm", "-D", os.path.join(ROOT, "eigenexa_amd", "lib", "libeigenexa_amd.so")],
                         capture_output=True, text=True).stdout
    assert "orc_" not in out


def test_no_gpu_fails_loudly():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from eigenexa_amd import _lib

    lib = _lib.load()
    assert lib.eigx_init(0) == -4  # EIGX_ERR_NO_DEVICE: there is no CPU path
    import eigenexa_amd as ee

    with pytest.raises(RuntimeError):
        ee.eigen_init()


def test_index_helpers_match_reference_formulas():
    """src/eigen_libs0.F:1825 (loop_start), :1911 (loop_end), :1995, :2079, :2163, :2247; SURVEY appendix A"""
    from eigenexa_amd import _lib

    lib = _lib.load()
    for P in (1, 2, 3, 4, 7):
        for p in range(1, P + 1):
            owned = [g for g in range(1, 60) if (g - 1) % P + 1 == p]
            for g in range(1, 60):
                ls = lib.eigx_loop_start(g, P, p)   # first local index whose global >= g
                le = lib.eigx_loop_end(g, P, p)     # last local index whose global <= g
                assert ls == 1 + sum(1 for x in owned if x < g)
                assert le == sum(1 for x in owned if x <= g)
                assert lib.eigx_owner_node(g, P, p) == (g - 1) % P + 1
                assert lib.eigx_translate_g2l(g, P, p) == (g - 1) // P + 1
                oi = lib.eigx_owner_index(g, P, p)
                assert oi == ((g - 1) // P + 1 if g in owned else -1)
            for l in range(1, 10):
                assert lib.eigx_translate_l2g(l, P, p) == (l - 1) * P + p


def test_grid_rule():
    """src/eigen_libs0.F:526-570: 1->1x1, 2->1x2, 4->2x2, 8->2x4, 6->2x3, 7->1x7"""
    from eigenexa_amd import layout

    assert [layout.grid_shape(p) for p in (1, 2, 4, 8, 6, 7, 16)] == [(1, 1), (1, 2), (2, 2), (2, 4), (2, 3),
                                                                     (1, 7), (4, 4)]
    assert layout.rank_coords(5, 8) == (1, 2)         # column-major: x = r % Px, y = r // Px
    assert layout.rank_coords(5, 8, "R") == (1, 1)


@pytest.mark.parametrize("nranks", [1, 2, 4, 6, 8])
def test_cyclic_scatter_gather_roundtrip(nranks):
    from eigenexa_amd import layout

    n = 37
    A = layout.random_symmetric(n)
    blocks = [layout.scatter_cyclic(A, nranks, r) for r in range(nranks)]
    assert np.array_equal(layout.gather_cyclic(blocks, n, n), A)
    # generators evaluated at local index sets give the same local blocks (layout independence)
    Px, Py = layout.grid_shape(nranks)
    for r in range(nranks):
        px, py = layout.rank_coords(r, nranks)
        loc = layout.random_symmetric(n, rows=np.arange(px, n, Px), cols=np.arange(py, n, Py))
        assert np.array_equal(loc, blocks[r][: loc.shape[0], : loc.shape[1]])


def test_torch_generator_is_bit_identical():
    from eigenexa_amd import layout

    n = 131
    assert np.array_equal(layout.random_symmetric(n), layout.random_symmetric_torch(n, "cpu", chunk=50).numpy())
    rows, cols = np.arange(1, n, 2), np.arange(0, n, 4)
    assert np.array_equal(layout.random_symmetric(n, rows=rows, cols=cols),
                          layout.random_symmetric_torch(n, "cpu", rows=rows, cols=cols).numpy())


def test_frank_formula():
    from eigenexa_amd import layout

    n = 50
    assert np.abs(np.linalg.eigvalsh(layout.frank(n)) - layout.frank_eigenvalues(n)).max() < 1e-9


_WORKER = r'''
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch, torch.distributed as dist
from eigenexa_amd import layout
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%(port)d", rank=int(sys.argv[1]), world_size=2)
rank = dist.get_rank()
n = 29
A = layout.random_symmetric(n)
mine = layout.scatter_cyclic(A, 2, rank)
# 1) unique-id style broadcast used by eigen_init(comm): rank 0's 128 bytes reach everyone
t = torch.arange(128, dtype=torch.uint8) if rank == 0 else torch.zeros(128, dtype=torch.uint8)
dist.broadcast(t, src=0)
assert bytes(t.tolist()) == bytes(range(128))
# 2) gather the cyclic blocks and rebuild the global matrix on every rank
Px, Py = layout.grid_shape(2)
blocks = [torch.zeros(n, (n + 1) // 2, dtype=torch.float64) for _ in range(2)]
pad = torch.zeros(n, (n + 1) // 2, dtype=torch.float64)
pad[: mine.shape[0], : mine.shape[1]] = torch.from_numpy(np.ascontiguousarray(mine))
dist.all_gather(blocks, pad)
G = layout.gather_cyclic([b.numpy() for b in blocks], n, n)
assert np.array_equal(G, A)
# 3) the row-group / column-group sums of a distributed mat-vec reproduce A @ u (the reduction's pattern)
u = np.arange(1, n + 1, dtype=np.float64)
px, py = layout.rank_coords(rank, 2)
part = np.zeros(n)
part[px::Px] = mine[: layout.local_count(n, px, Px), : layout.local_count(n, py, Py)] @ u[py::Py]
tt = torch.from_numpy(part)
dist.all_reduce(tt)
assert np.allclose(tt.numpy(), A @ u)
dist.barrier()
dist.destroy_process_group()
print("OK", rank)
'''


def test_gloo_world_size_2(tmp_path):
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = tmp_path / "worker.py"
    script.write_text(_WORKER % {"root": ROOT, "port": port})
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              text=True) for r in range(2)]
    outs = [p.communicate(timeout=180)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"OK {r}" in o, o


def test_benchmark_driver_input_format(tmp_path):
    """the reference driver's input-file format (benchmark/main2.f:262-300, benchmark/IN): comments, 8 integers
    per case, a non-positive N ends the run"""
    from eigenexa_amd import benchmark

    p = tmp_path / "IN"
    p.write_text("! N nvec bx by m t s e\n 1000     0 48 128 1 0 1 0\n!comment\n 64 64 48 128 2 2 0 1\n-1 0 0 0 0 0 0 0\n"
                 " 5 5 48 128 1 0 0 1\n")
    cases = list(benchmark.parse_input(str(p)))
    assert cases == [(1000, 0, 48, 128, 1, 0, 1, 0), (64, 64, 48, 128, 2, 2, 0, 1)]
    assert benchmark.MODES[0] == "N" and benchmark.MODES[2] == "X" and benchmark.MODES[5] == "C"
    assert benchmark._verdict(1e-9) == "PASSED" and benchmark._verdict(1e-5) == "CAUTION"
    assert benchmark._verdict(1e-3) == "FAILED"
    msgs = []
    lam = np.array([1.0, 2.0, 3.0])
    assert benchmark.w_test(lam * (1 + 1e-12), lam, msgs.append)
    assert any("Relative Error *** : PASSED" in m for m in msgs)


def test_numroc_and_block_cyclic_layout():
    """NUMROC of the C-ABI against the python restatement and a brute-force count; block-cyclic scatter/gather round
    trip (the layout eigx_solve_bc accepts); nb = 1 reduces to the cyclic layout of the EigenExa API"""
    from eigenexa_amd import _lib, layout

    lib = _lib.load()
    for n in (1, 5, 64, 100, 301):
        for nb in (1, 2, 7, 32, 64):
            for P in (1, 2, 3, 4):
                tot = 0
                for p in range(P):
                    c = layout.numroc(n, nb, p, P)
                    assert c == lib.eigx_numroc(n, nb, p, P) == len(layout.block_cyclic_indices(n, nb, p, P))
                    if nb == 1:
                        assert c == layout.local_count(n, p, P)
                    tot += c
                assert tot == n
    assert lib.eigx_numroc(10, 0, 0, 2) == -1 and lib.eigx_numroc(10, 2, 2, 2) == -1
    A = np.arange(35 * 29.0).reshape(35, 29)
    for nb in (1, 4, 16):
        blocks = [layout.scatter_block_cyclic(A, nb, 4, r) for r in range(4)]
        assert (layout.gather_block_cyclic(blocks, 35, 29, nb) == A).all()
    # nb = 1 block-cyclic == cyclic
    for r in range(4):
        assert (layout.scatter_block_cyclic(A, 1, 4, r) == layout.scatter_cyclic(A, 4, r)).all()


# ---------------------------------------------------------------------------- eigen_get_matdims >= the reference's
def _ref_cstab_optdim(n_min, n_unroll=6, delta_l1=64, delta_l2=128):
    """CSTAB_get_optdim restated (src/CSTAB.F:73-131) with the A64FX constants of src/CSTAB.h (the ones compiled in)"""
    L1_SIZE, L1_WAY, L1_LINE = 64 * 1024, 4, 256
    L2_SIZE, L2_WAY = 8 * 1024 * 1024, 16
    L1_LSIZE, L1_WINDOW, L2_LSIZE = (L1_SIZE // L1_WAY) // 8, L1_LINE // 8, (L2_SIZE // L2_WAY) // 8

    def fmod(a, b):  # Fortran MOD: sign of the dividend
        return int(np.fmod(a, b))

    n_opt = n_min
    while True:
        n_opt = (n_opt - 1) // L1_WINDOW + 1
        n_opt = (n_opt // 2) * 2 + 1
        n_opt *= L1_WINDOW
        n_delta = 0
        for lsize, way, delta in ((L1_LSIZE, L1_WAY, delta_l1), (L2_LSIZE, L2_WAY, delta_l2)):
            for i in range(1, int((n_unroll * 1.2 - 1.0) / way + 1) + 1):
                k = fmod(i * n_opt + lsize // 2, lsize) - lsize // 2
                if abs(k) <= delta // 2:
                    n_delta = (delta // 2 - k - 1) // i + 1
                    break
            if n_delta:
                break
        if n_delta == 0:
            return n_opt
        n_opt += n_delta


def _ref_matdims(n, Px, Py, m_b=128, mode="O"):
    """eigen_get_matdims of the reference's default build: eigen_get_matdims0 (src/eigen_libs0.F:1270-1343) max-ed
    with FS_get_matdims (src/eigen_libs.F:139-146, src/FS_libs.F90:356-375)"""
    if mode == "M":
        nx, ny = (n - 1) // Px + 1, (n - 1) // Py + 1
    elif mode == "L":
        nx = ((n - 1) // Px + 1 - 1) // 32 * 32 + 32
        ny = (n - 1) // Py + 1
    else:
        nm = _ref_cstab_optdim((n - 1) // Px + 1)
        NB = max(m_b, 64)

        def ext(P):
            v = (n - 1) // P + 1
            v = ((v - 1) // NB + 1) * NB + 1
            v2 = (((n - 1) // NB + 1) - 1) // P + 1
            return max(v, v2 * NB)

        larray = max(ext(Px), nm) * ext(Py)
        nx, ny = nm, (larray - 1) // nm + 1
    P = Px * Py
    n1 = (n + P - 1) // P
    return max(nx, n1 * (P // Px)), max(ny, n1 * (P // Py))


def test_matdims_not_smaller_than_reference():
    """callers allocate a(nx, ny), z(nx, ny) from eigen_get_matdims, so the extents returned here must be
    >= the reference's for the same (n, grid, m_backward, mode) -- sizes 1..70000, every grid of up to 8 ranks"""
    import ctypes as C

    from eigenexa_amd import _lib

    lib = _lib.load()
    sizes = list(range(1, 140)) + [255, 256, 257, 1000, 1024, 4095, 4096, 4097, 8192, 10000, 16384, 23168, 32768,
                                   40000, 65536, 70000]
    grids = [(1, 1), (1, 2), (2, 1), (1, 3), (2, 2), (1, 5), (2, 3), (3, 2), (1, 7), (2, 4), (4, 2), (1, 8)]
    for Px, Py in grids:
        for mode in "OML":
            for mb in (128, 48, 256):
                for n in sizes:
                    nx, ny = C.c_int(), C.c_int()
                    rc = lib.eigx_matdims_for_grid(n, Px, Py, 48, mb, mode.encode(), C.byref(nx), C.byref(ny))
                    rx, ry = _ref_matdims(n, Px, Py, mb, mode)
                    if rc == -3:   # 32-bit guard (src/eigen_libs0.F:1349-1365): the reference refuses as well
                        side = (((n - 1) // min(Px, Py) + 1 - 1) // 64 + 1) * 64
                        assert side * side >= 2 ** 31
                        continue
                    assert rc == 0 and nx.value >= rx and ny.value >= ry, (n, Px, Py, mode, mb, nx.value, ny.value, rx, ry)
                    assert nx.value >= (n + Px - 1) // Px and ny.value >= (n + Py - 1) // Py


def test_matdims_leading_dimension_avoids_channel_aliasing():
    """the nx that eigen_get_matdims recommends (mode 'O') puts consecutive columns 4 - 12 KiB apart
    modulo 16 KiB from 2048 doubles on (nx mod 2048 in [512, 1536]), stays a multiple of 32 (16-byte column loads need it
    even) and costs at most 1024 + 160 doubles over the local extent"""
    import ctypes as C

    from eigenexa_amd import _lib

    lib = _lib.load()
    for Px, Py in [(1, 1), (2, 2), (2, 4), (1, 8)]:
        for n in [100, 2047, 2048, 3000, 4096, 8192, 10000, 12289, 16384, 20000, 32768, 40000, 65536]:
            nx, ny = C.c_int(), C.c_int()
            rc = lib.eigx_matdims_for_grid(n, Px, Py, 48, 128, b"O", C.byref(nx), C.byref(ny))
            if rc == -3:
                continue
            assert rc == 0
            n1 = (n + Px - 1) // Px
            assert nx.value % 32 == 0 and nx.value >= n1
            if nx.value >= 2048:
                assert 512 <= nx.value % 2048 <= 1536, (n, Px, nx.value)
            assert nx.value <= n1 + 1024 + 160, (n, Px, nx.value)


# ------------------------------------------------- 2-D cyclic partition of the reduction step: index arithmetic on the CPU
def _mg_nty(tx, T, Lc, Px, px, Py, py):
    """tiles of tile column tx of a rank's local block (band_reduce.hip mg_nty)"""
    lc = min(tx * T + T - 1, Lc - 1)
    num = lc * Py + py - px
    return num // (Px * T) + 1 if num >= 0 else 0


@pytest.mark.parametrize("Px,Py", [(1, 2), (2, 1), (2, 2), (1, 3), (2, 3), (3, 2), (2, 4), (4, 2), (1, 8)])
def test_step_partition_covers_the_upper_triangle(Px, Py):
    """What one reduction step does on a Px x Py grid (the 2x4 grid of the 8-GPU node included, which the one-GPU box
    cannot host: it admits six processes), restated with numpy from the kernels' index formulas: every rank walks
    the tiles of its local block that mg_nty enumerates, masks by global indices, forms row / column partial sums;
    the consumer adds the Py row-sum and Px column-sum contributions of a row.  Checks (a) every element of the
    global upper triangle is visited exactly once over all ranks, (b) the assembled vector equals A_sym u, (c) the
    closed form the GPU uses to invert the tile numbering (Px | Py) agrees with the enumeration, (d) the first
    tile column with work for a tile row (kl_kernel's txmin) is the first enumerated one."""
    rng = np.random.default_rng(5)
    for L, T in ((37, 8), (64, 8), (130, 16), (257, 32)):
        A = rng.standard_normal((L, L))
        A = A + A.T
        u = rng.standard_normal(L)
        visits = np.zeros((L, L), dtype=int)
        yr = {}
        yc = {}
        for px in range(Px):
            for py in range(Py):
                rows = np.arange(px, L, Px)
                cols = np.arange(py, L, Py)
                Lr, Lc = len(rows), len(cols)
                r_sum = np.zeros(Lr)
                c_sum = np.zeros(Lc)
                ntc = -(-Lc // T) if Lc else 0
                ntiles = 0
                starts = []
                for tx in range(ntc):
                    nty = _mg_nty(tx, T, Lc, Px, px, Py, py)
                    starts.append(ntiles)
                    ntiles += nty
                    for ty in range(nty):
                        rr = rows[ty * T:(ty + 1) * T]
                        cc = cols[tx * T:(tx + 1) * T]
                        assert len(rr) > 0, "an enumerated tile has rows"
                        blk = A[np.ix_(rr, cc)]
                        strict = rr[:, None] < cc[None, :]
                        upper = rr[:, None] <= cc[None, :]
                        visits[np.ix_(rr, cc)] += upper
                        r_sum[ty * T:ty * T + len(rr)] += (blk * strict) @ u[cc]
                        c_sum[tx * T:tx * T + len(cc)] += (blk * upper).T @ u[rr]
                    # no tile below the enumerated ones touches the upper triangle
                    for ty in range(nty, -(-Lr // T) if Lr else 0):
                        assert rows[ty * T] > cols[min(tx * T + T - 1, Lc - 1)]
                # closed form of the numbering when Px divides Py (symv_kernel): column tx starts at s tx(tx-1)/2 + c1 tx
                if Py % Px == 0 and ntc > 1:
                    s = Py // Px
                    c1 = ((T - 1) * Py + py - px) // (Px * T) + 1
                    for tx in range(ntc - 1):
                        assert starts[tx] == s * (tx * (tx - 1) // 2) + c1 * tx
                # kl_kernel: first tile column with a tile in tile row ty
                for ty in range(-(-Lr // T) if Lr else 0):
                    g0 = ty * T * Px + px
                    cneed = (g0 - py + Py - 1) // Py if g0 > py else 0
                    have = [tx for tx in range(ntc) if _mg_nty(tx, T, Lc, Px, px, Py, py) > ty]
                    if cneed <= Lc - 1:
                        assert have and have[0] == cneed // T and have == list(range(cneed // T, ntc))
                    else:
                        assert not have
                yr[(px, py)] = r_sum
                yc[(px, py)] = c_sum
        iu = np.triu_indices(L)
        assert (visits[iu] == 1).all() and (np.tril(visits, -1) == 0).all()
        y = np.zeros(L)
        for r in range(L):
            for qy in range(Py):            # K_A: Py row-sum contributions, then Px column-sum contributions
                y[r] += yr[(r % Px, qy)][r // Px]
            for qx in range(Px):
                y[r] += yc[(qx, r % Py)][r // Py]
        assert np.allclose(y, A @ u, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("Px,Py,row_major", [(1, 2, 0), (2, 1, 0), (2, 2, 0), (1, 3, 0), (2, 3, 1), (3, 2, 0), (1, 5, 0), (2, 4, 0), (2, 4, 1),
                                              (4, 2, 0), (1, 8, 0), (8, 1, 0), (1, 7, 0)])
def test_owner_directed_step_exchange(Px, Py, row_major):
    """Round 4's distribution of the per-step panel work, restated with numpy from the kernels' index formulas
    (band_reduce.hip: own_of / own_row, kl_chunk's destinations, mg_partial, the X message layout), for every grid up to
    8 ranks -- the 2 x 4 grid of the 8-GPU node included, which the one-GPU box cannot host.  Rows are dealt to the ranks in
    groups of 16: row r belongs to world rank (r // 16) % P at owned index ((r // 16) // P) * 16 + r % 16.
    Checks: (a) the owner map is a bijection onto [0, rows owned) per rank, ascending with the row, and the float
    reciprocal the GPU uses for g // P is exact; (b) Y: every rank sends the sum of local row li (column lj) to the owner of
    its global row only (rows L-1, L-2 to everybody) at the offsets mg_partial reads, and the owner, adding its Py + Px
    entries, gets A_sym u for exactly its rows -- nobody reads an entry that was not written in this step; (c) the shares
    of the panel dots over the ranks' own rows add up to the full dot products; (d) X: the owners' x, W rows at their
    owned indices reassemble the full vectors on every rank; (e) the rows below L that a rank owns come first in its
    owned order (what K_P's dot role and the host's own_count assume)."""
    P = Px * Py
    rng = np.random.default_rng(7)
    KA = 16

    def world(qx, qy):
        return qx * Py + qy if row_major else qx + qy * Px

    inv = np.float32(1.0) / np.float32(P)
    for L in (1, 2, 15, 16, 17, 33, 130, 257, 1000):
        n = L + 5                                    # the window strides come from n, the step works on rows < L
        nxs = (-(-n // Px) + 7) // 8 * 8
        nys = (-(-n // Py) + 7) // 8 * 8
        nown = -(-(-(-n // KA)) // P) * KA
        r = np.arange(n)
        g = r // KA
        own = g % P
        oidx = (g // P) * KA + r % KA
        # (a) exact float division, bijection, order
        q32 = ((g.astype(np.float32) + np.float32(0.5)) * inv).astype(np.int64)
        assert (q32 == g // P).all()
        for me in range(P):
            mine = r[own == me]
            assert (oidx[own == me] == np.arange(len(mine))).all() or len(mine) == 0 or \
                (np.diff(oidx[own == me]) > 0).all()                     # ascending with the row
            assert oidx[own == me].max(initial=-1) < nown
            # own_row inverts it
            o = oidx[own == me]
            assert ((((o // KA) * P + me) * KA) + o % KA == mine).all()
            # (e) rows below L come first: count = full groups below L owned + the partial group if mine
            gfull, rem = L // KA, L % KA
            cnt = len([gg for gg in range(gfull) if gg % P == me]) * KA + (rem if (rem and gfull % P == me) else 0)
            below = oidx[(own == me) & (r < L)]
            assert len(below) == cnt and (np.sort(below) == np.arange(cnt)).all()
        # (b) the Y exchange of one step
        A = rng.standard_normal((L, L))
        A = A + A.T
        u = rng.standard_normal(L)
        # window of destination d: [source][NB=1 row sums: nxs | column sums: nys], NaN = never written this step
        win = np.full((P, P, nxs + nys), np.nan)
        for px in range(Px):
            for py in range(Py):
                src = world(px, py)
                rows = np.arange(px, L, Px)
                cols = np.arange(py, L, Py)
                blk = A[np.ix_(rows, cols)]
                strict = rows[:, None] < cols[None, :]
                upper = rows[:, None] <= cols[None, :]
                rsum = (blk * strict) @ u[cols] if len(cols) else np.zeros(len(rows))
                csum = (blk * upper).T @ u[rows] if len(rows) else np.zeros(len(cols))
                for li, gr in enumerate(rows):
                    dests = range(P) if gr >= L - 2 else [own[gr]]
                    for d in dests:
                        win[d, src, li] = rsum[li]
                for lj, gc in enumerate(cols):
                    dests = range(P) if gc >= L - 2 else [own[gc]]
                    for d in dests:
                        win[d, src, nxs + lj] = csum[lj]
        y = A @ u
        for me in range(P):
            for gr in r[(own == me) & (r < L)]:
                acc = 0.0
                for t in range(Py + Px):                                  # mg_partial
                    if t < Py:
                        qx, qy, off = gr % Px, t, gr // Px
                    else:
                        qx, qy, off = t - Py, gr % Py, nxs + gr // Py
                    v = win[me, world(qx, qy), off]
                    assert not np.isnan(v), (L, me, gr, t)
                    acc += v
                assert abs(acc - y[gr]) <= 1e-12 * (1 + abs(y[gr]))
            for c in (L - 1, L - 2):                                      # P(c, :) of the next block columns: on every rank
                if c < 0:
                    continue
                acc = sum(win[me, world(c % Px, t), c // Px] for t in range(Py)) + \
                    sum(win[me, world(t, c % Py), nxs + c // Py] for t in range(Px))
                assert abs(acc - y[c]) <= 1e-12 * (1 + abs(y[c]))
        # (c) panel dots: shares over the ranks' own rows
        U = rng.standard_normal((L, 5))
        shares = [U[(own[:L] == me), :].T @ u[own[:L] == me] for me in range(P)]
        assert np.allclose(sum(shares), U.T @ u, rtol=1e-12, atol=1e-12)
        # (d) X: owners' rows at their owned indices reassemble the vector
        x = rng.standard_normal(L)
        msg = np.full((P, nown), np.nan)
        for me in range(P):
            sel = (own[:L] == me)
            msg[me, oidx[:L][sel]] = x[sel]
        assert (msg[own[:L], oidx[:L]] == x).all()


@pytest.mark.parametrize("Px,Py", [(1, 2), (2, 1), (2, 2), (1, 3), (3, 1), (2, 3), (3, 2), (2, 4), (4, 2), (1, 8), (8, 1)])
def test_distributed_transpose_plan_assembles_the_transpose(Px, Py):
    """KMATH_EIGEN_GEV on several ranks symmetrises A and transposes B^(-1/2) by an all-to-all whose pieces come from
    eigx_transpose_plan (pure arithmetic in the library: Chinese remainder theorem on lcm(Px, Py)).  Restated with numpy
    for every grid up to 8 ranks (2 x 4 included): every rank packs the pieces the plan names from its cyclic block, the
    receivers place them by the plan's receive side -- the assembled blocks must be exactly the cyclic blocks of A^T,
    every element sent once, and send / receive sides of a pair must agree."""
    import ctypes as C

    from eigenexa_amd import _lib

    lib = _lib.load()
    rng = np.random.default_rng(11)

    def plan(px, py, qx, qy):
        v = [C.c_int() for _ in range(5)]
        assert lib.eigx_transpose_plan(Px, Py, px, py, qx, qy, *[C.byref(x) for x in v]) == 0
        return [x.value for x in v]

    for n in (1, 2, 7, 24, 37):
        A = rng.standard_normal((n, n))
        Z = {(px, py): np.full((len(range(px, n, Px)), len(range(py, n, Py))), np.nan) for px in range(Px) for py in range(Py)}
        sent = np.zeros((n, n), dtype=int)
        for px in range(Px):
            for py in range(Py):
                Aloc = A[px::Px, py::Py]                      # my cyclic block: rows j = px mod Px, columns i = py mod Py
                for qx in range(Px):
                    for qy in range(Py):
                        si0, sj0, _, _, L = plan(px, py, qx, qy)
                        ri0, rj0 = plan(qx, qy, px, py)[2:4]
                        assert (si0, sj0) == (ri0, rj0), "the two sides of a pair disagree"
                        if si0 < 0 or sj0 < 0:
                            continue
                        for i in range(si0, n, L):            # Z(i, j) = A(j, i): I hold row j, column i
                            for j in range(sj0, n, L):
                                assert j % Px == px and i % Py == py and i % Px == qx and j % Py == qy
                                Z[(qx, qy)][i // Px, j // Py] = Aloc[j // Px, i // Py]
                                sent[j, i] += 1
        assert (sent == 1).all()
        for (px, py), blk in Z.items():
            assert np.array_equal(blk, A.T[px::Px, py::Py])


def test_matrix_type_10_reads_w_dat(tmp_path, monkeypatch):
    """matrix type 10 of the reference driver (benchmark/mat_set.f:205-216, :714-729): the spectrum comes from the file
    'W.dat' in the working directory (free format, first n numbers); without the file its content is regenerated
    (10 + sin(k - 1) printed with six significant digits -- the formula was checked against all 100000 entries)"""
    from eigenexa_amd import layout

    monkeypatch.chdir(tmp_path)
    gen = layout.spectrum(50, 10)
    assert gen[0] == 10.0 and abs(gen[1] - 10.8415) < 1e-12 and abs(gen[4] - 9.2432) < 1e-12    # W.dat lines 1, 2, 5
    (tmp_path / "W.dat").write_text("\n".join(f"{1.5 + 0.25 * k}" for k in range(60)) + "\n")
    got = layout.spectrum(40, 10)
    assert len(got) == 40 and got[0] == 1.5 and got[39] == 1.5 + 0.25 * 39
    A, lam = layout.reference_matrix(40, 10)
    assert np.abs(np.linalg.eigvalsh(A) - lam).max() < 1e-13 * 40
    with pytest.raises(ValueError):
        layout.spectrum(100, 10)


def test_matrix_market_reader(tmp_path):
    """matrix types -1 / -2 of the reference driver (benchmark/mat_set.f:218-330, mat_dim_get :461-533): coordinate
    triples of a symmetric matrix, comment lines, Fortran D exponents"""
    from eigenexa_amd import layout

    p = tmp_path / "A.mtx"
    p.write_text("%%MatrixMarket matrix coordinate real symmetric\n% a comment\n4 4 5\n1 1 2.0\n2 1 -1.0\n3 3 1.5D0\n4 2 0.25\n4 4 3\n")
    assert layout.matrix_market_dim(str(p)) == 4
    A = layout.read_matrix_market(str(p), 4)
    ref = np.array([[2, -1, 0, 0], [-1, 0, 0, 0.25], [0, 0, 1.5, 0], [0, 0.25, 0, 3.0]])
    assert np.array_equal(A, ref)
    with pytest.raises(ValueError):
        layout.read_matrix_market(str(p), 5)


def test_bench_dump_columns_fit_the_size_cap():
    """bench.py --dump-outputs: eigenvalues plus the chosen eigenvector columns stay within 64 MiB at every N (the .npy
    headers included); every column while they fit, else a seeded, sorted, duplicate-free sample, the same every time"""
    from bench import dump_columns

    for n in (1, 2, 640, 2508, 2509, 2560, 8192, 16384, 32768, 65536, 131072):
        sel = dump_columns(n)
        assert 8 * n + 8 * n * len(sel) + 2 * 128 <= 64 << 20, n
        assert len(sel) >= 1 and sel.min() >= 0 and sel.max() < n and (np.diff(sel) > 0).all(), n
        assert np.array_equal(sel, dump_columns(n)), n
        if 8 * n * n <= 48 << 20:
            assert len(sel) == n, n
        else:
            assert len(sel) < n and 8 * n * (len(sel) + 1) > 48 << 20, n   # as many columns as fit
    assert len(dump_columns(8192)) == 768 and len(dump_columns(32768)) == 192


def test_bench_spawns_its_own_ranks():
    """`python bench.py --gpus N` without a launcher starts N ranks itself (before anything touches a GPU) and relays
    rank 0's line and the worst exit code; `--gpus N` under a different WORLD_SIZE is refused."""
    import json
    import subprocess

    bench = os.path.join(ROOT, "bench.py")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["EIGX_BENCH_DRYRUN"] = "1"
    r = subprocess.run([sys.executable, bench, "--gpus", "4"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0])["n_gpus"] == 4
    env["EIGX_BENCH_DRYRUN"] = "fail2"           # rank 2 exits with code 3: the launcher reports it
    r = subprocess.run([sys.executable, bench, "--gpus", "4"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 3
    env["EIGX_BENCH_DRYRUN"] = "1"
    env["WORLD_SIZE"] = "2"
    env["RANK"] = "0"
    r = subprocess.run([sys.executable, bench, "--gpus", "8"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "WORLD_SIZE" in r.stderr


def test_reference_benchmark_sources_find_their_symbols_in_the_module():
    """Boundary check: every entity of eigen_libs_mod / eigen_blacs_mod that the reference's OWN benchmark sources
    (benchmark/main2.f, mat_set.f, w_test.f, ev_test.f) call, and every keyword argument they pass, exists in
    eigenexa_amd/fortran/eigen_libs_mod.F90 with that dummy-argument name.  The calls and keywords were read from those
    sources as TEXT into tests/golden/reference_calls.json (tools/make_reference_calls.py): a `flang -fsyntax-only`
    pass over them is not possible, because they also `use mpi` and the image's mpi.mod is in gfortran's format (unreadable
    by flang) -- writing a replacement module would be a stand-in for something the image lacks, which this project's
    rules exclude."""
    import json

    mod = open(os.path.join(ROOT, "eigenexa_amd", "fortran", "eigen_libs_mod.F90")).read().lower()
    public = set()
    for m in re.finditer(r"^\s*public\s*::\s*(.+)$", mod, re.M):
        public |= {t.strip() for t in m.group(1).split("!")[0].split(",") if t.strip()}
    # dummy-argument names per procedure (generic interfaces: union over their module procedures)
    dummies = {}
    for m in re.finditer(r"^\s*(?:[a-z0-9_()]+\s+)*(?:subroutine|function)\s+([a-z0-9_]+)\s*\(([^)]*)\)", mod, re.M):
        dummies[m.group(1)] = {a.strip() for a in m.group(2).split(",") if a.strip()}
    for m in re.finditer(r"^\s*interface\s+([a-z0-9_]+)\s*$(.*?)^\s*end interface", mod, re.M | re.S):
        names = re.findall(r"module procedure\s+(.+)", m.group(2))
        args = set()
        for line in names:
            for nm in line.split(","):
                args |= dummies.get(nm.strip(), set())
        dummies[m.group(1)] = args
    with open(os.path.join(ROOT, "tests", "golden", "reference_calls.json")) as f:
        calls = json.load(f)
    used = set(calls["used"])
    kw = {k: set(v) for k, v in calls["keywords"].items()}
    assert {"eigen_init", "eigen_sx", "eigen_s", "eigen_free", "eigen_get_matdims", "eigen_get_comm",
            "eigen_get_blacs_context", "eigen_memory_internal", "eigen_loop_start", "eigen_owner_node"} <= used   # the stored list holds the calls
    missing = sorted(n for n in used if n not in public)
    assert not missing, f"the reference's benchmark sources use {missing}, which eigen_libs_mod.F90 does not export"
    for name, keys in kw.items():
        bad = sorted(k for k in keys if k not in dummies.get(name, set()))
        assert not bad, f"{name}: keyword argument(s) {bad} of the reference's callers are not dummy names here ({sorted(dummies.get(name, []))})"
