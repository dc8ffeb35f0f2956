"""The one-GPU trailing update in a rocprofv3 kernel trace (CSV): duration of the tri-mode ring-kernel launches.
usage: short_k_trace_table.py reduce <kernel_trace.csv> [N=8192] [m=64]   launches of the LAST reduction against nr
       short_k_trace_table.py lab <kernel_trace.csv>                      tools/gpu_gemm2_lab.py short: median per shape
A launch with t = ceil(nr / 128) tile rows updates t (t + 1) / 2 tiles: 2 K 128^2 flop and 2 * 8 * 128^2 bytes of C each,
so at one K the MFMA work and the C traffic are both proportional to the tile count and a fit separates only their sum
(the slope per tile) from the launch's fixed cost; the lab's shapes at several K separate the two."""
import csv, sys, statistics

mode, path = sys.argv[1], sys.argv[2]
rows = [r for r in csv.DictReader(open(path)) if "gemm2_kernel" in r["Kernel_Name"]]
def dur(r): return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3   # us
def fit(x, y):
    n = len(x); mx = sum(x) / n; my = sum(y) / n
    s = sum((a - mx) * (b - my) for a, b in zip(x, y)) / sum((a - mx) ** 2 for a in x)
    return s, my - s * mx
if mode == "reduce":
    N = int(sys.argv[3]) if len(sys.argv) > 3 else 8192
    m = int(sys.argv[4]) if len(sys.argv) > 4 else 64
    K = 2 * m
    nl = (N - 1) // m
    last = rows[-nl:]
    print(f"{len(rows)} ring-kernel launches in the trace, {nl} per reduction; kernel: {last[0]['Kernel_Name'][:90]}")
    tiles, ds = [], []
    for j, r in enumerate(last):
        nr = N - m * (j + 1)
        t = (nr + 127) // 128
        tiles.append(t * (t + 1) // 2); ds.append(dur(r))
        if j % 8 == 0 or j == nl - 1:
            print(f"  nr={nr:5d} tiles={tiles[-1]:5d} grid={r.get('Grid_Size', r.get('Grid_Size_X', '?')):>8}  {ds[-1]:8.1f} us")
    big = [(a, b) for a, b in zip(tiles, ds) if a >= 512]   # at least one full generation of 512 workgroup slots
    s, c = fit([a for a, _ in big], [b for _, b in big])
    fl, by = 2.0 * K * 128 * 128, 2.0 * 8 * 128 * 128
    print(f"total {sum(ds)*1e-3:.2f} ms, avg {sum(ds)/len(ds):.1f} us; fit over tiles >= 512: {s*1e3:.1f} ns per tile + {c:.1f} us")
    print(f"  per tile at K={K}: {fl/s*1e-6:.1f} TFLOP/s if it were all MFMA, {by/s*1e-6:.2f} TB/s if it were all C traffic")
else:
    per = 12   # launches per shape in the lab's "short" mode, in the order it prints the shapes
    for q in range(0, len(rows), per):
        v = [dur(r) for r in rows[q + 1:q + per]]   # the first launch of a shape is the warm-up
        r = rows[q]
        print(f"  shape {q // per}: grid={r.get('Grid_Size', r.get('Grid_Size_X', '?')):>9} n={len(v):3d} median {statistics.median(v):8.1f} us"
              f"  min {min(v):8.1f}  max {max(v):8.1f}   {r['Kernel_Name'][:100]}")
