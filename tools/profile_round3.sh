#!/bin/bash
# Round-3 evidence: full bench line, kernel stats (CSV) of the N=8192 bench and of one N=32768 solve, written under OUTDIR.
# Run from the repo root on the GPU box: tools/profile_round3.sh OUTDIR
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
out=${1:?usage: tools/profile_round3.sh OUTDIR}
mkdir -p "$out"
python bench.py --full > "$out"/bench.json 2> "$out"/bench.err
echo "bench rc=$?"
rocprofv3 --kernel-trace --stats --output-format csv -d "$out"/prof8192 -o p -- python3 bench.py --no-cpu-baseline --no-extra > "$out"/bench_under_rocprof.json 2> "$out"/bench_under_rocprof.err
rocprofv3 --kernel-trace --stats --output-format csv -d "$out"/prof32768 -o p -- python3 bench.py --size 32768 --steps 1 --warmup 1 --mf 256 --no-cpu-baseline --no-extra > "$out"/bench_n32768_under_rocprof.json 2> "$out"/bench_n32768_under_rocprof.err
find "$out" -name "*kernel_trace.csv" -delete
find "$out" -name "*.db" -delete
ls -la "$out" "$out"/prof8192/* "$out"/prof32768/* 2>/dev/null | head -30
tail -c 400 "$out"/bench.json
