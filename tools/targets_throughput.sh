#!/bin/bash
# The command line on bench.py's configs[2] database (its cached copy, built if missing) for N 2 kb queries: the 20 best
# pairs per query (-t -n 20) and the 20 best queries per target (-r 20), three alternating runs of each, default
# PRB_BATCH.  Prints wall time, queries/s, peak RSS, output bytes and lines of every run, and gives the device time and
# the launch counts of the stages "summary", "top" and "targets" (one batch of the same queries through the C ABI, once
# into a top-N table and once into a per-target table).
# Every step runs under a time limit of its own; the first failure ends the script.
# usage: tools/targets_throughput.sh [N=64]
N=${1:-64}
K=20
HERE=$(cd "$(dirname "$0")/.." && pwd)
W=${BENCH_WORKDIR:-$(cd "$HERE" && python3 -c "import bench; print(bench.default_workdir())")}
BIN=$HERE/priblast_amd/bin/pRIblast-hip
DB=$W/db_s50000x2000
# run NAME CMD...: CMD under a time limit; its wall time, queries/s and peak RSS; the size of its output file
run() {
  local name=$1
  shift
  python3 -c 'import resource, subprocess, sys, time
t = time.time()
rc = subprocess.call(["timeout", "-k", "10", "300"] + sys.argv[3:])
w = time.time() - t
rss = resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss / 1024
print(f"{sys.argv[1]}: {w:.2f} s, {int(sys.argv[2]) / w:.2f} queries/s, peak RSS {rss:.0f} MB")
sys.exit(rc)' "$name" "$N" "$@" && echo "$name: $(stat -c %s "$W/tg_${name%_*}.out") bytes, $(($(wc -l < "$W/tg_${name%_*}.out") - 3)) lines"
}
(cd "$HERE" && BENCH_WORKDIR="$W" timeout -k 10 900 python3 -c "import bench; bench.prepare_database()") 2> "$W.build.log" &&
  timeout -k 10 60 python3 "$HERE/tools/gen_synthetic.py" -n "$N" -L 2000 --seed 2 --prefix q -o "$W/tg_q.fa" &&
  run top_1 "$BIN" ris -t -n "$K" -i "$W/tg_q.fa" -o "$W/tg_top.out" -d "$DB" &&
  run targets_1 "$BIN" ris -r "$K" -i "$W/tg_q.fa" -o "$W/tg_targets.out" -d "$DB" &&
  run top_2 "$BIN" ris -t -n "$K" -i "$W/tg_q.fa" -o "$W/tg_top.out" -d "$DB" &&
  run targets_2 "$BIN" ris -r "$K" -i "$W/tg_q.fa" -o "$W/tg_targets.out" -d "$DB" &&
  run top_3 "$BIN" ris -t -n "$K" -i "$W/tg_q.fa" -o "$W/tg_top.out" -d "$DB" &&
  run targets_3 "$BIN" ris -r "$K" -i "$W/tg_q.fa" -o "$W/tg_targets.out" -d "$DB" &&
  (cd "$HERE" && timeout -k 10 600 python3 "$HERE/tools/targets_stage_times.py" "$W/tg_q.fa" "$DB" "$K") &&
  rm -f "$W/tg_top.out" "$W/tg_targets.out"
