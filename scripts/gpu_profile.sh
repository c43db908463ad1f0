#!/bin/bash
# rocprofv3 kernel-trace stats and a separate FETCH_SIZE PMC pass over the full bench line
# (64 GiB); output under profiles/out/ (or $PROFILE_OUT).
cd "$(dirname "$0")/.." || exit 1
R="$(pwd)"; export TMPDIR=/tmp; OUT="${PROFILE_OUT:-$R/profiles/out}"; mkdir -p "$OUT"
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run --output-format csv -- python bench.py --full --steps 5 --warmup 1 --cpu-baseline 0 --host-inclusive-gib 0 ${BENCH_ARGS:-} > "$OUT/prof_trace.log" 2>&1
rc=$?; echo "trace rc=$rc"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT/pmc_fetch" -o run -- python bench.py --full --steps 3 --warmup 1 --cpu-baseline 0 --host-inclusive-gib 0 ${BENCH_ARGS:-} > "$OUT/prof_pmc.log" 2>&1
rc=$?; echo "pmc rc=$rc"; [ $rc -eq 0 ] || exit $rc
python profiles/collect_traffic.py "$OUT/pmc_fetch" > "$OUT/traffic.log" 2>&1
echo "collect rc=$?"
