# kernel trace of the stage-1-to-BAM leg (every step under its own timeout: a profiler run that hangs costs box minutes)
# usage: bash tools/bamtrace.sh [output directory, default a new one under /tmp]
set -u
out=${1:-$(mktemp -d /tmp/bamtrace.XXXXXX)}; kt=$out/kt; cache=$(mktemp -d /tmp/telr_cache.XXXXXX)
mkdir -p $out $kt
export TMPDIR=/tmp
timeout 200 python3 bench.py --data-cache $cache --no-cpu-baseline --loci 0 --no-stream-leg --steps 1 --warmup 0 --bam-leg none > /dev/null 2>&1
rm -rf $kt/*
timeout 150 rocprofv3 --kernel-trace --stats --output-format csv -d $kt -- python3 bench.py --data-cache $cache --require-cache --no-cpu-baseline --loci 0 --no-stream-leg --steps 2 --warmup 1 --full > $out/bench_bam_under_rocprof.json 2>/dev/null
echo "rocprof exit $?"
rm -rf $cache
f=$(ls $kt/*/*kernel_stats.csv 2>/dev/null | head -1)
[ -n "$f" ] && python3 tools/prof_summary.py $kt | grep -E "^kernel|bam|bgzf|widen|iota|blk_first" | tee $out/bam_kernel_trace_summary.txt
