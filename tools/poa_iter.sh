#!/bin/bash
# POA iteration aid: the consensus parity tests, the loci leg's kernel trace, and (given a build of the library with -DPOA_PROF) the
# share of a window's wave time per phase.   usage: bash tools/poa_iter.sh <tag> [config] [path of the -DPOA_PROF library]
set -u
tag=${1:-poa}; cfg=${2:-c2}; prof_lib=${3:-}
timeout 900 python3 -m pytest tests/test_gpu_consensus.py -x -q -m gpu 2>&1 | tail -3
bash tools/loci_trace.sh $tag $cfg
if [ -n "$prof_lib" ] && [ -f "$prof_lib" ]; then
  cache=$(mktemp -d /tmp/c.XXXX)
  TELR_LIB=$(realpath "$prof_lib") timeout 800 python3 bench.py --config $cfg --data-cache $cache --bam-leg none --no-stream-leg --no-default-aligner-leg --no-shard-leg --no-cpu-baseline --no-upstream-check --steps 1 --warmup 0 --full 2>&1 >/dev/null | grep "poa prof" | tail -2
  rm -rf $cache
fi
