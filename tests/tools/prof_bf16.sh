#!/bin/bash
# One single-stream profile of bench.py --full (5 steps) -> <outdir>/pb<tag>/ and <outdir>/pb<tag>.json.  usage: prof_bf16.sh [dtype] [tag] [outdir]
ROOT=${GRAFT_REPO_ROOT:-/root/repo}
OUT=$(realpath -m "${3:-/tmp/tem_prof}")
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/pb$2; mkdir -p $OUT
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/pb$2 -- python3 $ROOT/bench.py --full --dtype ${1:-bf16} --steps 5 --warmup 2 --no-cpu-baseline --sustain 0 --single-stream > $OUT/pb$2.json 2> /dev/null
