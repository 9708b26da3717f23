#!/bin/bash
# usage (on the GPU box, from the repository root): bash tools/ab_bench.sh <other libptm_engine.so> [runs] [out dir]
# bench.py at its default arguments, the other build (PTM_ENGINE_LIB) and this tree's alternating, a fresh process and a time
# limit per run; stops at the first failure.  One JSON line per run in <out dir>/ab_other.jsonl and ab_this.jsonl.
set -o pipefail
OTHER=$(readlink -f "$1"); N=${2:-5}; OUT=${3:-ab/bench}
mkdir -p $OUT
: > $OUT/ab_other.jsonl; : > $OUT/ab_this.jsonl
one() {
  if [ -n "$2" ]; then export PTM_ENGINE_LIB=$2; else unset PTM_ENGINE_LIB; fi
  timeout -k 10 150 python bench.py --steps 100 --warmup 10 2>>$OUT/ab_$1.err | tail -1 >> $OUT/ab_$1.jsonl || return 1
  tail -1 $OUT/ab_$1.jsonl | cut -c1-300
}
for i in $(seq $N); do
  one other $OTHER || exit 1
  one this "" || exit 1
done
