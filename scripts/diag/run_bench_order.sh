#!/bin/bash
OUT=$(cd "$(dirname "$0")/../.." && pwd)/diag_out; mkdir -p $OUT    # results of this script
R=$GRAFT_REPO_ROOT
cd $R
for v in parallel pqmf_first stft_first; do
  for nb in 2 3; do
  IAS_BENCH_CONSUMERS=$v python3 bench.py --full --no-cpu-baseline --buffers $nb > $OUT/bench_order_$v$nb.json 2> $OUT/bench_order_$v$nb.err
  python3 -c "
import json; d=json.load(open('$OUT/bench_order_$v$nb.json')); print('$v buffers $nb', d['ms_per_step'], d['ms_per_step_min'])"
  done
done
