#!/bin/bash
OUT=$(cd "$(dirname "$0")/../.." && pwd)/diag_out; mkdir -p $OUT    # results of this script
R=$GRAFT_REPO_ROOT
cd $R
for w in ${WGS:-256 384 512 768 1024}; do
  IAS_STFT_WGS=$w python3 bench.py --full --no-cpu-baseline > $OUT/bench_sw_$w.json 2>/dev/null
  python3 -c "
import json; d=json.load(open('$OUT/bench_sw_$w.json')); print('stft wgs', $w, d['ms_per_step'], d['ms_per_step_min'])"
done
