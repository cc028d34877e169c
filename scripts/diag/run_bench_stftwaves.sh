#!/bin/bash
OUT=$(cd "$(dirname "$0")/../.." && pwd)/diag_out; mkdir -p $OUT    # results of this script
R=$GRAFT_REPO_ROOT
cd $R
for w in 4 8; do
  IAS_STFT_WAVES=$w python3 bench.py --full --no-cpu-baseline > $OUT/bench_swv_$w.json 2>/dev/null
  python3 -c "
import json; d=json.load(open('$OUT/bench_swv_$w.json')); print('stft waves/wg', $w, d['ms_per_step'], d['ms_per_step_min'])"
  IAS_STFT_WAVES=$w python3 scripts/diag/time_stft_parts.py 2>&1 | grep loss
done
