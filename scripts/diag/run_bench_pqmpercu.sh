#!/bin/bash
OUT=$(cd "$(dirname "$0")/../.." && pwd)/diag_out; mkdir -p $OUT    # results of this script
R=$GRAFT_REPO_ROOT
cd $R
for w in 1 2 3; do
  IAS_PQM_PERCU=$w python3 bench.py --full --no-cpu-baseline > $OUT/bench_pp_$w.json 2>/dev/null
  python3 -c "
import json; d=json.load(open('$OUT/bench_pp_$w.json')); print('pqmf wgs/cu', $w, d['ms_per_step'], d['ms_per_step_min'])"
done
for w in 2 3; do
  IAS_VOICE_PERCU=$w python3 bench.py --full --no-cpu-baseline > $OUT/bench_vp_$w.json 2>/dev/null
  python3 -c "
import json; d=json.load(open('$OUT/bench_vp_$w.json')); print('render wgs/cu', $w, d['ms_per_step'], d['ms_per_step_min'])"
done
