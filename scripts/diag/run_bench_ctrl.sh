#!/bin/bash
OUT=$(cd "$(dirname "$0")/../.." && pwd)/diag_out; mkdir -p $OUT    # results of this script
R=$GRAFT_REPO_ROOT
cd $R
run() { name=$1; shift; env "$@" python3 bench.py --full --no-cpu-baseline > $OUT/bench_$name.json 2>$OUT/bench_$name.err; python3 -c "
import json; d=json.load(open('$OUT/bench_$name.json')); print('$name', d['ms_per_step'], d['ms_per_step_min'])"; }
run ctrl_late A=1
run ctrl_early IAS_BENCH_EARLY_CTRL=1
