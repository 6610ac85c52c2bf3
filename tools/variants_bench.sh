#!/bin/bash
# Runs ON THE GPU BOX: the default bench (three batches in flight, no CPU legs) once per environment setting.
# usage: tools/variants_bench.sh "" "VAR=value ..." ... [-- bench flags]
SETS=()
while [ $# -gt 0 ] && [ "$1" != "--" ]; do SETS+=("$1"); shift; done
[ "$1" == "--" ] && shift
J=$(mktemp)
for s in "${SETS[@]}"; do
  env CM3D_BENCH_CACHE=/tmp/cm3d_bench_cache $s timeout -k 10 300 python3 bench.py --full --cpu-sample 0 --no-secondary --steps 300 --warmup 20 "$@" > $J 2> $J.err || { echo "failed: $s"; tail -3 $J.err; continue; }
  python3 -c "
import json
d=json.load(open('$J'))
print('${s:-default}:', d['value'], 'frames/s', d['ms_per_step'], 'ms/step; project in flight', d['roofline']['avg_launch_ms'], 'alone', d['roofline']['avg_launch_ms_alone'], d['kernels']['stage_ms_one_batch_alone'])
"
done
