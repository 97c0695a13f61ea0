#!/bin/bash
# Same-box A/B of kernel builds on the headline alone (config 2, 1 024 walkers), the libraries taken in turn, REPS runs each:
#   [REPS=4] bash tools/ab_headline.sh ab/libA.so ab/libB.so ...        (GPU box; one call, one box)
# Prints one line per run (kernel_ms_avg, value) and, at the end, median and max - min per library.  A change counts on the
# headline when its median kernel time is below the parent's by more than twice the parent's max - min (docs/EXPERIMENTS.md).
set -o pipefail
REPS=${REPS:-4}
LOG=$(mktemp)
for rep in $(seq $REPS); do
  for lib in "$@"; do
    MAGPROP_AMD_LIB=$PWD/$lib timeout -k 10 300 python bench.py --no-cpu-baseline --no-mcmc --no-extra 2>/dev/null | \
      python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print('$lib', 'kernel_ms_avg %.5f value %.4f M' % (d['roofline']['kernel_ms_avg'], d['value']/1e6))" | tee -a $LOG || exit 1
  done
done
python3 - $LOG <<'PY'
import statistics, sys
runs = {}
for line in open(sys.argv[1]):
    f = line.split()
    runs.setdefault(f[0], []).append(float(f[2]))
for lib, v in runs.items():
    print(f"{lib}: median {statistics.median(v):.5f} ms, max - min {max(v) - min(v):.5f} ms over {len(v)} runs")
PY
rm -f $LOG
