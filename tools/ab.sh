#!/bin/bash
# A/B of experimental builds (tools/variants/*.so, same ABI) in one box session: kernel ms per variant, twice, interleaved
cd "$(dirname "$0")/.."
OUT=${OUT:-$(mktemp -d)}
for round in 1 2; do
for v in "$@"; do
  MFCC_HIP_LIB=$PWD/tools/variants/$v.so timeout -k 10 200 python3 bench.py --full --no-cpu-baseline --no-config5 $AB_ARGS > $OUT/ab_$v.json 2> $OUT/ab_$v.err || { echo "$v FAILED"; tail -3 $OUT/ab_$v.err; continue; }
  python3 -c "
import json; b=json.loads(open('$OUT/ab_$v.json').read().strip().splitlines()[-1]); print('%-24s %.4f ms/step  kernel %.4f ms  %.3f G frames/s' % ('$v', b['ms_per_step'], b['roofline']['kernel_ms'], b['value']/1e9))"
done; done
