#!/bin/bash
# Run on the GPU box from the repo root: tools/ab_orb.sh ROUNDS ab/libA.so ab/libB.so ...
# A/B timing of builds of libccm_hot.so on ONE box (box-to-box spread of k_fast_cells is ~3 %, the effects looked for are smaller):
# the front-end leg of bench.py per library, the libraries interleaved, ROUNDS times.
# AB_STEPS=N times N steps per run instead of bench.py's 20: a window of 20 steps is 19 ms, and one build's step time then varies by
# 0.02-0.03 ms from run to run; at 200 steps by 0.004 ms (profiles/orb_lanes_ab.txt).
# AB_KERNEL=k_orient_desc prints that kernel's time of the profiled pass beside the bench line's dominant kernel (profiles/od_diet_ab.txt).
rounds=$1; shift
steps=${AB_STEPS:-20}
also=${AB_KERNEL:-}
err=$(mktemp)
for r in $(seq $rounds); do
  for lib in "$@"; do
    CCM_HOT_LIB=$PWD/$lib timeout -k 10 120 python3 bench.py --full --no-cpu --no-gba --no-extra --steps $steps 2> "$err" | grep '^{' | python3 -c "
import sys, json
d = json.loads(sys.stdin.readline()); r = d['roofline']
also = '  $also %.4f ms' % d['kernels'].get('$also', {}).get('ms_per_step', 0) if '$also' else ''
print('$lib round $r: step %.4f ms  value %.1f  %s %.4f ms  k_octree %.4f ms%s' % (d['ms_per_step'], d['value'], r['kernel'], r['algorithmic_bytes_per_launch'] / r['achieved'] / 1e6, d['kernels'].get('k_octree', {}).get('ms_per_step', 0), also))
" || { tail -5 "$err"; exit 1; }
  done
done
