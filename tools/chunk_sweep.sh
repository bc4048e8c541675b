#!/bin/bash
# k_icp chunk target per shard size (YOUTH_ICP_TARGET_CHUNKS), one box.
out=$(mktemp)
trap 'rm -f "$out"' EXIT
for gp in ${PAIRS:-64 128}; do
  for tc in ${CHUNKS:-2048 2560 3072}; do
    YOUTH_ICP_TARGET_CHUNKS=$tc timeout -k 10 120 python3 bench.py --full --global-pairs $gp --steps 40 --warmup 5 --windows 1 --no-cpu-baseline --no-host-io --no-legs --no-viewer > "$out" 2>/dev/null || exit 1
    python3 -c "
import json,sys;d=json.load(open(sys.argv[1]))
print('pairs ${gp} chunks ${tc}: %.0f aligns/s (window %.0f)  k_icp %.1f us  sched %s' % (d['value'], d['window_rates'][0], d['roofline']['avg_launch_ms']*1e3, d['sched_last_step']))" "$out"
  done
done
