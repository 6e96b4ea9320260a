#!/bin/bash
# Section timers and event counts of nw_forward_lds_v2 (poa_fwd2.hpp) per wave, config B
# (diagnostic builds: make prof prof1 profc1 profh1; LIBS=<dir> takes them from elsewhere).
# One JSON line per build.  prof / prof1: shader-clock cycles per window of wave 0 / wave 1 in
#   setup        record decode, next records and lists, substitution profile (sig)
#   pred1        single-predecessor rows: the predecessor row (registers or ring), diagonal / vertical
#   multi        the predecessor loop of rows with several predecessors and of marked rows
#   scan         in-lane prefix and wave scan
#   handover     consumer: wait for and read of the carry (block: head wait, load, merge, tail);
#                producer: post and flow control; column 0 and the HBM carries of later sweeps
#   codes        closure with the carry, codes, ring / spill / code stores
#   rest         sink row, register moves, loop
# (every lap ends in a wait for the clock read, which also waits for the LDS reads in flight: a
# section's share is an upper bound where it follows loads issued in an earlier one.)
# profh1: wave 1's hand-over section alone against its whole row loop (two clock reads per
# section instead of one per lap: the kernel runs 1.1-1.3 times slower instead of 2.7 times).
# profc1: counts per window on wave 1: rows with the predecessor r-1, with one ring predecessor,
# with several, marked rows, poll misses (s_sleep rounds) of the consumer and of the producer's
# flow control, rows in all.  (The count build of wave 0 trips a register-class error in the
# ROCm 7.2 compiler; rows by kind are the same on every wave.)
cd "$(dirname "$0")/.." || exit 1
O=gpurun_out/fwdprof_${TAG:-x}
LIBS=${LIBS:-claragenomicsanalysis_amd/lib}
mkdir -p $O
for L in ${BUILDS:-prof prof1 profh1 profc1}; do
  GWAMD_DIAG=1 GWAMD_LIBRARY=$LIBS/$L/libgwamd.so timeout -k 10 200 python -u bench.py --config B --steps 2 --warmup 1 --no-cpu > $O/$L.log 2>&1 || { tail -5 $O/$L.log; exit 1; }
  tail -1 $O/$L.log | python -c "
import json, sys
d = json.loads(sys.stdin.read()); p = d['config']['phase_ms_mean_per_window']
slots = ['backbone', 'add', 'topsort', 'output', 'forward', 'traceback', 'rowprog', 'total']
names = [None, None, None, None, 'handover', None, None, 'row_loop'] if '$L'.startswith('profh') else ['rows_d1', 'rows_ring1', 'rows_multi', 'rows_marked', 'poll_miss', 'flow_miss', None, 'rows'] if '$L'.startswith('profc') \
    else ['setup', 'pred1', 'multi', 'scan', 'handover', 'codes', 'rest', None]
v = {n: round(p[s] * 1e5) for n, s in zip(names, slots) if n}
out = {'build': '$L', 'tag': '${TAG:-x}', 'kernel_ms': d['roofline']['kernel_ms']}
if '$L'.startswith('profh'):
    out['share'] = {'handover': round(v['handover'] / v['row_loop'], 4)}
elif not '$L'.startswith('profc'):
    tot = sum(v.values()); out['cycles_per_window'] = tot
    out['share'] = {n: round(x / tot, 4) for n, x in v.items()}
out['per_window'] = v
print(json.dumps(out))" | tee -a $O/fwdprof.jsonl
done
