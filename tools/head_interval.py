#!/usr/bin/env python
"""The network head of the training step as ONE interval of a rocprofv3 `--kernel-trace --output-format csv` trace.

The stretch between the student's last forward convolution and its first backward-data convolution is a chain of small dependent
launches with nothing beside it, so what matters is its wall time, not the sum of its kernels.  Per step the interval runs from the
START of the last k_bn_finalize before the step's first k_ce_distill* launch to the END of the first k_bn_bwd_apply* launch behind
it (both anchors exist with and without PF_HEAD_FUSE).  Reported: the interval and the number of launches inside it -- all of them,
and those on the anchor's queue (the teacher's forward for the next batch runs on another one) -- averaged over the K consecutive
steps with the smallest wall time (as tools/prof_summary.py picks its window), and the launches of one of those steps by name.

    python tools/head_interval.py <..._kernel_trace.csv> [--steps 4]
"""
import argparse
import csv
import re
from collections import Counter


def short(name):
  name = re.sub(r'^void ', '', name)
  return re.sub(r'\(.*$', '', name)[:110]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('trace')
  ap.add_argument('--steps', type=int, default=4)
  args = ap.parse_args()
  rows = []
  with open(args.trace, newline='') as f:
    for r in csv.DictReader(f):
      rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), short(r['Kernel_Name']), r.get('Queue_Id', '')))
  rows.sort()
  ce = [i for i, r in enumerate(rows) if r[2].startswith('k_ce_distill')]
  if not ce:
    raise SystemExit('no k_ce_distill launch in the trace')
  # the first loss launch of every step: launches closer than 2 ms belong to one step
  firsts = [i for n, i in enumerate(ce) if n == 0 or rows[i][0] - rows[ce[n - 1]][0] > 2e6]
  steps = []
  for i in firsts:
    a = next((j for j in range(i - 1, -1, -1) if rows[j][2].startswith('k_bn_finalize')), None)
    b = next((j for j in range(i + 1, len(rows)) if rows[j][2].startswith('k_bn_bwd_apply')), None)
    if a is None or b is None:
      continue
    t0, t1 = rows[a][0], rows[b][1]
    inside = [r for r in rows if r[0] >= t0 and r[1] <= t1]
    steps.append(dict(t0=t0, wall=t1 - t0, n=len(inside), n_queue=sum(1 for r in inside if r[3] == rows[a][3]), inside=inside,
                      busy=sum(r[1] - r[0] for r in inside if r[3] == rows[a][3])))
  K = min(args.steps, len(steps) - 1)
  if K < 1:
    raise SystemExit('fewer than two complete steps in the trace')
  best = min(range(K, len(steps)), key=lambda i: steps[i]['t0'] - steps[i - K]['t0'])
  win = steps[best - K:best]
  print('# %d steps in the trace; the %d consecutive ones with the smallest wall time (%.3f ms/step):' %
        (len(steps), K, (steps[best]['t0'] - steps[best - K]['t0']) / K / 1e6))
  for s in win:
    print('#   interval %8.1f us   launches %3d (%3d on the anchor\'s queue, busy %7.1f us)' % (s['wall'] / 1e3, s['n'], s['n_queue'], s['busy'] / 1e3))
  print('head interval: %.1f us/step, %.1f launches/step (%.1f on the anchor\'s queue, busy %.1f us)' % (
      sum(s['wall'] for s in win) / K / 1e3, sum(s['n'] for s in win) / K, sum(s['n_queue'] for s in win) / K,
      sum(s['busy'] for s in win) / K / 1e3))
  print('# launches of the last of these steps, in order (us):')
  for r in win[-1]['inside']:
    print('#   %9.1f +%7.1f  q%s  %s' % ((r[0] - win[-1]['t0']) / 1e3, (r[1] - r[0]) / 1e3, r[3], r[2]))
  cnt = Counter(r[2] for r in win[-1]['inside'])
  print('# by name:', ', '.join('%d x %s' % (c, n) for n, c in cnt.most_common()))


if __name__ == '__main__':
  main()
