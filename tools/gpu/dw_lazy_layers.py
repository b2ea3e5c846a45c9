"""The lazy depthwise route layer by layer: the ten distinct depthwise 3x3 shapes of MobileNet-v2 1.0 at B = 256 / 224 x 224, bf16, with
and without an 8-bit quantiser behind the producer's ReLU6, forward and backward-filter separately.  GPU time of the launches the graph
makes for the layer on each side of graph.dw_lazy_on,

  pair   pf_bn_act_quant_apply (the producer BN's normalise / ReLU6 / fake-quant pass, bf16 -> bf16) + the parent kernel on its output:
         pf_depthwise_fwd (with the statistics rows the graph asks it for) / pf_depthwise_wrw
  fused  pf_depthwise_fwd_act / pf_depthwise_wrw_act on the raw tensor: one launch

in ROUNDS alternating rounds inside one process and one build: the MEDIAN round of each launch and the spread (max - min over the
rounds).  `wins`: the fused median beats the pair's by more than the larger spread.  A training step runs the apply pass ONCE for both
directions, so the verdict for a layer is taken on the step's launches: apply + fwd + wrw against fwd_act + wrw_act (`pays`, with the
spreads of the two sums) -- what graph.dw_lazy_pays(C, stride, quantised, bfloat16) has to return.  Bounds: bytes / 8 TB/s; forward
pair 2 + 2 + 2 bytes per input element and 2 per output, fused 2 and 2; backward-filter pair 2 + 2 + 2 and 2 per gradient element,
fused 2 and 2.

  python tools/gpu/dw_lazy_layers.py > profiles/dw_lazy_layers.txt
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
from _timing import gpu_time_us
from pocketflow_amd import hip

B = int(os.environ.get('B', 256))
ROUNDS = int(os.environ.get('ROUNDS', 3))
HBM_PEAK = 8.0e12
# (blocks, input H = W, C, stride, count) of utils/external/mobilenet_v2.py's op list at 224 x 224, multiplier 1.0
LAYERS = [('b0', 112, 32, 1, 1), ('b1 /2', 112, 96, 2, 1), ('b2', 56, 144, 1, 1), ('b3 /2', 56, 144, 2, 1), ('b4-5', 28, 192, 1, 2),
          ('b6 /2', 28, 192, 2, 1), ('b7-9', 14, 384, 1, 3), ('b10-12', 14, 576, 1, 3), ('b13 /2', 14, 576, 2, 1), ('b14-16', 7, 960, 1, 3)]


def same_front_pad(size, k, stride):
  out = -(-size // stride)
  return max((out - 1) * stride + k - size, 0) // 2


def time_rounds(fns, rounds):
  """fns: (key, launch) pairs timed one after the other in each round (the routes alternate).  ({key: median us}, {key: max - min})."""
  t = {key: [] for key, _ in fns}
  for _ in range(rounds):
    for key, fn in fns:
      t[key].append(gpu_time_us(fn))
  return {k: statistics.median(v) for k, v in t.items()}, {k: max(v) - min(v) for k, v in t.items()}


def main():
  assert torch.cuda.is_available(), 'dw_lazy_layers.py measures on the GPU'
  print('# B = %d, bf16, act ReLU6; us per launch: median of %d alternating rounds, each the best of 3 replays of 20 captured launches; '
        'spread = max - min over the rounds; bound = bytes / 8 TB/s over the median' % (B, ROUNDS))
  hdr = '%-7s %-11s %2s %-5s %-3s | %8s %8s %8s %8s | %6s | %6s %6s | %7s %7s | %4s'
  print(hdr % ('blocks', 'H,C,stride', 'n', 'quant', 'dir', 'apply', 'parent', 'pair', 'fused', 'p / f', 'p bnd', 'f bnd', 'p sprd', 'f sprd', 'wins'))
  verdicts = []
  tot = {}
  for name, H, C, stride, cnt in LAYERS:
    Ho = -(-H // stride)
    pad = same_front_pad(H, 3, stride)
    rows, M = B * H * H, B * Ho * Ho
    g = torch.Generator(device='cuda').manual_seed(H + C + stride)
    x = torch.randn((B, C, H, H), device='cuda', generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    dy = torch.randn((B, C, Ho, Ho), device='cuda', generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    w = (torch.randn((C, 3, 3), device='cuda', generator=g) * 0.3).bfloat16()
    ss = torch.stack([torch.rand(C, device='cuda', generator=g) + 0.5, torch.randn(C, device='cuda', generator=g)]).contiguous()
    q = torch.empty_like(x)
    slot = torch.empty((1, 2), dtype=torch.int32, device='cuda')
    hip.minmax_slots_init(slot)
    hip.bn_act_quant_apply(x, q, rows, C, ss, 'Relu6', None, 8, False)
    hip.minmax_tensor(q, slot[0])
    y = torch.empty((B, C, Ho, Ho), dtype=torch.bfloat16, device='cuda').contiguous(memory_format=torch.channels_last)
    G = hip.depthwise_groups(B, Ho, Ho, C)
    partial = torch.empty((G, 4, C), dtype=torch.float32, device='cuda')
    slabs = torch.empty((G + 32) * C * 9, dtype=torch.float32, device='cuda')
    dw = torch.empty((C, 3, 3), dtype=torch.float32, device='cuda')
    dims = (B, H, H, C, 3, stride, pad, pad, Ho, Ho)
    for quant in (False, True):
      sl = slot[0] if quant else None
      apply_f = lambda: hip.bn_act_quant_apply(x, q, rows, C, ss, 'Relu6', sl, 8, quant)
      fwd = lambda: hip.depthwise_fwd(q, w, y, *dims, partial=partial)
      fwd_act = lambda: hip.depthwise_fwd_act(x, ss, 'Relu6', sl, 8, w, y, *dims, partial=partial)
      wrw = lambda: hip.depthwise_wrw(dy, q, dw, slabs, *dims)
      wrw_act = lambda: hip.depthwise_wrw_act(dy, x, ss, 'Relu6', sl, 8, dw, slabs, *dims)

      def pair_fwd():
        apply_f()
        fwd()

      def pair_wrw():
        apply_f()
        wrw()

      def step_off():
        apply_f()
        fwd()
        wrw()

      def step_on():
        fwd_act()
        wrw_act()
      t, sp = time_rounds((('apply', apply_f), ('fwd', fwd), ('pair_fwd', pair_fwd), ('fwd_act', fwd_act), ('wrw', wrw),
                           ('pair_wrw', pair_wrw), ('wrw_act', wrw_act), ('step_off', step_off), ('step_on', step_on)), ROUNDS)
      bytes_pair = {'fwd': rows * C * 6 + M * C * 2, 'wrw': rows * C * 6 + M * C * 2}
      bytes_fused = {'fwd': rows * C * 2 + M * C * 2, 'wrw': rows * C * 2 + M * C * 2}
      for d, parent, pair, fused in (('fwd', 'fwd', 'pair_fwd', 'fwd_act'), ('wrw', 'wrw', 'pair_wrw', 'wrw_act')):
        wins = t[pair] - t[fused] > max(sp[pair], sp[fused])
        print('%-7s %-11s %2d %-5s %-3s | %8.1f %8.1f %8.1f %8.1f | %6.2f | %6.2f %6.2f | %7.1f %7.1f | %4s' % (
            name, '%d,%d,%d' % (H, C, stride), cnt, 'a8' if quant else '-', d, t['apply'], t[parent], t[pair], t[fused], t[pair] / t[fused],
            bytes_pair[d] / HBM_PEAK * 1e6 / t[pair], bytes_fused[d] / HBM_PEAK * 1e6 / t[fused], sp[pair], sp[fused], 'yes' if wins else 'no'))
      pays = t['step_off'] - t['step_on'] > max(sp['step_off'], sp['step_on'])
      verdicts.append((name, H, C, stride, cnt, quant, t['step_off'], t['step_on'], sp['step_off'], sp['step_on'], pays))
      key = 'a8' if quant else '-'
      a = tot.setdefault(key, [0.0, 0.0])
      a[0] += cnt * t['step_off']
      a[1] += cnt * t['step_on']
    del x, q, y, dy
  print()
  print('# one training step of the layer: apply + fwd + wrw (off) against fwd_act + wrw_act (on); pays = on wins by more than the larger spread')
  print('%-7s %-11s %2s %-5s | %9s %9s | %6s | %8s %8s | %4s' % ('blocks', 'H,C,stride', 'n', 'quant', 'off us', 'on us', 'off/on', 'off sprd', 'on sprd', 'pays'))
  for name, H, C, stride, cnt, quant, off, on, s0, s1, pays in verdicts:
    print('%-7s %-11s %2d %-5s | %9.1f %9.1f | %6.2f | %8.1f %8.1f | %4s' % (name, '%d,%d,%d' % (H, C, stride), cnt, 'a8' if quant else '-',
                                                                        off, on, off / on, s0, s1, 'yes' if pays else 'no'))
  for key, (off, on) in tot.items():
    print('# all 17 depthwise layers of one step, quant %s: off %.3f ms, on %.3f ms, off / on %.2f' % (key, off / 1e3, on / 1e3, off / max(on, 1e-9)))
  print('# dw_lazy_pays rows (C, stride, quantised): %s' % sorted((C, stride, quant) for _, _, C, stride, _, quant, _, _, _, _, pays in verdicts if pays))


if __name__ == '__main__':
  main()
