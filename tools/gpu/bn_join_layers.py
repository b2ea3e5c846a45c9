"""The BN + shortcut + ReLU join of the ResNet-v1 blocks (pf_bn_join.hip) against the composition of existing kernels it replaces,
forward + backward pair, at the four stage shapes of ResNet-50 at batch 256 in bf16 (rows x C: 256 * 56^2 x 256, 256 * 28^2 x 512,
256 * 14^2 x 1024, 256 * 7^2 x 2048), with and without the 8-bit activation quantiser.

  fused      forward : pf_bn_add_act_fwd (+ the slot) [+ pf_uq_apply in place]
             backward: pf_bn_add_act_bwd_gate, pf_bn_bwd_finalize, pf_bn_bwd_apply(act none)
  composition forward : pf_bn_act_quant_apply(act none), aten add, then aten relu  [or pf_minmax_tensor + pf_uq_apply(Relu)]
             backward: pf_act_grad(Relu), pf_bn_bwd_stats(act none), pf_bn_bwd_finalize, pf_bn_bwd_apply(act none)

Bytes are counted from the shapes, E = rows * C * 2 bytes per pass over one tensor (the [.][C] tables and partial sums are < 1 %):
fused 3 E (+ 2 E quantiser) forward and 4 E + 3 E backward; composition 2 E + 3 E + 2 E (quantiser: + 1 E + 2 E instead of the relu's
2 E) forward and 3 E + 2 E + 3 E backward.  Each route's time is the device-event time of `iters` back-to-back pairs; the routes
alternate over `rounds` rounds and the table gives the median and the spread (max - min) over the rounds.  The fraction of peak is
bytes / time over 8 TB/s (HBM3E; the 51 MB tensors of the last stage fit the 256 MB last-level cache, so that row can exceed what
HBM alone would give).

Usage: python tools/gpu/bn_join_layers.py [--out FILE] [--batch 256] [--iters 20] [--rounds 7]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from pocketflow_amd import hip  # noqa: E402

PEAK = 8.0e12
STAGES = [(56, 256), (28, 512), (14, 1024), (7, 2048)]


def buffers(rows, C):
  gen = torch.Generator(device='cuda').manual_seed(rows + C)
  t = lambda: torch.randn(rows, C, generator=gen, device='cuda', dtype=torch.float32).to(torch.bfloat16)
  b = dict(x=t(), r=t(), dq=t())
  for k in ('u', 'g', 'dx', 'y', 'z', 'dz', 'q'):
    b[k] = torch.empty(rows, C, dtype=torch.bfloat16, device='cuda')
  b['ss'] = torch.stack([0.5 + 1.5 * torch.rand(C, generator=gen, device='cuda'),
                         2.0 * torch.rand(C, generator=gen, device='cuda') - 1.0]).float().contiguous()
  b['mi'] = torch.stack([0.3 * torch.randn(C, generator=gen, device='cuda'),
                         0.5 + torch.rand(C, generator=gen, device='cuda')]).float().contiguous()
  b['dgamma'], b['dbeta'] = torch.empty(C, device='cuda'), torch.empty(C, device='cuda')
  b['slot'] = torch.zeros(2, dtype=torch.int32, device='cuda')
  return b


def routes(b, rows, C, quant):
  nj = hip.bn_add_act_groups(rows, C)
  pj = torch.empty(nj * 2 * C, device='cuda')
  # the row splits graph._bn_blocks gives the separate statistics pass at these shapes
  cg = min(C // 8, 8)
  nb = int(max(1, min(256 // (C // (cg * 8)), rows // ((1024 // cg) * 2))))
  pb = torch.empty(nb * 2 * C, device='cuda')
  slot = b['slot']

  def fused():
    if quant:
      hip.minmax_slots_init(slot)
    hip.bn_add_act_fwd(b['x'], b['r'], b['u'], rows, C, b['ss'], 'Relu', slot if quant else None)
    if quant:
      hip.uq_apply(b['u'], b['u'], slot, 8, None)
    hip.bn_add_act_bwd_gate(b['dq'], b['x'], b['r'], b['g'], rows, C, b['ss'], b['mi'], 'Relu', pj)
    hip.bn_bwd_finalize(pj, nj, C, b['dgamma'], b['dbeta'])
    hip.bn_bwd_apply(b['g'], b['x'], b['dx'], rows, C, b['ss'], b['mi'], b['dgamma'], b['dbeta'], None)

  def composition():
    hip.bn_act_quant_apply(b['x'], b['y'], rows, C, b['ss'], None, None, 8, False)
    torch.add(b['y'], b['r'], out=b['z'])
    if quant:
      hip.minmax_slots_init(slot)
      hip.minmax_tensor(b['z'], slot, 'Relu')
      hip.uq_apply(b['z'], b['q'], slot, 8, 'Relu')
    else:
      torch.clamp_min(b['z'], 0, out=b['q'])         # aten's relu kernel with an output buffer
    hip.act_grad(b['dq'], b['z'], b['dz'], 'Relu')
    hip.bn_bwd_stats(b['dz'], b['x'], rows, C, b['ss'], b['mi'], None, pb, nb)
    hip.bn_bwd_finalize(pb, nb, C, b['dgamma'], b['dbeta'])
    hip.bn_bwd_apply(b['dz'], b['x'], b['dx'], rows, C, b['ss'], b['mi'], b['dgamma'], b['dbeta'], None)
  passes = {'fused': (3 + 2 * quant) + 7, 'composition': (2 + 3 + (3 if quant else 2)) + 8}
  return {'fused': fused, 'composition': composition}, passes


def time_ms(fn, iters):
  a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for _ in range(iters):
    fn()
  e.record()
  torch.cuda.synchronize()
  return a.elapsed_time(e) / iters


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=None)
  ap.add_argument('--batch', type=int, default=256)
  ap.add_argument('--iters', type=int, default=20)
  ap.add_argument('--rounds', type=int, default=7)
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'this measurement needs the GPU'
  lines = ['BN + shortcut + ReLU join, forward + backward pair, bf16, batch %d; %d rounds of %d pairs per route, routes alternating'
           % (args.batch, args.rounds, args.iters),
           'device: %s' % torch.cuda.get_device_name(0),
           '%-16s %-6s %-12s %9s %9s %9s %8s %9s' % ('rows x C', 'quant', 'route', 'median us', 'spread us', 'MB moved', 'TB/s', 'of 8 TB/s')]
  for hw, C in STAGES:
    rows = args.batch * hw * hw
    b = buffers(rows, C)
    for quant in (False, True):
      fns, passes = routes(b, rows, C, quant)
      for fn in fns.values():                      # warm-up: code objects, allocator
        fn()
        fn()
      torch.cuda.synchronize()
      t = {k: [] for k in fns}
      for _ in range(args.rounds):
        for k, fn in fns.items():
          t[k].append(time_ms(fn, args.iters) * 1e3)
      med = {k: statistics.median(v) for k, v in t.items()}
      for k in fns:
        nbytes = passes[k] * rows * C * 2
        rate = nbytes / (med[k] * 1e-6)
        lines.append('%-16s %-6s %-12s %9.1f %9.1f %9.1f %8.2f %8.1f%%' % (
            '%d x %d' % (rows, C), 'a8' if quant else '-', k, med[k], max(t[k]) - min(t[k]), nbytes / 1e6, rate / 1e12,
            100.0 * rate / PEAK))
      lines.append('%-16s %-6s fused / composition time: %.3f' % ('', '', med['fused'] / med['composition']))
    del b
    torch.cuda.empty_cache()
  text = '\n'.join(lines)
  print(text)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(text + '\n')


if __name__ == '__main__':
  main()
