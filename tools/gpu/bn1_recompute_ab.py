"""Per-layer A/B of "conv1 backward-data, then bn1 backward apply" in the identity bottleneck blocks of ResNet-50 at B = 256:
today's pair (conv1x1_bwd_data_bnstats -> bn_bwd_finalize -> bn_bwd_apply with the shortcut addend) against the pair that never
writes conv1's input gradient (conv1x1_bwd_data_bnsums -> bn_bwd_finalize -> conv1x1_bwd_data_bnapply).  HIP events, each variant
alone on the chip; the results are compared bit for bit once.  The step has two such blocks in stage 1 and three in stage 2."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from pocketflow_amd import hip


def timeit(fn, n=10):
  for _ in range(2): fn()
  torch.cuda.synchronize()
  a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
  a.record()
  for _ in range(n): fn()
  b.record(); torch.cuda.synchronize()
  return a.elapsed_time(b) / n * 1e3   # us


B = int(os.environ.get('B', 256))
shapes = [(56, 64, 256, 2), (28, 128, 512, 3)]        # (H = W, N, K, identity blocks per step)
print('%-14s | %-40s | %-40s | %-9s | bytes: today  new' % ('HW,N,K', 'today: bwd-data+sums  finalize  apply  sum', 'new:   sums-only  finalize  gemm+apply  sum', 'saved us'))
total = 0.0
for hw, N, K, blocks in shapes:
  M = B * hw * hw
  g = torch.Generator(device='cuda').manual_seed(hw + K + N)
  dY = (torch.randn(M, N, device='cuda', generator=g) * 0.1).bfloat16()
  Wt = (torch.randn(N, K, device='cuda', generator=g) * 0.1).bfloat16().t().contiguous()
  x = torch.randn(M, K, device='cuda', generator=g).bfloat16()
  addend = (torch.randn(M, K, device='cuda', generator=g) * 0.1).bfloat16()
  ss = torch.stack([torch.rand(K, device='cuda', generator=g) + 0.5, torch.randn(K, device='cuda', generator=g) * 0.3])
  mi = torch.stack([torch.randn(K, device='cuda', generator=g) * 0.1, torch.rand(K, device='cuda', generator=g) + 0.5])
  assert hip.conv1x1_bwd_apply_plan(M, N, K) != 0
  G = hip.conv1x1_stats_groups(M, K, N)
  p_a, p_b = torch.empty(G, 2, K, device='cuda'), torch.empty(G, 2, K, device='cuda')
  dg, db = torch.empty(K, device='cuda'), torch.empty(K, device='cuda')
  dQ = torch.empty(M, K, device='cuda', dtype=torch.bfloat16)
  dx_a, dx_b = torch.empty_like(dQ), torch.empty_like(dQ)
  a1 = lambda: hip.conv1x1_bwd_data_bnstats(dY, Wt, dQ, x, ss, mi, 'Relu', p_a, M, N, K)
  fin_a = lambda: hip.bn_bwd_finalize(p_a, G, K, dg, db)
  a2 = lambda: hip.bn_bwd_apply(dQ, x, dx_a, M, K, ss, mi, dg, db, 'Relu', addend=addend)
  b1 = lambda: hip.conv1x1_bwd_data_bnsums(dY, Wt, x, ss, mi, 'Relu', p_b, M, N, K)
  fin_b = lambda: hip.bn_bwd_finalize(p_b, G, K, dg, db)
  b2 = lambda: hip.conv1x1_bwd_data_bnapply(dY, Wt, x, ss, mi, 'Relu', dg, db, addend, dx_b, M, N, K)
  a1(); fin_a(); a2(); b1(); fin_b(); b2()
  torch.cuda.synchronize()
  same = torch.equal(p_a, p_b) and torch.equal(dx_a.view(torch.int16), dx_b.view(torch.int16))
  t = [timeit(f) for f in (a1, fin_a, a2, b1, fin_b, b2)]
  ta, tb = sum(t[:3]), sum(t[3:])
  u = M * K * 2
  bytes_a, bytes_b = 6.25 * u, 4.5 * u
  total += blocks * (ta - tb)
  print('%-14s | %9.0f %9.0f %9.0f %9.0f   | %9.0f %9.0f %9.0f %9.0f   | %7.0f   | %.2f GB %.2f GB | x%d per step | bit-equal %s' % (
      '%d,%d,%d' % (hw, N, K), t[0], t[1], t[2], ta, t[3], t[4], t[5], tb, ta - tb, bytes_a / 1e9, bytes_b / 1e9, blocks, same))
  print('%-14s | TB/s of the pair: today %.2f, new %.2f' % ('', bytes_a / ta / 1e6, bytes_b / tb / 1e6))
  del dY, x, addend, dQ, dx_a, dx_b
print('kernel time saved per step (five blocks): %.0f us' % total)
