"""Shrunk layers one by one: every convolution shape of ResNet-50 (v2 bottleneck) and MobileNet-v1 1.0 at B = 256 / 224 x 224,
bf16, with 0.5 and 0.75 of the input channels kept (the export tool's own apply_fake_pruning): GPU time of

  dense   the dense inference kernel Conv2D dispatches the shape to, on the ZERO-FILLED full-shape kernel (what a user gets without
          a shrunk file); 1x1 layers whose dense twin reads an un-materialised BN output (graph.LazyAct) run WITH that prologue
  gather  pf_conv_gather_fwd on the shrunk kernel; for those 1x1 layers PLUS the pf_bn_act_quant_apply pass that materialises the
          input first (the gather kernel has no prologue), i.e. the pair the graph really launches

alternating inside one process, their ratio, and each one's share of its bound = max(FLOPs / 2.5 PFLOP/s bf16 MFMA peak,
bytes / 8 TB/s HBM peak), FLOPs and bytes computed here from the shapes (dense: all C channels, gather: the kept ones; input bytes
are the full tensor for both -- the gather kernel reads every cache line).

  python tools/gpu/gather_conv_layers.py > profiles/gather_conv_layers.txt
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from _timing import gpu_time_us
from pocketflow_amd import hip
from pocketflow_amd.flags import FLAGS
from pocketflow_amd.tools.conversion import export_chn_pruned_model as E

B = int(os.environ.get('B', 256))
MFMA_PEAK, HBM_PEAK = 2.5e15, 8.0e12
# (name, input H, C, N, k, stride, pad, lazy input (the dense 1x1 fuses the producer BN + ReLU), launches per network)
RESNET50 = [
    ('stem 7x7/2', 224, 3, 64, 7, 2, 3, 0, 1),
    ('s1 conv1 (pool out)', 56, 64, 64, 1, 1, 0, 1, 1), ('s1 conv1', 56, 256, 64, 1, 1, 0, 1, 2), ('s1 conv2 3x3', 56, 64, 64, 3, 1, 1, 0, 3),
    ('s1 conv3', 56, 64, 256, 1, 1, 0, 0, 3), ('s1 proj', 56, 64, 256, 1, 1, 0, 1, 1),
    ('s2 conv1 @56', 56, 256, 128, 1, 1, 0, 1, 1), ('s2 conv2 3x3/2', 56, 128, 128, 3, 2, 1, 0, 1), ('s2 conv1', 28, 512, 128, 1, 1, 0, 1, 3),
    ('s2 conv2 3x3', 28, 128, 128, 3, 1, 1, 0, 3), ('s2 conv3', 28, 128, 512, 1, 1, 0, 0, 4), ('s2 proj /2', 56, 256, 512, 1, 2, 0, 1, 1),
    ('s3 conv1 @28', 28, 512, 256, 1, 1, 0, 1, 1), ('s3 conv2 3x3/2', 28, 256, 256, 3, 2, 1, 0, 1), ('s3 conv1', 14, 1024, 256, 1, 1, 0, 1, 5),
    ('s3 conv2 3x3', 14, 256, 256, 3, 1, 1, 0, 5), ('s3 conv3', 14, 256, 1024, 1, 1, 0, 0, 6), ('s3 proj /2', 28, 512, 1024, 1, 2, 0, 1, 1),
    ('s4 conv1 @14', 14, 1024, 512, 1, 1, 0, 1, 1), ('s4 conv2 3x3/2', 14, 512, 512, 3, 2, 1, 0, 1), ('s4 conv1', 7, 2048, 512, 1, 1, 0, 1, 2),
    ('s4 conv2 3x3', 7, 512, 512, 3, 1, 1, 0, 2), ('s4 conv3', 7, 512, 2048, 1, 1, 0, 0, 3), ('s4 proj /2', 14, 1024, 2048, 1, 2, 0, 1, 1)]
MOBILENET = [('pw1', 112, 32, 64, 1, 1, 0, 1, 1), ('pw2', 56, 64, 128, 1, 1, 0, 1, 1), ('pw3', 56, 128, 128, 1, 1, 0, 1, 1),
             ('pw4', 28, 128, 256, 1, 1, 0, 1, 1), ('pw5', 28, 256, 256, 1, 1, 0, 1, 1), ('pw6', 14, 256, 512, 1, 1, 0, 1, 1),
             ('pw7-11', 14, 512, 512, 1, 1, 0, 1, 5), ('pw12', 7, 512, 1024, 1, 1, 0, 1, 1), ('pw13', 7, 1024, 1024, 1, 1, 0, 1, 1),
             ('logits', 1, 1024, 1001, 1, 1, 0, 0, 1)]
# (MobileNet's 3x3/2 stem over the 3-channel image has asymmetric 'SAME' pads: a shrunk stem keeps the padded image copy Conv2D makes,
#  and int(3 * ratio) prunes 1 of 3 channels at 0.5 and none at 0.25 -- left out of the table)


def dense_fn(x, wfull, y, H, C, N, k, stride, pad, Ho, ss):
  M = B * Ho * Ho
  if k == 7:
    return lambda: hip.conv_stem_fwd(x, wfull, y, B, H, H)
  if k == 1 and C % 8 == 0 and N % 8 == 0:
    geom = None if stride == 1 else (Ho, Ho, H, H, stride)
    w2 = wfull.reshape(N, C)
    return lambda: hip.conv1x1_fwd(x, w2, y, M, N, C, scale_shift=ss, act='Relu' if ss is not None else None, geom=geom)
  if k > 1 and C % 64 == 0:
    return lambda: hip.conv2d_fwd(x, wfull, y, B, H, H, C, N, k, k, stride, pad, pad, Ho, Ho)
  return lambda: hip.convg_fwd(x, wfull, None, y, B, H, H, C, N, k, k, stride, pad, pad, Ho, Ho)


def main():
  print('# B = %d, bf16; us per launch (best of 3 replays of 20 captured launches); bound = max(FLOPs / 2.5 PF, bytes / 8 TB/s)' % B)
  print('%-10s %-20s %-22s %5s %2s | %9s %9s %6s | %7s %7s' % ('net', 'layer', 'H,C,N,k,stride', 'keep', 'n', 'dense us', 'gather us',
                                                             'd / g', 'd bound', 'g bound'))
  for net, layers in (('resnet50', RESNET50), ('mobilenet', MOBILENET)):
    for keep in (0.5, 0.75):
      tot_d = tot_g = 0.0
      for name, H, C, N, k, stride, pad, lazy, cnt in layers:
        Ho = (H + 2 * pad - k) // stride + 1
        M = B * Ho * Ho
        g = torch.Generator(device='cuda').manual_seed(H + C + N + k)
        x = torch.randn((B, C, H, H), device='cuda', generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
        FLAGS.fake_prune_ratio = 1.0 - keep
        kern = E.apply_fake_pruning((np.random.RandomState(C + N).randn(k, k, C, N) * 0.05).astype(np.float32), np.random.RandomState(7))
        shrunk, nnz = E.shrink_kernel(kern)
        Ck = int(nnz.size)
        wfull = torch.from_numpy(np.ascontiguousarray(kern.transpose(3, 0, 1, 2))).cuda().bfloat16()
        wk = torch.from_numpy(np.ascontiguousarray(shrunk.transpose(3, 0, 1, 2))).cuda().bfloat16()
        gather = torch.from_numpy(hip.check_gather(nnz, C, Ck)).cuda()
        y = torch.empty((B, N, Ho, Ho), dtype=torch.bfloat16, device='cuda').contiguous(memory_format=torch.channels_last)
        ss = torch.stack([torch.rand(C, device='cuda') + 0.5, torch.randn(C, device='cuda')]).contiguous() if lazy else None
        xq = torch.empty_like(x)
        dense = dense_fn(x, wfull, y, H, C, N, k, stride, pad, Ho, ss)

        def gathered():
          xin = x
          if lazy:
            hip.bn_act_quant_apply(x, xq, B * H * H, C, ss, 'Relu', None, 8, False)
            xin = xq
          hip.conv_gather_fwd(xin, wk, gather, y, B, H, H, C, N, k, k, stride, pad, pad, Ho, Ho)
        td, tg = [], []
        for _ in range(2):                          # alternate the two variants
          td.append(gpu_time_us(dense))
          tg.append(gpu_time_us(gathered))
        td, tg = min(td), min(tg)
        nbytes = (B * H * H * C // (stride * stride if k == 1 else 1) + M * N) * 2
        bound_d = max(2.0 * M * N * k * k * C / MFMA_PEAK, (nbytes + N * k * k * C * 2) / HBM_PEAK) * 1e6
        bound_g = max(2.0 * M * N * k * k * Ck / MFMA_PEAK, (nbytes + N * k * k * Ck * 2) / HBM_PEAK) * 1e6
        print('%-10s %-20s %-22s %5.2f %2d | %9.1f %9.1f %6.2f | %7.2f %7.2f' % (
            net, name, '%d,%d,%d,%d,%d' % (H, C, N, k, stride), keep, cnt, td, tg, td / tg, bound_d / td, bound_g / tg))
        tot_d += cnt * td
        tot_g += cnt * tg
        del x, xq, y
      print('%-10s keep %.2f: convolutions of one forward pass  dense %.2f ms   gather %.2f ms   dense / gather %.2f'
            % (net, keep, tot_d / 1e3, tot_g / 1e3, tot_d / tot_g))


if __name__ == '__main__':
  main()
