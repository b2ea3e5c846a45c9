"""Int8 layers one by one: every eligible convolution shape of ResNet-50 (v2 bottleneck) and every pointwise convolution of
MobileNet-v1 1.0 at B = 256 / 224 x 224, bf16 output, 8-bit activations and weights: GPU time of the launches the graph makes for
the layer on each route of inference.load_int8,

  float  pf_bn_act_quant_apply (the producer BN's normalise / ReLU / fake-quant pass, bf16 -> bf16) + the bf16 kernel Conv2D
         dispatches the shape to (pf_conv1x1_fwd / pf_conv2d_fwd), on the decoded kernel: int8 = 'off'
  int8   pf_bn_act_quant_codes (bf16 -> uint8 codes) + pf_conv_i8_fwd on the packed kernel: int8 = 'on'

alternating inside one process, and their ratio.  A producer pass that feeds two convolutions (bn1 of a projection block) is counted
with each of them on both routes.  Bounds: max(FLOPs / peak, bytes / 8 TB/s) with the bf16 MFMA peak 2.5 PFLOP/s for the float
route and twice that for int8; bytes = pre-BN input read + intermediate written and read + output written + kernel.

  python tools/gpu/int8_conv_layers.py > profiles/int8_conv_layers.txt

STATIC=1 prints the static column instead -- the layer on a graph with FIXED activation ranges, where the BatchNorm + activation +
quantiser BEHIND the layer has a known range:

  float  the bf16 kernel on the fake-quantised bf16 input + pf_bn_act_quant_static over its output (bf16 -> the consumer's uint8 codes)
  int8   pf_conv_i8_fwd_q: codes in, the consumer's codes out, one launch

in ROUNDS alternating rounds; `pays` marks the rows where the int8 route is faster by more than the larger spread (max - min over the
rounds): what graph.int8_pays_static has to return.  (A layer whose output joins a residual has no such consumer; it is timed as if
it had, for the kernel's sake.)

  STATIC=1 python tools/gpu/int8_conv_layers.py >> profiles/int8_conv_layers.txt
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
from _int8_layers import conv_layer, nhwc, time_rounds
from pocketflow_amd import hip
from gather_conv_layers import MOBILENET, RESNET50

B = int(os.environ.get('B', 256))
MFMA_PEAK, HBM_PEAK = 2.5e15, 8.0e12
NETS = (('resnet50', RESNET50), ('mobilenet', MOBILENET))


def eligible(net, layers):
  """(label of the row, H, C, N, k, stride, pad, count) of the layers the i8 kernel takes; the others are printed as such."""
  for name, H, C, N, k, stride, pad, _lazy, cnt in layers:
    label = '%-10s %-20s %-22s %2d' % (net, name, '%d,%d,%d,%d,%d' % (H, C, N, k, stride), cnt)
    if not hip.conv_i8_supported(C, N, k, k, stride) or (k > 1 and C % 64):
      print(label + ' | not eligible')
      continue
    yield label, H, C, N, k, stride, pad, cnt


def float_conv(xq, wfull, y, H, C, N, k, stride, pad, Ho):
  """The launch of the bf16 kernel Conv2D dispatches the shape to."""
  if k == 1:
    geom = None if stride == 1 else (Ho, Ho, H, H, stride)
    w2 = wfull.reshape(N, C)
    return lambda: hip.conv1x1_fwd(xq, w2, y, B * Ho * Ho, N, C, geom=geom)
  return lambda: hip.conv2d_fwd(xq, wfull, y, B, H, H, C, N, k, k, stride, pad, pad, Ho, Ho)


def main_static():
  rounds = int(os.environ.get('ROUNDS', 3))
  print('# STATIC ranges: B = %d, bf16 activations, 8-bit codes; us per layer (best of %d alternating rounds, each the best of 3 replays of '
        '20 captured launches); spread = max - min over the rounds' % (B, rounds))
  print('%-10s %-20s %-22s %2s | %9s %9s %9s | %9s | %7s | %8s %8s | %4s' % (
      'net', 'layer', 'H,C,N,k,stride', 'n', 'bf16 us', 'static us', 'float us', 'i8_q us', 'f / i8', 'f spread', 'i spread', 'pays'))
  for net, layers in NETS:
    tot_f = tot_i = 0.0
    for label, H, C, N, k, stride, pad, cnt in eligible(net, layers):
      Ho = (H + 2 * pad - k) // stride + 1
      M = B * Ho * Ho
      g = torch.Generator(device='cuda').manual_seed(H + C + N + k)
      xq = torch.rand((B, C, H, H), device='cuda', generator=g).mul_(4.0).bfloat16().contiguous(memory_format=torch.channels_last)
      codes = torch.randint(0, 256, (B, C, H, H), dtype=torch.uint8, device='cuda').contiguous(memory_format=torch.channels_last)
      ab = torch.tensor([4.0, 0.0], device='cuda')
      oab = torch.tensor([3.0, 0.0], device='cuda')
      ss = torch.stack([torch.rand(N, device='cuda') * 0.1 + 0.05, torch.randn(N, device='cuda')]).contiguous()
      wfull, (pw, psb, pts, ptp) = conv_layer(k, C, N)
      y, out = nhwc((B, N, Ho, Ho), torch.bfloat16), nhwc((B, N, Ho, Ho), torch.uint8)
      conv_f = float_conv(xq, wfull, y, H, C, N, k, stride, pad, Ho)
      static_f = lambda: hip.bn_act_quant_static(y, out, M, N, ss, 'Relu', oab, 8)
      conv_q = lambda: hip.conv_i8_fwd_q(codes, pw, ab, 8, psb, pts, ptp, ss, 'Relu', oab, 8, out, B, H, H, C, N, k, k, stride, pad, pad,
                                         Ho, Ho)

      def route_f():
        conv_f()
        static_f()
      t, spread = time_rounds((('bf16', conv_f), ('static', static_f), ('float', route_f), ('int8', conv_q)), rounds)
      pays = t['float'] - t['int8'] > max(spread['float'], spread['int8'])
      print('%s | %9.1f %9.1f %9.1f | %9.1f | %7.2f | %8.1f %8.1f | %4s' % (
          label, t['bf16'], t['static'], t['float'], t['int8'], t['float'] / t['int8'], spread['float'], spread['int8'],
          'yes' if pays else 'no'))
      tot_f += cnt * t['float']
      tot_i += cnt * t['int8']
      del xq, y, codes, out
    print('%-10s eligible convolutions of one forward pass with the quantiser behind them, static ranges  float %.2f ms   int8 %.2f ms   '
          'float / int8 %.2f' % (net, tot_f / 1e3, tot_i / 1e3, tot_f / max(tot_i, 1e-9)))


def main():
  print('# B = %d, bf16 activations, 8-bit codes; us per layer (best of 2 alternating rounds, each the best of 3 replays of 20 captured '
        'launches); bound = max(FLOPs / peak, bytes / 8 TB/s)' % B)
  print('%-10s %-20s %-22s %2s | %9s %9s %9s | %9s %9s %9s | %7s | %7s %7s' % (
      'net', 'layer', 'H,C,N,k,stride', 'n', 'apply us', 'bf16 us', 'float us', 'codes us', 'i8 us', 'int8 us', 'f / i8', 'f bound', 'i bound'))
  for net, layers in NETS:
    tot_f = tot_i = 0.0
    for label, H, C, N, k, stride, pad, cnt in eligible(net, layers):
      Ho = (H + 2 * pad - k) // stride + 1
      M = B * Ho * Ho
      rows = B * H * H
      g = torch.Generator(device='cuda').manual_seed(H + C + N + k)
      x = torch.randn((B, C, H, H), device='cuda', generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
      ss = torch.stack([torch.rand(C, device='cuda') + 0.5, torch.randn(C, device='cuda')]).contiguous()
      xq = torch.empty_like(x)
      codes = nhwc(x.shape, torch.uint8)
      ab = torch.empty(2, device='cuda')
      slot = torch.empty((1, 2), dtype=torch.int32, device='cuda')
      hip.minmax_slots_init(slot)
      hip.bn_act_quant_apply(x, xq, rows, C, ss, 'Relu', None, 8, False)
      hip.minmax_tensor(xq, slot[0])
      wfull, (pw, psb, pts, ptp) = conv_layer(k, C, N)
      y = nhwc((B, N, Ho, Ho), torch.bfloat16)
      conv_f = float_conv(xq, wfull, y, H, C, N, k, stride, pad, Ho)
      apply_f = lambda: hip.bn_act_quant_apply(x, xq, rows, C, ss, 'Relu', slot[0], 8, True)
      codes_f = lambda: hip.bn_act_quant_codes(x, codes, rows, C, ss, 'Relu', slot[0], 8, ab)
      conv_i = lambda: hip.conv_i8_fwd(codes, pw, ab, 8, psb, pts, ptp, y, B, H, H, C, N, k, k, stride, pad, pad, Ho, Ho)

      def route_f():
        apply_f()
        conv_f()

      def route_i():
        codes_f()
        conv_i()
      t, _ = time_rounds((('apply', apply_f), ('bf16', conv_f), ('float', route_f), ('codes', codes_f), ('i8', conv_i), ('int8', route_i)), 2)
      flops = 2.0 * M * N * k * k * C
      read = rows * C // (stride * stride if k == 1 else 1)
      bytes_f = rows * C * 4 + read * 2 + M * N * 2 + N * k * k * C * 2
      bytes_i = rows * C * 3 + read + M * N * 2 + N * k * k * C
      bound_f = max(flops / MFMA_PEAK, bytes_f / HBM_PEAK) * 1e6
      bound_i = max(flops / (2 * MFMA_PEAK), bytes_i / HBM_PEAK) * 1e6
      print('%s | %9.1f %9.1f %9.1f | %9.1f %9.1f %9.1f | %7.2f | %7.2f %7.2f' % (
          label, t['apply'], t['bf16'], t['float'], t['codes'], t['i8'], t['int8'], t['float'] / t['int8'], bound_f / t['float'],
          bound_i / t['int8']))
      tot_f += cnt * t['float']
      tot_i += cnt * t['int8']
      del x, xq, y, codes
    print('%-10s eligible convolutions of one forward pass (with their producer passes)  float %.2f ms   int8 %.2f ms   float / int8 %.2f'
          % (net, tot_f / 1e3, tot_i / 1e3, tot_f / max(tot_i, 1e-9)))


if __name__ == '__main__':
  main_static() if os.environ.get('STATIC', '0') == '1' else main()
