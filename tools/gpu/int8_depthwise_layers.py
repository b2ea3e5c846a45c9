"""Int8 depthwise layers one by one: the 13 depthwise 3x3 shapes of MobileNet-v1 1.0 at B = 256 / 224 x 224, bf16, 8-bit activations
and weights: GPU time of the launches the graph makes for the layer on each route of inference.load_int8(depthwise=...),

  float  pf_bn_act_quant_apply (the producer BN's normalise / ReLU6 / fake-quant pass, bf16 -> bf16) + pf_depthwise_fwd on the decoded
         kernel (with the statistics rows the graph asks it for): depthwise = 'off'
  int8   pf_bn_act_quant_codes (bf16 -> uint8 codes) + pf_dw_i8_fwd on the packed kernel: depthwise = 'on'

in ROUNDS alternating rounds inside one process: the best round of each launch and route, the spread (max - min over the rounds) of
the two routes, and their ratio.  `pays` marks the rows where the int8 route is faster by more than the larger spread: what
graph.int8_dw_pays has to return.  Bounds: bytes / 8 TB/s, bytes = pre-BN input read + intermediate written and read + output
written (float: 2 + 2 + 2 and 2 per output; int8: 2 + 1 + 1 and 2 per output).

  python tools/gpu/int8_depthwise_layers.py > profiles/int8_depthwise_layers.txt

STATIC=1 prints the static column instead -- the layer on a graph with FIXED activation ranges, where the BatchNorm + ReLU6 + quantiser
BEHIND the layer has a known range:

  float  pf_depthwise_fwd on the fake-quantised bf16 input (with the statistics rows the graph asks it for) + pf_bn_act_quant_static
         over its output (bf16 -> the consumer's uint8 codes)
  int8   pf_dw_i8_fwd_q: codes in, the consumer's codes out, one launch

`pays` as above: what graph.int8_dw_pays_static has to return.  Bounds: float 2 + 2, 2 + 1 bytes per input / output element; int8 1 + 1.

  STATIC=1 python tools/gpu/int8_depthwise_layers.py >> profiles/int8_depthwise_layers.txt
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
from _int8_layers import depthwise_layer, nhwc, time_rounds
from pocketflow_amd import hip, int8

B = int(os.environ.get('B', 256))
ROUNDS = int(os.environ.get('ROUNDS', 3))
HBM_PEAK = 8.0e12
# (name, input H = W, C, stride, count) of utils/external/mobilenet_v1.py's conv defs at 224 x 224
LAYERS = [('dw1', 112, 32, 1, 1), ('dw2 /2', 112, 64, 2, 1), ('dw3', 56, 128, 1, 1), ('dw4 /2', 56, 128, 2, 1), ('dw5', 28, 256, 1, 1),
          ('dw6 /2', 28, 256, 2, 1), ('dw7-11', 14, 512, 1, 5), ('dw12 /2', 14, 512, 2, 1), ('dw13', 7, 1024, 1, 1)]


def main_static():
  print('# STATIC ranges: B = %d, bf16 activations, 8-bit codes; us per layer (best of %d alternating rounds, each the best of 3 replays of '
        '20 captured launches); spread = max - min over the rounds; bound = bytes / 8 TB/s' % (B, ROUNDS))
  print('%-10s %-10s %-14s %2s | %9s %9s %9s | %9s | %7s | %7s %7s | %8s %8s | %4s' % (
      'net', 'layer', 'H,C,stride', 'n', 'dw us', 'static us', 'float us', 'dw_q us', 'f / i8', 'f bound', 'i bound', 'f spread', 'i spread',
      'pays'))
  tot_f = tot_i = 0.0
  for name, H, C, stride, cnt in LAYERS:
    Ho = -(-H // stride)
    pad = int8.same_pads(H, 3, stride)[0]
    rows, M = B * H * H, B * Ho * Ho
    g = torch.Generator(device='cuda').manual_seed(H + C + stride)
    xq = torch.rand((B, C, H, H), device='cuda', generator=g).mul_(6.0).bfloat16().contiguous(memory_format=torch.channels_last)
    codes = torch.randint(0, 256, (B, C, H, H), dtype=torch.uint8, device='cuda').contiguous(memory_format=torch.channels_last)
    ab = torch.tensor([6.0, 0.0], device='cuda')
    oab = torch.tensor([4.5, 0.0], device='cuda')                  # narrower than ReLU6's image: the clamp acts
    ss = torch.stack([torch.rand(C, device='cuda') * 0.2 + 0.1, torch.randn(C, device='cuda')]).contiguous()
    wcrs, wcol, wsb = depthwise_layer(C, stride)
    y, out = nhwc((B, C, Ho, Ho), torch.bfloat16), nhwc((B, C, Ho, Ho), torch.uint8)
    partial = torch.empty((hip.depthwise_groups(B, Ho, Ho, C), 4, C), dtype=torch.float32, device='cuda')
    dw_f = lambda: hip.depthwise_fwd(xq, wcrs, y, B, H, H, C, 3, stride, pad, pad, Ho, Ho, partial=partial)
    static_f = lambda: hip.bn_act_quant_static(y, out, M, C, ss, 'Relu6', oab, 8)
    dw_q = lambda: hip.dw_i8_fwd_q(codes, wcol, wsb, ab, 8, ss, 'Relu6', oab, 8, out, B, H, H, C, stride, pad, pad, Ho, Ho)

    def route_f():
      dw_f()
      static_f()
    t, spread = time_rounds((('dw', dw_f), ('static', static_f), ('float', route_f), ('int8', dw_q)), ROUNDS)
    spread_f, spread_i = spread['float'], spread['int8']
    bound_f = (rows * C * 2 + M * C * 5) / HBM_PEAK * 1e6
    bound_i = (rows * C + M * C) / HBM_PEAK * 1e6
    pays = t['float'] - t['int8'] > max(spread_f, spread_i)
    print('%-10s %-10s %-14s %2d | %9.1f %9.1f %9.1f | %9.1f | %7.2f | %7.2f %7.2f | %8.1f %8.1f | %4s' % (
        'mobilenet', name, '%d,%d,%d' % (H, C, stride), cnt, t['dw'], t['static'], t['float'], t['int8'], t['float'] / t['int8'],
        bound_f / t['float'], bound_i / t['int8'], spread_f, spread_i, 'yes' if pays else 'no'))
    tot_f += cnt * t['float']
    tot_i += cnt * t['int8']
    del xq, y, codes, out
  print('mobilenet  depthwise layers of one forward pass with the quantiser behind them, static ranges  float %.2f ms   int8 %.2f ms   '
        'float / int8 %.2f' % (tot_f / 1e3, tot_i / 1e3, tot_f / max(tot_i, 1e-9)))


def main():
  print('# B = %d, bf16 activations, 8-bit codes; us per layer (best of %d alternating rounds, each the best of 3 replays of 20 captured '
        'launches); spread = max - min over the rounds; bound = bytes / 8 TB/s' % (B, ROUNDS))
  print('%-10s %-10s %-14s %2s | %9s %9s %9s | %9s %9s %9s | %7s | %7s %7s | %8s %8s | %4s' % (
      'net', 'layer', 'H,C,stride', 'n', 'apply us', 'dw us', 'float us', 'codes us', 'i8 us', 'int8 us', 'f / i8', 'f bound', 'i bound',
      'f spread', 'i spread', 'pays'))
  tot_f = tot_i = 0.0
  for name, H, C, stride, cnt in LAYERS:
    Ho = -(-H // stride)
    pad = int8.same_pads(H, 3, stride)[0]
    rows, M = B * H * H, B * Ho * Ho
    g = torch.Generator(device='cuda').manual_seed(H + C + stride)
    x = torch.randn((B, C, H, H), device='cuda', generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    ss = torch.stack([torch.rand(C, device='cuda') + 0.5, torch.randn(C, device='cuda')]).contiguous()
    xq = torch.empty_like(x)
    codes = nhwc(x.shape, torch.uint8)
    ab = torch.empty(2, device='cuda')
    slot = torch.empty((1, 2), dtype=torch.int32, device='cuda')
    hip.minmax_slots_init(slot)
    hip.bn_act_quant_apply(x, xq, rows, C, ss, 'Relu6', None, 8, False)
    hip.minmax_tensor(xq, slot[0])
    wcrs, wcol, wsb = depthwise_layer(C, stride)
    y = nhwc((B, C, Ho, Ho), torch.bfloat16)
    partial = torch.empty((hip.depthwise_groups(B, Ho, Ho, C), 4, C), dtype=torch.float32, device='cuda')
    apply_f = lambda: hip.bn_act_quant_apply(x, xq, rows, C, ss, 'Relu6', slot[0], 8, True)
    dw_f = lambda: hip.depthwise_fwd(xq, wcrs, y, B, H, H, C, 3, stride, pad, pad, Ho, Ho, partial=partial)
    codes_f = lambda: hip.bn_act_quant_codes(x, codes, rows, C, ss, 'Relu6', slot[0], 8, ab)
    dw_i = lambda: hip.dw_i8_fwd(codes, wcol, wsb, ab, 8, y, B, H, H, C, stride, pad, pad, Ho, Ho)

    def route_f():
      apply_f()
      dw_f()

    def route_i():
      codes_f()
      dw_i()
    t, spread = time_rounds((('apply', apply_f), ('dw', dw_f), ('float', route_f), ('codes', codes_f), ('i8', dw_i), ('int8', route_i)), ROUNDS)
    spread_f, spread_i = spread['float'], spread['int8']
    bound_f = (rows * C * 6 + M * C * 2) / HBM_PEAK * 1e6
    bound_i = (rows * C * 4 + M * C * 2) / HBM_PEAK * 1e6
    pays = t['float'] - t['int8'] > max(spread_f, spread_i)
    print('%-10s %-10s %-14s %2d | %9.1f %9.1f %9.1f | %9.1f %9.1f %9.1f | %7.2f | %7.2f %7.2f | %8.1f %8.1f | %4s' % (
        'mobilenet', name, '%d,%d,%d' % (H, C, stride), cnt, t['apply'], t['dw'], t['float'], t['codes'], t['i8'], t['int8'],
        t['float'] / t['int8'], bound_f / t['float'], bound_i / t['int8'], spread_f, spread_i, 'yes' if pays else 'no'))
    tot_f += cnt * t['float']
    tot_i += cnt * t['int8']
    del x, xq, y, codes
  print('mobilenet  depthwise layers of one forward pass (with their producer passes)  float %.2f ms   int8 %.2f ms   float / int8 %.2f'
        % (tot_f / 1e3, tot_i / 1e3, tot_f / max(tot_i, 1e-9)))


if __name__ == '__main__':
  main_static() if os.environ.get('STATIC', '0') == '1' else main()
