"""The static (fixed-range, clamping) activation quantiser on the device: pf_bn_act_quant_static against the per-batch kernels and the
NumPy oracle (int8.static_codes / static_value), and the requantising epilogues pf_conv_i8_fwd_q / pf_dw_i8_fwd_q against their
definition -- the stand-alone pass applied to the float32 output of the parent kernel, bit for bit, for every output kind.

Shapes, operands and the slot-calibrated case are those of tests/test_conv_i8_gpu.py and tests/test_dw_i8_gpu.py."""
from ctypes import c_int, c_int64, c_void_p

import numpy as np
import pytest
import torch

from pocketflow_amd import int8
from pocketflow_amd.tools.conversion import export_quant_int8_model as ex

pytestmark = pytest.mark.gpu

B, H, W = 2, 13, 11
GEOMS = [(1, 1, 0), (1, 2, 0), (3, 1, 1), (3, 2, 1)]          # (R = S, stride, pad)
DW_CASES = [(h, w, C) for (h, w) in ((1, 1), (5, 7), (8, 6), (9, 4)) for C in (16, 48)] + [(28, 28, 64), (9, 4, 4080)]
KINDS = [torch.uint8, torch.float32, torch.bfloat16]


@pytest.fixture(scope='module')
def hip():
  from pocketflow_amd import hip as h
  assert torch.cuda.is_available(), 'gpu tests need a GPU'
  return h


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
  return c_void_p(0 if t is None else t.data_ptr())


def _bn_case(hip, C, act, dtype, seed):
  """tests/test_conv_i8_gpu.py::_bn_case: x [286][C], scale / shift, u = act(scale * x + shift) in float32 exactly as the kernels
  compute it, and a slot calibrated on u."""
  rows = B * H * W
  g = torch.Generator(device='cuda').manual_seed(seed)
  x = (torch.randn(rows, C, device='cuda', generator=g) * 2).to(dtype)
  ss = torch.cat([torch.rand(C, device='cuda', generator=g) + 0.5, torch.randn(C, device='cuda', generator=g)]).contiguous()
  x32 = x.float().contiguous()
  u = torch.empty_like(x32)
  hip.bn_act_quant_apply(x32, u, rows, C, ss, act, None, 8, False)
  slot = torch.empty((1, 2), dtype=torch.int32, device='cuda')
  hip.minmax_slots_init(slot)
  hip.minmax_tensor(u, slot[0])
  return rows, x, ss, u, slot


def _static(hip, x, rows, C, ss, act, ab, bits, out_dtype):
  out = torch.full((rows, C), 77, dtype=out_dtype, device='cuda')
  hip.bn_act_quant_static(x, out, rows, C, ss, act, ab, bits)
  torch.cuda.synchronize()
  return out


def _bits_of(t):
  """A tensor's raw bits, for bit-for-bit comparisons of float32 / bf16 / uint8 alike."""
  t = t.contiguous()
  return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]).cpu().numpy()


def _narrow_range(u):
  """(lo, hi) = the 10th and 90th percentile of u, as float32 numbers."""
  s = torch.sort(u.reshape(-1).float()).values
  n = s.numel()
  return float(s[n // 10]), float(s[(9 * n) // 10])


def _inner_range(u):
  """(lo, hi) = the 20th and 80th percentile of the POSITIVE part of u.  Behind a ReLU about half of u is exactly 0, so a percentile
  of u itself puts the minimum at 0 and nothing lies below it; this minimum lies strictly above the zeros and a fifth of the
  positive values, and the maximum strictly below another fifth: both halves of the clamp act."""
  s = torch.sort(u.reshape(-1).float()).values
  s = s[s > 0]
  n = s.numel()
  return float(s[n // 5]), float(s[(4 * n) // 5])


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('C', [16, 24, 64])
@pytest.mark.parametrize('bits', [4, 8])
@pytest.mark.parametrize('act', ['Relu', 'Relu6'])
def test_static_pass_on_its_own_range_is_the_per_batch_pass(hip, act, bits, C, dtype):
  """The range calibrated on the tensor itself: the clamp never acts, codes and values are those of pf_bn_act_quant_codes /
  pf_bn_act_quant_apply bit for bit (C = 24 takes the scalar path)."""
  rows, x, ss, _, slot = _bn_case(hip, C, act, dtype, 11 * C + bits)
  ab = hip.minmax_decode(slot)[0].contiguous()
  codes = torch.full((rows, C), 77, dtype=torch.uint8, device='cuda')
  ab_out = torch.empty(2, device='cuda')
  hip.bn_act_quant_codes(x, codes, rows, C, ss, act, slot[0], bits, ab_out)
  q = torch.empty_like(x)
  hip.bn_act_quant_apply(x, q, rows, C, ss, act, slot[0], bits, True)
  got_codes = _static(hip, x, rows, C, ss, act, ab, bits, torch.uint8)
  assert torch.equal(got_codes, codes) and int(codes.max()) == 2 ** bits - 1 and int(codes.min()) == 0
  got_q = _static(hip, x, rows, C, ss, act, ab, bits, dtype)
  assert np.array_equal(_bits_of(got_q), _bits_of(q))
  assert torch.equal(got_codes, _static(hip, x, rows, C, ss, act, ab, bits, torch.uint8))          # two calls, the same bits


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('C', [16, 24, 64])
@pytest.mark.parametrize('bits', [4, 8])
@pytest.mark.parametrize('act', ['Relu', 'Relu6'])
@pytest.mark.parametrize('which', ['percentile', 'inner'])
def test_static_pass_on_a_narrowed_range_is_the_oracle(hip, which, act, bits, C, dtype):
  """A narrowed range: codes = int8.static_codes, values = int8.static_value, bit for bit, and both end codes occur.
  'percentile': the 10th - 90th percentile of u.  At least 5 % of the elements lie strictly above the maximum and clamp; behind a
  ReLU the 10th percentile is 0 itself, the minimum of u, so nothing can lie strictly below it -- there the share at the minimum is
  asserted, and the lower half of the clamp is the business of the other range.
  'inner': the 20th - 80th percentile of the positive part of u.  At least 5 % of the elements lie STRICTLY beyond each end: both
  halves of the device clamp act (without the lower one the values of u < min would come out below the range)."""
  rows, x, ss, u, _ = _bn_case(hip, C, act, dtype, 11 * C + bits)
  lo, hi = _narrow_range(u) if which == 'percentile' else _inner_range(u)
  assert lo < hi
  alpha, beta = int8.range_alpha_beta(lo, hi)
  ab = dev(np.array([alpha, beta], np.float32))
  uh = u.cpu().numpy()
  want = int8.static_codes(uh, alpha, beta, bits)
  k = 2 ** bits - 1
  low, high = float((uh <= lo).mean()), float((uh >= hi).mean())
  print('C=%d %s bits=%d: range [%g, %g], share at or below %.3f (strictly %.3f), at or above %.3f (strictly %.3f)'
        % (C, act, bits, lo, hi, low, float((uh < lo).mean()), high, float((uh > hi).mean())))
  assert float((uh > hi).mean()) >= 0.05 and low >= 0.05
  if which == 'inner':
    assert lo > 0 and float((uh < lo).mean()) >= 0.05
    t = (uh.astype(np.float64) - float(beta)) / float(alpha) * k        # unclamped: really below 0 and above k
    assert float((t < -0.5).mean()) >= 0.05 and float((t > k).mean()) >= 0.05
  assert want.min() == 0 and want.max() == k
  got = _static(hip, x, rows, C, ss, act, ab, bits, torch.uint8).cpu().numpy()
  assert np.array_equal(got, want)
  val = int8.static_value(want, alpha, beta, bits)
  got32 = _static(hip, x, rows, C, ss, act, ab, bits, torch.float32).cpu().numpy()
  assert np.array_equal(got32.view(np.uint32), val.view(np.uint32))
  assert got32.min() == np.float32(beta) and got32.max() == val.max()                        # nothing leaves the range
  got16 = _static(hip, x, rows, C, ss, act, ab, bits, torch.bfloat16)
  assert torch.equal(got16.cpu(), torch.from_numpy(val).to(torch.bfloat16))


# ------------------------------------------------------------------------------------------------
# the requantising epilogues
# ------------------------------------------------------------------------------------------------

def _consumer(hip, y32, Cn, act, seed):
  """A consumer BatchNorm for the float32 parent output y32 [M][Cn]: scale / shift that centre it, and ONE narrowed output range,
  strictly inside the positive part of u (_inner_range), so that both halves of the clamp act in the epilogue.  Returns (scale_shift,
  alpha_beta on the device, share of u strictly below the range, share strictly above)."""
  g = torch.Generator(device='cuda').manual_seed(seed)
  std = float(y32.std()) + 1e-6
  scale = (torch.rand(Cn, device='cuda', generator=g) + 0.5) * (1.0 / std)       # u spreads over about [-3, 4]: ReLU6's 6 stays out of reach
  shift = torch.randn(Cn, device='cuda', generator=g) - scale * float(y32.mean())
  ss = torch.cat([scale, shift]).contiguous()
  M = y32.numel() // Cn
  u = torch.empty_like(y32)
  hip.bn_act_quant_apply(y32, u, M, Cn, ss, act, None, 8, False)
  lo, hi = _inner_range(u) if int((u > 0).sum()) >= 10 else (0.0, 0.0)
  if not lo < hi:                                 # a one-pixel image: any range that cuts through the values
    lo, hi = 0.25, 1.5
  alpha, beta = int8.range_alpha_beta(lo, hi)
  return ss, dev(np.array([alpha, beta], np.float32)), float((u < lo).float().mean()), float((u > hi).float().mean())


def _conv_layer(rng, C, N, R):
  d_hwio = rng.integers(0, 256, size=(R, R, C, N)).astype(np.uint8)
  meta = np.array([8, ex.MODE_CHANNEL, 0, R, R, C, N], np.int64)
  return int8.pack_layer(ex.pack_codes(d_hwio.reshape(-1), 8), rng.uniform(0.05, 0.6, N).astype(np.float32),
                         (-rng.uniform(0.02, 0.3, N)).astype(np.float32), meta)


@pytest.mark.parametrize('N', [8, 72, 256])
@pytest.mark.parametrize('C', [16, 64])
@pytest.mark.parametrize('R,stride,pad', GEOMS)
def test_conv_epilogue_is_the_static_pass_on_the_float32_output(hip, R, stride, pad, C, N):
  rng = np.random.default_rng(R * 1000 + stride * 100 + C * 7 + N)
  c = dev(rng.integers(0, 256, size=(B, H, W, C)).astype(np.uint8))
  p = _conv_layer(rng, C, N, R)
  tabs = (dev(p['scale_beta']), dev(p['tsum']), dev(p['tapsum']))
  w = dev(p['w'])
  Ho, Wo = int8.out_size(H, R, stride, pad), int8.out_size(W, R, stride, pad)
  M = B * Ho * Wo
  alpha_a = float(np.float32(rng.uniform(1.0, 6.0)))
  for i, beta_a in enumerate((0.0, float(np.float32(0.37)))):
    ab = dev(np.array([alpha_a, beta_a], np.float32))
    y32 = torch.empty((B, Ho, Wo, N), dtype=torch.float32, device='cuda')
    hip.conv_i8_fwd(c, w, ab, 8, *tabs, y32, B, H, W, C, N, R, R, stride, pad, pad, Ho, Wo)
    act = ('Relu', 'Relu6')[i]
    ss, oab, below, above = _consumer(hip, y32, N, act, C + N + i)
    print('conv R=%d stride=%d C=%d N=%d beta_a=%g: %.3f of u strictly below the range, %.3f strictly above' % (R, stride, C, N, beta_a, below, above))
    assert below >= 0.05 and above >= 0.05          # the epilogue really clamps at both ends
    for bits in (4, 8):
      seen = set()
      for kind in KINDS:
        want = _static(hip, y32, M, N, ss, act, oab, bits, kind)
        out = torch.full((B, Ho, Wo, N), 77, dtype=kind, device='cuda')
        hip.conv_i8_fwd_q(c, w, ab, 8, *tabs, ss, act, oab, bits, out, B, H, W, C, N, R, R, stride, pad, pad, Ho, Wo)
        torch.cuda.synchronize()
        assert np.array_equal(_bits_of(out).reshape(-1), _bits_of(want).reshape(-1)), (beta_a, bits, kind)
        again = torch.full_like(out, 55)
        hip.conv_i8_fwd_q(c, w, ab, 8, *tabs, ss, act, oab, bits, again, B, H, W, C, N, R, R, stride, pad, pad, Ho, Wo)
        assert torch.equal(out, again)
        if kind == torch.uint8:
          seen = {int(out.min()), int(out.max())}
      assert seen == {0, 2 ** bits - 1}             # the epilogue clamped at both ends


def _dw_kernel(rng, C):
  d_hwio = rng.integers(0, 256, size=(3, 3, C, 1)).astype(np.uint8)
  meta = np.array([8, ex.MODE_TENSOR, 0, 3, 3, C, 1], np.int64)
  return int8.pack_depthwise(ex.pack_codes(d_hwio.reshape(-1), 8), np.array([rng.uniform(0.05, 0.6)], np.float32),
                             np.array([-rng.uniform(0.02, 0.3)], np.float32), meta)


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('Hh,Ww,C', DW_CASES)
def test_depthwise_epilogue_is_the_static_pass_on_the_float32_output(hip, Hh, Ww, C, stride):
  rng = np.random.default_rng(1000 * Hh + 100 * Ww + C * 7 + stride)
  c = dev(rng.integers(0, 256, size=(B, Hh, Ww, C)).astype(np.uint8))
  p = _dw_kernel(rng, C)
  wcol, wsb = dev(p['wcol'].view(np.int32)), dev(p['scale_beta'])
  Ho, Wo = -(-Hh // stride), -(-Ww // stride)
  ph, pw = int8.same_pads(Hh, 3, stride)[0], int8.same_pads(Ww, 3, stride)[0]
  M = B * Ho * Wo
  alpha_a = float(np.float32(rng.uniform(1.0, 6.0)))
  for i, beta_a in enumerate((0.0, float(np.float32(0.37)))):
    ab = dev(np.array([alpha_a, beta_a], np.float32))
    y32 = torch.empty((B, Ho, Wo, C), dtype=torch.float32, device='cuda')
    hip.dw_i8_fwd(c, wcol, wsb, ab, 8, y32, B, Hh, Ww, C, stride, ph, pw, Ho, Wo)
    act = ('Relu6', 'Relu')[i]
    ss, oab, below, above = _consumer(hip, y32, C, act, C + Hh + i)
    print('dw %dx%dx%d stride=%d beta_a=%g: %.3f of u strictly below the range, %.3f strictly above' % (Hh, Ww, C, stride, beta_a, below, above))
    if M * C >= 1000:
      assert below >= 0.05 and above >= 0.05        # the epilogue really clamps at both ends
    for bits in (4, 8):
      for kind in KINDS:
        want = _static(hip, y32, M, C, ss, act, oab, bits, kind)
        out = torch.full((B, Ho, Wo, C), 77, dtype=kind, device='cuda')
        hip.dw_i8_fwd_q(c, wcol, wsb, ab, 8, ss, act, oab, bits, out, B, Hh, Ww, C, stride, ph, pw, Ho, Wo)
        torch.cuda.synchronize()
        assert np.array_equal(_bits_of(out).reshape(-1), _bits_of(want).reshape(-1)), (beta_a, bits, kind)
        again = torch.full_like(out, 55)
        hip.dw_i8_fwd_q(c, wcol, wsb, ab, 8, ss, act, oab, bits, again, B, Hh, Ww, C, stride, ph, pw, Ho, Wo)
        assert torch.equal(out, again)
        if kind == torch.uint8 and M * C >= 1000:
          assert {int(out.min()), int(out.max())} == {0, 2 ** bits - 1}


def test_entries_refuse_what_they_do_not_cover(hip):
  """A null pointer, an ineligible shape, an unknown output kind and (convolution) a residual return non-zero from the C entries and
  leave a canary-filled output untouched; the same calls with nothing wrong are taken."""
  lib = hip._lib
  Hh = Ww = 6
  ss16, ss48 = torch.ones(2 * 16, device='cuda'), torch.ones(2 * 48, device='cuda')
  oab = torch.tensor([1.0, 0.0], device='cuda')
  ab = torch.tensor([1.0, 0.0], device='cuda')

  # ---- a: the stand-alone pass
  x = torch.zeros((10, 16), device='cuda')
  out = torch.full((10, 16), 12345.0, device='cuda')

  def call_a(x_, out_, ss_, oab_, kind=1, C=16, bits=8, rows=10):
    return lib.pf_bn_act_quant_static(_ptr(x_), _ptr(out_), c_int(hip.PF_F32), c_int(kind), c_int64(rows), c_int(C), _ptr(ss_), c_int(1),
                                      _ptr(oab_), c_int(bits), c_void_p(0))
  for args in ((None, out, ss16, oab), (x, None, ss16, oab), (x, out, None, oab), (x, out, ss16, None)):
    assert call_a(*args) != 0
  assert call_a(x, out, ss16, oab, kind=3) != 0 and call_a(x, out, ss16, oab, C=0) != 0 and call_a(x, out, ss16, oab, rows=0) != 0
  assert call_a(x, out, ss16, oab, kind=0, bits=9) != 0 and call_a(x, out, ss16, oab, bits=0) != 0
  torch.cuda.synchronize()
  assert bool((out == 12345.0).all())
  assert call_a(x, out, ss16, oab) == 0
  torch.cuda.synchronize()
  assert bool((out == 1.0).all())                                     # relu(1 * 0 + 1) = 1 = the top of the range [0, 1]

  # ---- b: the depthwise epilogue
  xc = torch.zeros((B, Hh, Ww, 48), dtype=torch.uint8, device='cuda')
  wcol = torch.zeros((48, 3), dtype=torch.int32, device='cuda')
  wsb = torch.ones(2, device='cuda')
  y = torch.full((B, Hh, Ww, 48), 12345.0, device='cuda')

  def call_b(x_, wcol_, wsb_, ab_, ss_, oab_, y_, C=48, stride=1, kind=1, bits=8):
    return lib.pf_dw_i8_fwd_q(_ptr(x_), _ptr(wcol_), _ptr(wsb_), _ptr(ab_), c_int(8), _ptr(ss_), c_int(2), _ptr(oab_), c_int(bits), _ptr(y_),
                              c_int(kind), c_int(B), c_int(Hh), c_int(Ww), c_int(C), c_int(stride), c_int(1), c_int(1), c_int(Hh), c_int(Ww),
                              c_void_p(0))
  good = (xc, wcol, wsb, ab, ss48, oab, y)
  for i in range(len(good)):
    assert call_b(*[None if j == i else t for j, t in enumerate(good)]) != 0
  assert call_b(*good, C=24) != 0 and call_b(*good, stride=3) != 0 and call_b(*good, kind=7) != 0 and call_b(*good, bits=9) != 0
  torch.cuda.synchronize()
  assert bool((y == 12345.0).all())
  assert call_b(*good) == 0
  torch.cuda.synchronize()
  assert bool((y == 1.0).all())                                       # y = 0 everywhere, relu6(0 + 1) = 1

  # ---- c: the convolution epilogue
  rng = np.random.default_rng(0)
  p = _conv_layer(rng, 16, 8, 1)
  xk = torch.zeros((B, Hh, Ww, 16), dtype=torch.uint8, device='cuda')
  w, wtab, tsum, tap = dev(p['w']), dev(p['scale_beta']), dev(p['tsum']), dev(p['tapsum'])
  ss8 = torch.ones(2 * 8, device='cuda')
  yc = torch.full((B, Hh, Ww, 8), 12345.0, device='cuda')
  res = torch.zeros((B, Hh, Ww, 8), device='cuda')

  def call_c(x_, w_, ab_, wtab_, tsum_, tap_, ss_, oab_, y_, res_=None, C=16, stride=1, kind=1, bits=8):
    return lib.pf_conv_i8_fwd_q(_ptr(x_), _ptr(w_), _ptr(ab_), c_int(8), _ptr(wtab_), _ptr(tsum_), _ptr(tap_), _ptr(res_), _ptr(ss_), c_int(1),
                                _ptr(oab_), c_int(bits), _ptr(y_), c_int(kind), c_int(B), c_int(Hh), c_int(Ww), c_int(C), c_int(8), c_int(1),
                                c_int(1), c_int(stride), c_int(0), c_int(0), c_int(Hh), c_int(Ww), c_void_p(0))
  good = (xk, w, ab, wtab, tsum, tap, ss8, oab, yc)
  for i in range(len(good)):
    assert call_c(*[None if j == i else t for j, t in enumerate(good)]) != 0
  assert call_c(*good, res_=res) != 0                                 # a residual is refused
  assert call_c(*good, C=24) != 0 and call_c(*good, stride=3) != 0 and call_c(*good, kind=-1) != 0 and call_c(*good, bits=9) != 0
  torch.cuda.synchronize()
  assert bool((yc == 12345.0).all())
  with pytest.raises(TypeError):
    hip.bn_act_quant_static(x, torch.empty((10, 16), dtype=torch.int32, device='cuda'), 10, 16, ss16, 'Relu', oab, 8)
  with pytest.raises(ValueError):
    hip.bn_act_quant_static(x, torch.empty((10, 16), dtype=torch.uint8, device='cuda'), 10, 16, ss16, 'Relu', oab, 9)
  assert call_c(*good) == 0
  torch.cuda.synchronize()
  assert bool(torch.isfinite(yc).all()) and not bool((yc == 12345.0).any())
