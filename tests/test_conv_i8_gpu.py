"""pf_conv_i8_fwd and pf_bn_act_quant_codes (through hip.py) against int8.conv_reference and pf_bn_act_quant_apply.

The exact case pins the lane maps of v_mfma_i32_16x16x64_i8: with integer-valued scales every term of the layer formula is an
integer below 2^24, so the float32 output has to equal the reference bit for bit."""
from ctypes import c_int, c_void_p

import numpy as np
import pytest
import torch

from pocketflow_amd import int8
from pocketflow_amd.tools.conversion import export_quant_int8_model as ex

pytestmark = pytest.mark.gpu

B, H, W = 2, 13, 11
GEOMS = [(1, 1, 0), (1, 2, 0), (3, 1, 1), (3, 2, 1)]          # (R = S, stride, pad)


@pytest.fixture(scope='module')
def hip():
  from pocketflow_amd import hip as h
  assert torch.cuda.is_available(), 'gpu tests need a GPU'
  return h


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _layer(rng, C, N, R, bits_w, alpha_w, beta_w):
  d_hwio = rng.integers(0, 2 ** bits_w, size=(R, R, C, N)).astype(np.uint8)
  d_hwio.reshape(-1, N)[0, :] = 2 ** bits_w - 1                # both ends of the grid occur
  d_hwio.reshape(-1, N)[1, :] = 0
  meta = np.array([bits_w, ex.MODE_CHANNEL, 0, R, R, C, N], np.int64)
  return int8.pack_layer(ex.pack_codes(d_hwio.reshape(-1), bits_w), alpha_w.astype(np.float32), beta_w.astype(np.float32), meta)


def _run(hip, c, p, alpha_a, beta_a, stride, pad, out_dtype, residual=None):
  R, S, C, N = p['shape']
  Ho, Wo = int8.out_size(H, R, stride, pad), int8.out_size(W, S, stride, pad)
  y = torch.full((B, Ho, Wo, N), float('nan'), dtype=out_dtype, device='cuda')
  ab = dev(np.array([alpha_a, beta_a], np.float32))
  hip.conv_i8_fwd(dev(c), dev(p['w']), ab, 8, dev(p['scale_beta']), dev(p['tsum']), dev(p['tapsum']), y, B, H, W, C, N, R, S, stride, pad,
                  pad, Ho, Wo, residual=residual)
  torch.cuda.synchronize()
  return y


def _ref(c, p, alpha_a, beta_a, stride, pad, residual=None):
  return int8.conv_reference(c, alpha_a, beta_a, 8, p['d'], p['alpha'], p['beta'], p['bits'], stride, pad, pad, residual=residual,
                             terms=True)


@pytest.mark.parametrize('beta_a', [0.0, 1.0])
@pytest.mark.parametrize('N', [8, 72, 256])
@pytest.mark.parametrize('C', [16, 48, 64])
@pytest.mark.parametrize('R,stride,pad', GEOMS)
def test_exact_case_is_bit_for_bit(hip, R, stride, pad, C, N, beta_a):
  """alpha_a = 255 (step 1), alpha_w = 15 * 2^e over 4-bit codes (step 2^e), integer beta_w and beta_a: every term an integer < 2^24."""
  rng = np.random.default_rng(R * 1000 + stride * 100 + C + N)
  c = rng.integers(0, 256, size=(B, H, W, C)).astype(np.uint8)
  c[0, 0, 0, :2] = (0, 255)
  p = _layer(rng, C, N, R, 4, 15.0 * 2.0 ** rng.integers(0, 2, N), -rng.integers(0, 3, N).astype(np.float64))
  want, mag = _ref(c, p, 255.0, beta_a, stride, pad)
  assert mag.max() < 2 ** 24 and np.array_equal(want, np.rint(want))
  got = _run(hip, c, p, 255.0, beta_a, stride, pad, torch.float32).cpu().numpy()
  bad = np.argwhere(got != want.astype(np.float32))
  assert bad.size == 0, (len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
  res = rng.integers(-1000, 1000, size=want.shape).astype(np.float32)
  want_r, mag_r = _ref(c, p, 255.0, beta_a, stride, pad, residual=res)
  assert mag_r.max() < 2 ** 24
  got_r = _run(hip, c, p, 255.0, beta_a, stride, pad, torch.float32, residual=dev(res)).cpu().numpy()
  assert np.array_equal(got_r, want_r.astype(np.float32))


@pytest.mark.parametrize('N', [8, 72, 256])
@pytest.mark.parametrize('C', [16, 48, 64, 256])
@pytest.mark.parametrize('R,stride,pad', GEOMS)
def test_general_parameters_and_determinism(hip, R, stride, pad, C, N):
  """float32 output within 1e-5 * sum |terms| of the reference (a handful of float32 roundings of the largest term); bf16 output
  additionally 2^-8 |y| for its one rounding; a residual goes in before that rounding; two calls give the same bits."""
  rng = np.random.default_rng(R * 1000 + stride * 100 + C * 7 + N)
  c = rng.integers(0, 256, size=(B, H, W, C)).astype(np.uint8)
  p = _layer(rng, C, N, R, 8, rng.uniform(0.05, 0.6, N), -rng.uniform(0.02, 0.3, N))
  alpha_a = float(np.float32(rng.uniform(1.0, 6.0)))
  for beta_a in (0.0, float(np.float32(0.37))):
    want, mag = _ref(c, p, alpha_a, beta_a, stride, pad)
    y32 = _run(hip, c, p, alpha_a, beta_a, stride, pad, torch.float32)
    err = np.abs(y32.cpu().numpy().astype(np.float64) - want)
    assert np.all(err <= 1e-5 * mag), (beta_a, float((err / mag).max()))
    assert torch.equal(y32, _run(hip, c, p, alpha_a, beta_a, stride, pad, torch.float32))
    res = torch.randn(want.shape, device='cuda').to(torch.bfloat16)
    want_r, mag_r = _ref(c, p, alpha_a, beta_a, stride, pad, residual=res.float().cpu().numpy())
    y16 = _run(hip, c, p, alpha_a, beta_a, stride, pad, torch.bfloat16, residual=res)
    err = np.abs(y16.float().cpu().numpy().astype(np.float64) - want_r)
    assert np.all(err <= 1e-5 * mag_r + 2.0 ** -8 * np.abs(want_r)), (beta_a, float((err / (1e-5 * mag_r + 2.0 ** -8 * np.abs(want_r))).max()))
    assert torch.equal(y16, _run(hip, c, p, alpha_a, beta_a, stride, pad, torch.bfloat16, residual=res))


def test_entry_point_rejects_what_it_does_not_cover(hip):
  rng = np.random.default_rng(0)
  p = _layer(rng, 16, 8, 1, 8, np.ones(8), np.zeros(8))
  c = dev(np.zeros((B, H, W, 16), np.uint8))
  ab = dev(np.array([1.0, 0.0], np.float32))
  y = torch.empty((B, H, W, 8), device='cuda')
  args = (dev(p['w']), ab, 8, dev(p['scale_beta']), dev(p['tsum']), dev(p['tapsum']), y)
  with pytest.raises(ValueError, match='not eligible'):
    hip.conv_i8_fwd(c, *args, B, H, W, 16, 8, 1, 1, 3, 0, 0, H, W)
  with pytest.raises(ValueError, match='beyond'):
    hip.conv_i8_fwd(c, *args, B, H, W, 16, 8, 1, 1, 2, 0, 0, H, W)
  with pytest.raises(TypeError):
    hip.conv_i8_fwd(c.float(), *args, B, H, W, 16, 8, 1, 1, 1, 0, 0, H, W)


def _small_operands():
  """2 images of 6 x 6, 16 -> 8 channels, 1 x 1, codes all 0 and unit scales (every output is 0); the output holds a canary."""
  p = _layer(np.random.default_rng(0), 16, 8, 1, 8, np.ones(8), np.zeros(8))
  x = torch.zeros((B, 6, 6, 16), dtype=torch.uint8, device='cuda')
  ab = torch.tensor([1.0, 0.0], device='cuda')
  y = torch.full((B, 6, 6, 8), 12345.0, device='cuda')
  return x, dev(p['w']), ab, dev(p['scale_beta']), dev(p['tsum']), dev(p['tapsum']), y


def test_c_entry_refuses_what_it_does_not_cover(hip):
  """pf_conv_i8_fwd itself (its checks are the setup shared with pf_conv_i8_fwd_q plus its own operands): every defect returns
  non-zero before a launch and leaves the canary-filled output untouched; the same call with nothing wrong is taken."""
  lib = hip._lib
  ptr = lambda t: c_void_p(0 if t is None else t.data_ptr())
  good = _small_operands()
  y = good[-1]

  def call(x, w, ab, wtab, tsum, tap, y_, C=16, stride=1, act_bits=8, dtype=hip.PF_F32, Ho=6):
    return lib.pf_conv_i8_fwd(ptr(x), ptr(w), ptr(ab), c_int(act_bits), ptr(wtab), ptr(tsum), ptr(tap), c_void_p(0), ptr(y_), c_int(dtype),
                              c_int(B), c_int(6), c_int(6), c_int(C), c_int(8), c_int(1), c_int(1), c_int(stride), c_int(0), c_int(0),
                              c_int(Ho), c_int(Ho), c_void_p(0))
  for i in range(len(good)):
    assert call(*[None if j == i else t for j, t in enumerate(good)]) != 0, i
  assert call(*good, C=24) != 0 and call(*good, stride=3) != 0
  assert call(*good, act_bits=0) != 0 and call(*good, act_bits=9) != 0
  assert call(*good, dtype=7) != 0
  assert call(*good, stride=2) != 0                                   # Ho = H at stride 2: the output window leaves the input
  torch.cuda.synchronize()
  assert bool((y == 12345.0).all())
  assert call(*good) == 0
  torch.cuda.synchronize()
  assert bool((y == 0.0).all())


def test_requantising_wrapper_refuses_what_it_does_not_cover(hip):
  """hip.conv_i8_fwd_q shares its operand checks with hip.conv_i8_fwd: the same defects, refused under its own name."""
  x, w, ab, wtab, tsum, tap, _ = _small_operands()
  ss, oab = torch.ones(2 * 8, device='cuda'), torch.tensor([1.0, 0.0], device='cuda')
  out = torch.zeros((B, 6, 6, 8), dtype=torch.uint8, device='cuda')

  def call(x_=x, out_=out, stride=1, bits=8):
    hip.conv_i8_fwd_q(x_, w, ab, 8, wtab, tsum, tap, ss, 'Relu', oab, bits, out_, B, 6, 6, 16, 8, 1, 1, stride, 0, 0, 6, 6)
  with pytest.raises(ValueError, match='^conv_i8_fwd_q: .*not eligible'):
    call(stride=3)
  with pytest.raises(ValueError, match='^conv_i8_fwd_q: .*beyond'):
    call(stride=2)
  with pytest.raises(TypeError, match='^conv_i8_fwd_q: '):
    call(x_=x.float())
  with pytest.raises(ValueError, match='^conv_i8_fwd_q: '):
    call(bits=9)
  with pytest.raises(ValueError, match='^conv_i8_fwd_q: '):
    call(out_=out.float(), bits=9)                                    # a value output: still at most 8 bits in an epilogue


# ------------------------------------------------------------------------------------------------
# the producer
# ------------------------------------------------------------------------------------------------

def _bn_case(hip, C, act, dtype, seed):
  """x [rows][C], scale / shift, y = act(scale * x + shift) in float32 exactly as the kernels compute it, and the slot calibrated on y."""
  rows = B * H * W                                            # 286: no multiple of any row block
  g = torch.Generator(device='cuda').manual_seed(seed)
  x = (torch.randn(rows, C, device='cuda', generator=g) * 2).to(dtype)
  ss = torch.cat([torch.rand(C, device='cuda', generator=g) + 0.5, torch.randn(C, device='cuda', generator=g)]).contiguous()
  x32 = x.float().contiguous()                                 # the float32 value the kernels load
  y = torch.empty_like(x32)
  hip.bn_act_quant_apply(x32, y, rows, C, ss, act, None, 8, False)
  slot = torch.empty((1, 2), dtype=torch.int32, device='cuda')
  hip.minmax_slots_init(slot)
  hip.minmax_tensor(y, slot[0])
  return rows, x, ss, y, slot


def _codes(hip, x, rows, C, ss, act, slot, bits):
  codes = torch.full((rows, C), 77, dtype=torch.uint8, device='cuda')
  ab = torch.full((2,), float('nan'), device='cuda')
  hip.bn_act_quant_codes(x, codes, rows, C, ss, act, slot[0], bits, ab)
  torch.cuda.synchronize()
  return codes.cpu().numpy(), ab.cpu().numpy()


@pytest.mark.parametrize('C', [16, 24, 64])
@pytest.mark.parametrize('bits', [4, 8])
@pytest.mark.parametrize('act', ['Relu', 'Relu6'])
def test_codes_make_the_rounding_decision_of_the_apply_pass(hip, act, bits, C):
  rows, x, ss, _, slot = _bn_case(hip, C, act, torch.float32, 11 * C + bits)
  q = torch.empty_like(x)
  hip.bn_act_quant_apply(x, q, rows, C, ss, act, slot[0], bits, True)
  codes, ab = _codes(hip, x, rows, C, ss, act, slot, bits)
  want_ab = hip.minmax_decode(slot).cpu().numpy()[0]
  assert np.array_equal(ab.view(np.uint32), want_ab.view(np.uint32))
  k = np.float32(2 ** bits - 1)
  assert codes.max() <= int(k) and codes.max() == int(k) and codes.min() == 0
  decoded = ab[0] * (codes.astype(np.float32) / k).astype(np.float32) + ab[1]          # __inv_scale: mul, then add
  assert np.array_equal(decoded.astype(np.float32).view(np.uint32), q.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize('C', [16, 24, 64])
@pytest.mark.parametrize('bits', [4, 8])
def test_codes_from_bf16_input(hip, bits, C):
  rows, x, ss, y, slot = _bn_case(hip, C, 'Relu', torch.bfloat16, 5 * C + bits)
  codes, ab = _codes(hip, x, rows, C, ss, 'Relu', slot, bits)
  k = np.float32(2 ** bits - 1)
  yh = y.cpu().numpy()
  want = np.rint(((yh - ab[1]).astype(np.float32) / ab[0]).astype(np.float32) * k)
  assert want.min() >= 0 and want.max() <= k
  assert codes.max() <= int(k) and np.array_equal(codes, want.astype(np.uint8))
