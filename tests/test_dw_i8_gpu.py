"""pf_dw_i8_fwd (through hip.py, and the raw C entry for what it must refuse) against int8.depthwise_reference.

The exact case pins the byte gathering and the dot products of the kernel: with integer-valued scales every term of the layer formula
is an integer below 2^24, so the float32 output has to equal the reference bit for bit and the bf16 output its bf16 rounding."""
from ctypes import c_int, c_void_p

import numpy as np
import pytest
import torch

from pocketflow_amd import int8
from pocketflow_amd.tools.conversion import export_quant_int8_model as ex

pytestmark = pytest.mark.gpu

B = 2
# (H, W, C): the four small images at one and at three channel groups; 28 x 28 x 64 makes several workgroups, full strips and (stride 2) a tail
CASES = [(H, W, C) for (H, W) in ((1, 1), (5, 7), (8, 6), (9, 4)) for C in (16, 48)] + [(28, 28, 64)]
# C = 4080: 255 channel groups in a workgroup of 256 lanes, one strip per workgroup and one lane that leaves at `sl >= a.spb`
CASES += [(9, 4, 4080)]
# stride -> (H, W, C) with more strips than one pass of the capped grid covers: every lane of k_dw_i8 walks its `strip += gridDim.x * spb`
# loop a second time, the second pass ragged; a one-pixel tail strip in every output row (Wo = 5).  21 M and 84 M codes: the narrow
# image keeps the tensors small.
LOOP_CASES = {1: (2060, 5, 1024), 2: (4110, 10, 1024)}


def _strips_and_strips_per_pass(H, W, C, stride):
  """The launcher's arithmetic (pf_dw_i8_fwd, pf_depthwise_i8.hip): strips of 4 output pixels in the tensor, and how many of them the
  grid takes in one pass -- 256 lanes = cgb channel groups x spb strips, gridDim.x capped at 2048 / gridDim.y."""
  Ho, Wo = -(-H // stride), -(-W // stride)
  total = B * Ho * -(-Wo // 4)
  cgb = min(C // 16, 256)
  spb = 256 // cgb
  gy = -(-(C // 16) // cgb)
  gx = min(-(-total // spb), max(2048 // gy, 1))
  return total, gx * spb


def _check_grid(H, W, C, stride):
  total, per_pass = _strips_and_strips_per_pass(H, W, C, stride)
  if (H, W, C) == LOOP_CASES[stride]:
    assert per_pass == 8192 and per_pass < total < 2 * per_pass and -(-W // stride) % 4 == 1
  else:
    assert total <= per_pass


@pytest.fixture(scope='module')
def hip():
  from pocketflow_amd import hip as h
  assert torch.cuda.is_available(), 'gpu tests need a GPU'
  return h


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _kernel(rng, C, bits_w, alpha_w, beta_w):
  d_hwio = rng.integers(0, 2 ** bits_w, size=(3, 3, C, 1)).astype(np.uint8)
  d_hwio.reshape(-1)[0] = 2 ** bits_w - 1                      # both ends of the grid occur
  d_hwio.reshape(-1)[1] = 0
  meta = np.array([bits_w, ex.MODE_TENSOR, 0, 3, 3, C, 1], np.int64)
  return int8.pack_depthwise(ex.pack_codes(d_hwio.reshape(-1), bits_w), np.array([alpha_w], np.float32), np.array([beta_w], np.float32),
                             meta)


def _run(hip, c, p, alpha_a, beta_a, stride, out_dtype):
  _, H, W, C = c.shape
  Ho, Wo = -(-H // stride), -(-W // stride)
  y = torch.full((B, Ho, Wo, C), float('nan'), dtype=out_dtype, device='cuda')
  ab = dev(np.array([alpha_a, beta_a], np.float32))
  hip.dw_i8_fwd(dev(c), dev(p['wcol'].view(np.int32)), dev(p['scale_beta']), ab, 8, y, B, H, W, C, stride,
                int8.same_pads(H, 3, stride)[0], int8.same_pads(W, 3, stride)[0], Ho, Wo)
  torch.cuda.synchronize()
  return y


def _ref(c, p, alpha_a, beta_a, stride):
  return int8.depthwise_reference(c, alpha_a, beta_a, 8, p['d'], p['alpha'], p['beta'], p['bits'], stride, terms=True)


def _ref_on_device(c, p, alpha_a, beta_a, stride):
  """int8.depthwise_reference line by line in torch on the device (int64 sums, float64 terms in the same order), for the LOOP_CASES:
  numpy needs 3.6 s per call at 21 M outputs, two calls per test.  Elementwise IEEE float64 in the same order: the same bits, which
  `ref_large` asserts on every shape of CASES before a test relies on it."""
  B_, H, W, C = c.shape
  (ph, ph1), (pw, pw1) = int8.same_pads(H, 3, stride), int8.same_pads(W, 3, stride)
  Ho, Wo = -(-H // stride), -(-W // stride)
  ka, kw = float(2 ** 8 - 1), float(2 ** p['bits'] - 1)
  cp = torch.zeros((B_, H + ph + ph1, W + pw + pw1, C), dtype=torch.int64, device='cuda')
  cp[:, ph:ph + H, pw:pw + W] = dev(c)
  inside = torch.zeros((H + ph + ph1, W + pw + pw1), dtype=torch.int64, device='cuda')
  inside[ph:ph + H, pw:pw + W] = 1
  d64 = dev(p['d']).to(torch.int64)
  P = torch.zeros((B_, Ho, Wo, C), dtype=torch.int64, device='cuda')
  Sc = torch.zeros_like(P)
  Dv = torch.zeros((Ho, Wo, C), dtype=torch.int64, device='cuda')
  V = torch.zeros((Ho, Wo), dtype=torch.int64, device='cuda')
  for r in range(3):
    for s in range(3):
      win = cp[:, r:r + (Ho - 1) * stride + 1:stride, s:s + (Wo - 1) * stride + 1:stride]
      ok = inside[r:r + (Ho - 1) * stride + 1:stride, s:s + (Wo - 1) * stride + 1:stride]
      P += win * d64[:, r, s]
      Sc += win
      Dv += ok[:, :, None] * d64[None, None, :, r, s]
      V += ok
  sa, sw, bw = float(alpha_a) / ka, float(p['alpha']) / kw, float(p['beta'])
  t1 = (sa * sw) * P.double()
  t2 = (sa * bw) * Sc.double()
  t3a, t3b = float(beta_a) * (sw * Dv.double())[None], float(beta_a) * (bw * V.double()[..., None])[None]
  y = t1 + t2 + (t3a + t3b)
  mag = t1.abs() + t2.abs() + t3a.abs() + t3b.abs()
  return y.cpu().numpy(), mag.cpu().numpy()


@pytest.fixture(scope='module')
def ref_large(hip):
  """_ref_on_device, after it has reproduced int8.depthwise_reference exactly on every small shape, stride and kind of parameters."""
  rng = np.random.default_rng(7)
  for H, W, C in CASES:
    c = rng.integers(0, 256, size=(B, H, W, C)).astype(np.uint8)
    for stride in (1, 2):
      for p, alpha_a, beta_a in ((_kernel(rng, C, 4, 15.0, -2.0), 255.0, 2.0), (_kernel(rng, C, 8, 0.37, -0.11), 3.3, 0.0),
                                 (_kernel(rng, C, 8, 0.21, -0.05), float(np.float32(1.7)), float(np.float32(0.37)))):
        for got, want in zip(_ref_on_device(c, p, alpha_a, beta_a, stride), _ref(c, p, alpha_a, beta_a, stride)):
          assert got.dtype == want.dtype == np.float64 and np.array_equal(got, want), (H, W, C, stride, alpha_a, beta_a)
  return _ref_on_device


# every (H, W, C) of CASES at both strides (test ids as before), and the loop-entering shape of each stride
PARAMS = [(H, W, C, stride) for stride in (1, 2) for (H, W, C) in CASES] + [LOOP_CASES[stride] + (stride,) for stride in (1, 2)]


@pytest.mark.parametrize('beta_a', [0.0, 2.0])
@pytest.mark.parametrize('H,W,C,stride', PARAMS)
def test_exact_case_is_bit_for_bit(hip, ref_large, H, W, C, stride, beta_a):
  """alpha_a = 255 (step 1), alpha_w = 15 * 2^e over 4-bit codes (step 2^e), integer beta_w and beta_a: every term an integer < 2^24."""
  _check_grid(H, W, C, stride)
  ref = ref_large if (H, W, C) == LOOP_CASES[stride] else _ref
  rng = np.random.default_rng(1000 * H + 100 * W + C + stride)
  c = rng.integers(0, 256, size=(B, H, W, C)).astype(np.uint8)
  c.reshape(-1)[:2] = (0, 255)
  p = _kernel(rng, C, 4, 15.0 * 2.0 ** int(rng.integers(0, 2)), -float(rng.integers(1, 3)))
  want, mag = ref(c, p, 255.0, beta_a, stride)
  assert mag.max() < 2 ** 24 and np.array_equal(want, np.rint(want))
  got = _run(hip, c, p, 255.0, beta_a, stride, torch.float32).cpu().numpy()
  bad = np.argwhere(got != want.astype(np.float32))
  assert bad.size == 0, (len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
  got16 = _run(hip, c, p, 255.0, beta_a, stride, torch.bfloat16).cpu()
  assert torch.equal(got16, torch.from_numpy(want.astype(np.float32)).to(torch.bfloat16))


@pytest.mark.parametrize('H,W,C,stride', PARAMS)
def test_general_parameters_and_determinism(hip, ref_large, H, W, C, stride):
  """float32 output within 1e-5 * sum |terms| of the reference (a few float32 ulps of the summed term magnitudes); bf16 output
  additionally 2^-8 |y| for its one rounding; two calls give the same bits."""
  _check_grid(H, W, C, stride)
  ref = ref_large if (H, W, C) == LOOP_CASES[stride] else _ref
  rng = np.random.default_rng(1000 * H + 100 * W + C * 7 + stride)
  c = rng.integers(0, 256, size=(B, H, W, C)).astype(np.uint8)
  p = _kernel(rng, C, 8, float(rng.uniform(0.05, 0.6)), -float(rng.uniform(0.02, 0.3)))
  alpha_a = float(np.float32(rng.uniform(1.0, 6.0)))
  for beta_a in (0.0, float(np.float32(0.37))):
    want, mag = ref(c, p, alpha_a, beta_a, stride)
    y32 = _run(hip, c, p, alpha_a, beta_a, stride, torch.float32)
    err = np.abs(y32.cpu().numpy().astype(np.float64) - want)
    print('f32', H, W, C, stride, beta_a, float((err / mag).max()))
    assert np.all(err <= 1e-5 * mag), (beta_a, float((err / mag).max()))
    assert torch.equal(y32, _run(hip, c, p, alpha_a, beta_a, stride, torch.float32))
    y16 = _run(hip, c, p, alpha_a, beta_a, stride, torch.bfloat16)
    err = np.abs(y16.float().cpu().numpy().astype(np.float64) - want)
    bar = 1e-5 * mag + 2.0 ** -8 * np.abs(want)
    print('bf16', H, W, C, stride, beta_a, float((err / bar).max()))
    assert np.all(err <= bar), (beta_a, float((err / bar).max()))
    assert torch.equal(y16, _run(hip, c, p, alpha_a, beta_a, stride, torch.bfloat16))


def test_entry_point_rejects_what_it_does_not_cover(hip):
  """C = 24, stride 3, 0 or 9 activation bits, an unknown output dtype and a null pointer return non-zero from the C entry and leave a
  canary-filled output untouched; k = 5 is refused by the predicate (the forward entry is 3 x 3 only and takes no k)."""
  H = W = 6
  lib = hip._lib

  def call(x, wcol, wsb, ab, y, C, stride, act_bits=8, dtype=0):
    ptr = lambda t: c_void_p(0 if t is None else t.data_ptr())
    return lib.pf_dw_i8_fwd(ptr(x), ptr(wcol), ptr(wsb), ptr(ab), c_int(act_bits), ptr(y), c_int(dtype), c_int(B), c_int(H), c_int(W),
                            c_int(C), c_int(stride), c_int(1), c_int(1), c_int(H), c_int(W), c_void_p(0))
  x = torch.zeros((B, H, W, 48), dtype=torch.uint8, device='cuda')
  wcol = torch.zeros((48, 3), dtype=torch.int32, device='cuda')
  wsb = torch.ones(2, device='cuda')
  ab = torch.tensor([1.0, 0.0], device='cuda')
  y = torch.full((B, H, W, 48), 12345.0, device='cuda')
  assert call(x, wcol, wsb, ab, y, 24, 1) != 0
  assert call(x, wcol, wsb, ab, y, 16, 3) != 0 and call(x, wcol, wsb, ab, y, 48, 3) != 0
  assert call(x, wcol, wsb, ab, y, 48, 1, act_bits=0) != 0 and call(x, wcol, wsb, ab, y, 48, 1, act_bits=9) != 0
  assert call(x, wcol, wsb, ab, y, 48, 1, dtype=7) != 0
  assert not hip.dw_i8_supported(16, 5, 1) and not hip.dw_i8_supported(24, 3, 1) and not hip.dw_i8_supported(16, 3, 3)
  for args in ((None, wcol, wsb, ab, y), (x, None, wsb, ab, y), (x, wcol, None, ab, y), (x, wcol, wsb, None, y), (x, wcol, wsb, ab, None)):
    assert call(*args, 16, 1) != 0 and call(*args, 48, 1) != 0
  torch.cuda.synchronize()
  assert bool((y == 12345.0).all())
  with pytest.raises(ValueError, match='not eligible'):
    hip.dw_i8_fwd(x, wcol, wsb, ab, 8, y, B, H, W, 24, 1, 1, 1, H, W)
  with pytest.raises(TypeError):
    hip.dw_i8_fwd(x.float(), wcol, wsb, ab, 8, y, B, H, W, 48, 1, 1, 1, H, W)
  assert call(x, wcol, wsb, ab, y, 48, 1) == 0                       # the same call with nothing wrong is taken
  torch.cuda.synchronize()
  assert bool((y == 0.0).all())


def test_requantising_wrapper_refuses_what_it_does_not_cover(hip):
  """hip.dw_i8_fwd_q shares its operand checks with hip.dw_i8_fwd: the same defects, refused under its own name."""
  H = W = 6
  x = torch.zeros((B, H, W, 48), dtype=torch.uint8, device='cuda')
  wcol = torch.zeros((48, 3), dtype=torch.int32, device='cuda')
  wsb, ss = torch.ones(2, device='cuda'), torch.ones(2 * 48, device='cuda')
  ab = oab = torch.tensor([1.0, 0.0], device='cuda')
  out = torch.zeros((B, H, W, 48), dtype=torch.uint8, device='cuda')

  def call(x_=x, out_=out, stride=1, bits=8):
    hip.dw_i8_fwd_q(x_, wcol, wsb, ab, 8, ss, 'Relu6', oab, bits, out_, B, H, W, 48, stride, 1, 1, H, W)
  with pytest.raises(ValueError, match='^dw_i8_fwd_q: .*not eligible'):
    call(stride=3)
  with pytest.raises(TypeError, match='^dw_i8_fwd_q: '):
    call(x_=x.float())
  with pytest.raises(ValueError, match='^dw_i8_fwd_q: '):
    call(bits=9)
  with pytest.raises(ValueError, match='^dw_i8_fwd_q: '):
    call(out_=out.float(), bits=9)                                    # a value output: still at most 8 bits in an epilogue
