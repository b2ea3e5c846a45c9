"""pf_depthwise_fwd_act / pf_depthwise_wrw_act: the depthwise kernels with the producer BatchNorm's normalise / activation / fake-quant
as their prologue, held BIT FOR BIT to the two launches they replace -- pf_bn_act_quant_apply followed by pf_depthwise_fwd (output AND
statistics partials) / pf_depthwise_wrw.  A tap inside the image is the value the apply pass would have stored, rounded to the storage
type; a tap outside contributes 0.  Every channel's shift is strictly positive here, so a prologue applied to the padding would put
act(shift) != 0 into every border output and filter gradient.

Scale / shift come from pf_bn_finalize in inference mode over moving statistics chosen for that (mean < 0, gamma > 0, beta > 0), which
also leaves the quantiser's range of THIS tensor in the slot: the route of the quantising learners' calibration pass."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

GRID_CAP = 1024                                           # dw_groups (pf_depthwise.hip)
# smaller than a strip, odd, W not a multiple of 4, even and odd extents under stride 2 (asymmetric 'SAME' pads on the even ones)
SIZES = [(1, 1), (3, 5), (7, 7), (9, 6), (6, 10)]


@pytest.fixture(scope='module')
def hip():
  from pocketflow_amd import hip as h
  return h


def _same(size, k, stride):
  out = -(-size // stride)
  total = max((out - 1) * stride + k - size, 0)
  return total // 2, out


def _operands(hip, B, H, W, C, stride, dtype, act, bits, seed):
  """x (raw), w, dy, scale_shift (shift > 0), slot (None without a quantiser) and the geometry."""
  from pocketflow_amd.graph import _bn_blocks
  g = torch.Generator(device='cuda').manual_seed(seed)
  x = (torch.randn(B, C, H, W, device='cuda', generator=g) * 2).to(dtype).contiguous(memory_format=torch.channels_last)
  w = (torch.randn(C, 3, 3, device='cuda', generator=g) * 0.3).to(dtype)
  ph, Ho = _same(H, 3, stride)
  pw, Wo = _same(W, 3, stride)
  dy = torch.randn(B, C, Ho, Wo, device='cuda', generator=g).to(dtype).contiguous(memory_format=torch.channels_last)
  gamma = 0.5 + torch.rand(C, device='cuda', generator=g)
  beta = 0.25 + torch.rand(C, device='cuda', generator=g)
  mm = -0.1 - torch.rand(C, device='cuda', generator=g)
  mv = 0.5 + torch.rand(C, device='cuda', generator=g)
  rows = B * H * W
  nblk = _bn_blocks(rows, C)
  partial = torch.empty(nblk * 4 * C, device='cuda')
  ss = torch.empty((2, C), device='cuda')
  mi = torch.empty((2, C), device='cuda')
  slot = None
  if bits is not None:
    slots = torch.empty((1, 2), dtype=torch.int32, device='cuda')
    hip.minmax_slots_init(slots)
    slot = slots[0]
  hip.bn_stats(x, rows, C, partial, nblk)
  hip.bn_finalize(partial, nblk, rows, C, x, gamma, beta, mm, mv, 0.997, 1e-3, False, act, ss, mi, slot)
  assert bool((ss[1] > 0).all())                          # act(shift) != 0: padding that went through the prologue would show
  return x, w, dy, ss, slot, (ph, pw, Ho, Wo)


def _check(hip, B, H, W, C, stride, dtype, act, bits, seed=0):
  x, w, dy, ss, slot, (ph, pw, Ho, Wo) = _operands(hip, B, H, W, C, stride, dtype, act, bits, seed)
  rows = B * H * W
  quant = bits is not None
  G = hip.depthwise_groups(B, Ho, Wo, C)
  dims = (B, H, W, C, 3, stride, ph, pw, Ho, Wo)
  # the two launches the fused forward replaces
  q = torch.empty_like(x)
  hip.bn_act_quant_apply(x, q, rows, C, ss, act, slot, bits if quant else 8, quant)
  y_ref = torch.full((B, C, Ho, Wo), float('nan'), device='cuda', dtype=dtype).contiguous(memory_format=torch.channels_last)
  p_ref = torch.full((G, 4, C), float('nan'), device='cuda')
  hip.depthwise_fwd(q, w, y_ref, *dims, partial=p_ref)
  y = torch.full_like(y_ref, float('nan'))
  p = torch.full_like(p_ref, float('nan'))
  hip.depthwise_fwd_act(x, ss, act, slot, bits if quant else 8, w, y, *dims, partial=p)
  what = (B, H, W, C, stride, dtype, act, bits)
  assert not torch.isnan(y_ref).any() and not torch.isnan(p_ref).any(), what
  assert torch.equal(y, y_ref), ('forward', what, float((y.float() - y_ref.float()).abs().max()))
  assert torch.equal(p, p_ref), ('statistics', what)
  y2 = torch.full_like(y_ref, float('nan'))
  hip.depthwise_fwd_act(x, ss, act, slot, bits if quant else 8, w, y2, *dims)      # without statistics; run to run
  assert torch.equal(y2, y_ref), ('forward, no statistics', what)
  # backward-filter
  for dw_dtype in (torch.float32, dtype):
    slabs = torch.full(((G + 32) * C * 9,), float('nan'), device='cuda')
    dw_ref = torch.full((C, 3, 3), float('nan'), device='cuda', dtype=dw_dtype)
    hip.depthwise_wrw(dy, q, dw_ref, slabs, *dims)
    dw = torch.full_like(dw_ref, float('nan'))
    slabs2 = torch.full_like(slabs, float('nan'))
    hip.depthwise_wrw_act(dy, x, ss, act, slot, bits if quant else 8, dw, slabs2, *dims)
    assert not torch.isnan(dw_ref).any(), what
    assert torch.equal(dw, dw_ref), ('backward-filter', dw_dtype, what, float((dw.float() - dw_ref.float()).abs().max()))
  dw3 = torch.full_like(dw, float('nan'))
  hip.depthwise_wrw_act(dy, x, ss, act, slot, bits if quant else 8, dw3, slabs2, *dims)
  assert torch.equal(dw3, dw), ('backward-filter, run to run', what)
  return G


# C = 8: one channel group; 24 and 144: GEN (left-over lanes idle); 256: non-GEN
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('C', [8, 24, 144, 256])
def test_fused_prologue_equals_apply_then_depthwise_bit_for_bit(hip, C, dtype):
  seed = 0
  for H, W in SIZES:
    for stride in (1, 2):
      for act in ('Relu6', None):
        for bits in (None, 8, 4):
          seed += 1
          _check(hip, 2, H, W, C, stride, dtype, act, bits, seed)


# strip counts beyond one pass of the capped grid (pf_depthwise_groups): the grid-stride loop makes a second trip
LOOP_CASES = [(2, 64, 260, 256, 1), (2, 64, 452, 144, 1), (2, 127, 520, 256, 2)]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('B,H,W,C,stride', LOOP_CASES)
def test_fused_prologue_in_the_grid_stride_loop(hip, dtype, B, H, W, C, stride):
  _, Ho = _same(H, 3, stride)
  _, Wo = _same(W, 3, stride)
  strips = B * Ho * -(-Wo // 4)
  assert strips > GRID_CAP * (256 // (C // 8))
  G = _check(hip, B, H, W, C, stride, dtype, 'Relu6', 8 if dtype == torch.bfloat16 else None, seed=C + stride)
  assert G == GRID_CAP


def test_fused_entries_refuse_what_they_cannot_run(hip):
  """Null pointers, a misaligned tensor, unsupported C / k / stride, an unknown activation or ReLU (only ReLU6 and none are built), a quantiser without a sensible width:
  non-zero, and nothing written."""
  B, H, W, C = 2, 6, 6, 16
  x, w, dy, ss, slot, (ph, pw, Ho, Wo) = _operands(hip, B, H, W, C, 1, torch.float32, 'Relu6', 8, 5)
  y = torch.full((B, C, Ho, Wo), float('nan'), device='cuda').contiguous(memory_format=torch.channels_last)
  G = hip.depthwise_groups(B, Ho, Wo, C)
  slabs = torch.full(((G + 32) * C * 9,), float('nan'), device='cuda')
  dw = torch.full((C, 3, 3), float('nan'), device='cuda')
  flat = torch.zeros(x.numel() + 4, device='cuda')
  off = flat[1:1 + x.numel()]                               # 4 bytes off a 16-byte boundary
  assert off.data_ptr() % 16 != 0
  I, P = ctypes.c_int, hip._ptr

  def fwd(X=x, SS=ss, act=2, SLOT=slot, bits=8, Wt=w, Y=y, C_=C, k=3, stride=1):
    return hip._lib.pf_depthwise_fwd_act(P(X), P(SS), I(act), P(SLOT), I(bits), P(Wt), P(Y), I(0), P(None), I(B), I(H), I(W), I(C_), I(k),
                                         I(stride), I(ph), I(pw), I(Ho), I(Wo), hip._stream())

  def wrw(DY=dy, X=x, SS=ss, act=2, SLOT=slot, bits=8, DW=dw, SL=slabs, C_=C, k=3, stride=1):
    return hip._lib.pf_depthwise_wrw_act(P(DY), P(X), P(SS), I(act), P(SLOT), I(bits), P(DW), I(0), I(0), P(SL), I(B), I(H), I(W), I(C_),
                                         I(k), I(stride), I(ph), I(pw), I(Ho), I(Wo), hip._stream())
  for kw in (dict(X=None), dict(SS=None), dict(Wt=None), dict(Y=None), dict(X=off), dict(Y=off), dict(C_=12), dict(C_=4), dict(C_=2056),
             dict(k=5), dict(stride=3), dict(act=7), dict(act=1), dict(bits=0), dict(bits=33)):
    assert fwd(**kw) != 0, kw
  for kw in (dict(DY=None), dict(X=None), dict(SS=None), dict(DW=None), dict(SL=None), dict(X=off), dict(DY=off), dict(C_=12), dict(k=1),
             dict(stride=0), dict(act=-1), dict(act=1), dict(bits=0)):
    assert wrw(**kw) != 0, kw
  torch.cuda.synchronize()
  assert bool(torch.isnan(y).all()) and bool(torch.isnan(dw).all()) and bool(torch.isnan(slabs).all())
  assert fwd() == 0 and wrw() == 0                          # the same call sites with nothing wrong
  torch.cuda.synchronize()
  assert not torch.isnan(y).any() and not torch.isnan(dw).any()
