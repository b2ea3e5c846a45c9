"""Depthwise 3x3 convolution kernels (pf_depthwise.hip: forward + BN statistics, backward-data, backward-filter) against
float32 torch references built from the SAME inputs -- float32 storage to summation-order accuracy, bf16 storage to one
bf16 ulp -- with TensorFlow's 'SAME' padding (front pad floor(total / 2): asymmetric for stride 2 on even sizes), odd and
even sizes, every channel count of MobileNet-v1 (32 ... 1024), strip tails (Wo % 4 != 0).  The second half of the file runs the shapes
whose strip count exceeds the capped grid (the persistent loops every benchmarked launch walks), the channel edges 8 and 2048 and
images smaller than a strip against float64 references, and the 2^31-byte refusal of the entries."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hip():
  from pocketflow_amd import hip as h
  return h


def _same(size, k, stride):
  out = -(-size // stride)
  total = max((out - 1) * stride + k - size, 0)
  return total // 2, total - total // 2, out


def _ref(x, w, stride):
  """float32 reference on logical NCHW tensors, TF 'SAME' padding"""
  ph0, ph1, _ = _same(x.shape[2], 3, stride)
  pw0, pw1, _ = _same(x.shape[3], 3, stride)
  return F.conv2d(F.pad(x, (pw0, pw1, ph0, ph1)), w, stride=stride, groups=x.shape[1])


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('B,H,W,C,stride', [(3, 15, 13, 32, 1), (2, 16, 20, 64, 2), (5, 7, 7, 1024, 1), (2, 14, 14, 512, 2),
                                            (4, 28, 28, 256, 1), (2, 112, 112, 32, 1), (2, 112, 112, 64, 2), (1, 9, 6, 128, 2)])
def test_depthwise_fwd_bwd_wrw_match_torch(hip, monkeypatch, dtype, B, H, W, C, stride):
  assert hip.depthwise_supported(C, 3, stride)
  g = torch.Generator(device='cuda').manual_seed(B + H + W + C + stride)
  x = torch.randn(B, C, H, W, device='cuda', generator=g).to(dtype).contiguous(memory_format=torch.channels_last)
  w = (torch.randn(C, 1, 3, 3, device='cuda', generator=g) * 0.3).to(dtype)
  ph, _, Ho = _same(H, 3, stride)
  pw, _, Wo = _same(W, 3, stride)
  xf = x.float().requires_grad_(True)
  wf = w.float().requires_grad_(True)
  ref = _ref(xf, wf, stride)
  # forward + statistics
  y = torch.full((B, C, Ho, Wo), float('nan'), device='cuda', dtype=dtype).contiguous(memory_format=torch.channels_last)
  G = hip.depthwise_groups(B, Ho, Wo, C)
  partial = torch.full((G, 4, C), float('nan'), device='cuda')
  hip.depthwise_fwd(x, w.reshape(C, 3, 3), y, B, H, W, C, 3, stride, ph, pw, Ho, Wo, partial=partial)
  tol = dict(rtol=1e-5, atol=1e-5) if dtype == torch.float32 else dict(rtol=2 ** -7, atol=1e-3)
  torch.testing.assert_close(y.float(), ref.detach(), **tol)
  yr = y.float().permute(0, 2, 3, 1).reshape(-1, C)
  assert not torch.isnan(partial).any()
  torch.testing.assert_close(partial[:, 0].sum(0), yr.sum(0), rtol=1e-4, atol=1e-2)
  torch.testing.assert_close(partial[:, 1].sum(0), (yr * yr).sum(0), rtol=1e-4, atol=1e-2)
  assert torch.equal(partial[:, 2].min(0).values, yr.min(0).values) and torch.equal(partial[:, 3].max(0).values, yr.max(0).values)
  # backward
  dy = torch.randn(B, C, Ho, Wo, device='cuda', generator=g).to(dtype).contiguous(memory_format=torch.channels_last)
  ref.backward(dy.float())
  dx = torch.full_like(x, float('nan'))
  hip.depthwise_bwd_data(dy, w.reshape(C, 3, 3), dx, B, H, W, C, 3, stride, ph, pw, Ho, Wo)
  torch.testing.assert_close(dx.float(), xf.grad, **(dict(rtol=1e-5, atol=1e-5) if dtype == torch.float32 else dict(rtol=2 ** -7, atol=5e-3)))
  for dw_dtype in (torch.float32, dtype):
    dw = torch.full((C, 3, 3), float('nan'), device='cuda', dtype=dw_dtype)
    slabs = torch.full(((G + 32) * C * 9,), float('nan'), device='cuda')
    hip.depthwise_wrw(dy, x, dw, slabs, B, H, W, C, 3, stride, ph, pw, Ho, Wo)
    scale = float(wf.grad.abs().max())
    err = float((dw.float() - wf.grad.reshape(C, 3, 3)).abs().max())
    assert err <= (1e-4 if dw_dtype == torch.float32 else 2 ** -7) * scale + 1e-5, (err, scale)
  # determinism: fixed-order slab reduction
  dw2 = torch.empty((C, 3, 3), device='cuda', dtype=torch.float32)
  dw3 = torch.empty_like(dw2)
  hip.depthwise_wrw(dy, x, dw2, slabs, B, H, W, C, 3, stride, ph, pw, Ho, Wo)
  hip.depthwise_wrw(dy, x, dw3, slabs, B, H, W, C, 3, stride, ph, pw, Ho, Wo)
  assert torch.equal(dw2, dw3)


def test_depthwise_layer_through_the_executor_matches_torch(hip):
  """graph.DepthwiseConv2D on the in-tree kernels: forward value, statistics left for the BatchNorm, autograd gradients
  (dx through pf_depthwise_bwd_data, dW written straight into the flat gradient buffer)."""
  from pocketflow_amd import graph as G
  gr = G.Graph('model', 'cuda', torch.float32)
  layer = G.DepthwiseConv2D(gr, 'dw', 64, 3, 2)
  gr.finalize(seed=3)
  x = torch.randn(4, 64, 20, 20, device='cuda').contiguous(memory_format=torch.channels_last).requires_grad_(True)
  with gr.as_default():
    y = layer(x, want_stats=True)
  assert y.shape == (4, 64, 10, 10) and hasattr(y, '_pf_stats')
  w = layer.kernel.tensor
  xr = x.detach().clone().requires_grad_(True)
  wr = w.detach().clone().requires_grad_(True)
  ref = _ref(xr, wr, 2)
  torch.testing.assert_close(y, ref, rtol=1e-5, atol=1e-5)
  gy = torch.randn_like(ref)
  y.backward(gy)
  ref.backward(gy)
  torch.testing.assert_close(x.grad, xr.grad, rtol=1e-5, atol=1e-5)
  st = gr.store
  got = st.w_grad[layer.kernel.offset:layer.kernel.offset + layer.kernel.numel].view(64, 1, 3, 3)
  torch.testing.assert_close(got, wr.grad, rtol=1e-4, atol=1e-4)


# ---- the persistent loops, the channel edges, images smaller than a strip ------------------------------------------
# (B, H, W, C, stride) whose strip count exceeds what one pass of the capped grid covers: every lane of k_dw_fwd / k_dw_wrw walks its
# `strip += gridDim.x * SPB` loop more than once (statistics and filter accumulators carried across strips), the last pass ragged.
#   7 x 30 x 98 x 1024 / 1:   5250 strips, 2048 per pass (3 passes), Wo % 4 == 2; backward-data = the flipped forward kernel
#   2 x 61 x 150 x 2048 / 2:  C = 2048 (one strip per workgroup), 1178 strips, 1024 per pass; k_dw_bwd_data makes 18 passes;
#                             front pads 1 (rows) and 0 (columns)
#   4 x 128 x 516 x 32 / 1:   the first layer's channel count (64 strips per workgroup), 66048 strips, 65536 per pass; 264 k terms per
#                             tap of dW, 1024 slabs of 288 values: the two-stage pf_wrw_reduce with 32 slab ranges
LOOP_CASES = [(7, 30, 98, 1024, 1), (2, 61, 150, 2048, 2), (4, 128, 516, 32, 1)]
# C = 8 (256 strips per workgroup), a 1 x 1 image, images narrower than one strip
EDGE_CASES = [(3, 9, 10, 8, 1), (3, 9, 10, 8, 2), (2, 1, 1, 64, 1), (2, 1, 1, 64, 2), (2, 5, 3, 128, 1), (2, 6, 2, 128, 2)]
GRID_CAP = 1024                                           # dw_groups (pf_depthwise.hip)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('B,H,W,C,stride', LOOP_CASES + EDGE_CASES)
def test_depthwise_strip_loops_and_edges_match_float64(hip, dtype, B, H, W, C, stride):
  """The three passes against float64 torch (F.conv2d + autograd) on the same, already rounded operands, so the whole tolerance is
  the kernel's; the statistics against float64 sums of the stored values, within the rounding of the kernel's own float32 chain."""
  assert hip.depthwise_supported(C, 3, stride)
  ph, _, Ho = _same(H, 3, stride)
  pw, _, Wo = _same(W, 3, stride)
  SPB = 2048 // C                                         # strips (pixels in k_dw_bwd_data) per workgroup: DW_T / (C / 8)
  strips = B * Ho * -(-Wo // 4)
  G = hip.depthwise_groups(B, Ho, Wo, C)
  if (B, H, W, C, stride) in LOOP_CASES:
    assert G == GRID_CAP and strips > GRID_CAP * SPB      # forward and backward-filter enter the loop
    if stride == 2:
      assert B * H * W > GRID_CAP * SPB                   # k_dw_bwd_data: one lane per input pixel
    else:
      assert B * H * -(-W // 4) > GRID_CAP * SPB          # the flipped forward kernel over the input geometry
  else:
    assert G == -(-strips // SPB) < GRID_CAP
  passes = -(-strips // (G * SPB))
  g = torch.Generator(device='cuda').manual_seed(B + H + W + C + stride)
  x = torch.randn(B, C, H, W, device='cuda', generator=g).to(dtype).contiguous(memory_format=torch.channels_last)
  w = (torch.randn(C, 1, 3, 3, device='cuda', generator=g) * 0.3).to(dtype)
  xd = x.double().requires_grad_(True)
  wd = w.double().requires_grad_(True)
  ref = _ref(xd, wd, stride)
  # forward + statistics
  y = torch.full((B, C, Ho, Wo), float('nan'), device='cuda', dtype=dtype).contiguous(memory_format=torch.channels_last)
  partial = torch.full((G, 4, C), float('nan'), device='cuda')
  hip.depthwise_fwd(x, w.reshape(C, 3, 3), y, B, H, W, C, 3, stride, ph, pw, Ho, Wo, partial=partial)
  tol = dict(rtol=1e-5, atol=1e-5) if dtype == torch.float32 else dict(rtol=2 ** -7, atol=1e-3)
  torch.testing.assert_close(y.double(), ref.detach(), **tol)
  assert not torch.isnan(partial).any()
  yr = y.permute(0, 2, 3, 1).reshape(-1, C)
  v = yr.double()
  # the longest chain of float32 additions behind one value of partial: 4 pixels per strip and pass in a lane, then the SPB lanes of a
  # channel group through LDS; the G rows are folded here, in float64
  depth = 4 * passes + SPB
  for row, vals in ((0, v), (1, v * v)):
    got, want = partial[:, row].double().sum(0), vals.sum(0)
    bound = 2.0 ** -24 * depth * vals.abs().sum(0)
    worst = float(((got - want).abs() / bound.clamp_min(1e-300)).max())
    print('statistic %d: depth %d, worst error / bound %.3f' % (row, depth, worst))
    assert bool(((got - want).abs() <= bound).all()), (row, depth, worst)
  assert torch.equal(partial[:, 2].min(0).values, yr.float().min(0).values)
  assert torch.equal(partial[:, 3].max(0).values, yr.float().max(0).values)
  # backward
  dy = torch.randn(B, C, Ho, Wo, device='cuda', generator=g).to(dtype).contiguous(memory_format=torch.channels_last)
  ref.backward(dy.double())
  dx = torch.full_like(x, float('nan'))
  hip.depthwise_bwd_data(dy, w.reshape(C, 3, 3), dx, B, H, W, C, 3, stride, ph, pw, Ho, Wo)
  torch.testing.assert_close(dx.double(), xd.grad, **(dict(rtol=1e-5, atol=1e-5) if dtype == torch.float32 else dict(rtol=2 ** -7, atol=5e-3)))
  want_dw = wd.grad.reshape(C, 3, 3)
  scale = float(want_dw.abs().max())
  for dw_dtype in (torch.float32, dtype):
    dw = torch.full((C, 3, 3), float('nan'), device='cuda', dtype=dw_dtype)
    slabs = torch.full(((G + 32) * C * 9,), float('nan'), device='cuda')
    hip.depthwise_wrw(dy, x, dw, slabs, B, H, W, C, 3, stride, ph, pw, Ho, Wo)
    err = float((dw.double() - want_dw).abs().max())
    assert err <= (1e-4 if dw_dtype == torch.float32 else 2 ** -7) * scale + 1e-5, (err, scale)
  # determinism: fixed-order slab reduction
  dw2 = torch.empty((C, 3, 3), device='cuda', dtype=torch.float32)
  dw3 = torch.empty_like(dw2)
  hip.depthwise_wrw(dy, x, dw2, slabs, B, H, W, C, 3, stride, ph, pw, Ho, Wo)
  hip.depthwise_wrw(dy, x, dw3, slabs, B, H, W, C, 3, stride, ph, pw, Ho, Wo)
  assert torch.equal(dw2, dw3)


def test_entries_refuse_tensors_of_2_to_the_31_bytes(hip):
  """The kernels address their inputs through buffer descriptors with 31-bit byte offsets (dw_set_bytes): a tensor of 2^31 bytes or
  more is refused by all three C entries before any launch -- non-zero return, canary-filled outputs untouched.  Nothing of the refused
  calls runs on the device, so the small buffers behind the pointers are never addressed with the large dimensions."""
  from ctypes import c_int, c_void_p
  lib = hip._lib
  S, C = 112, 64                                          # real buffers: one 112 x 112 x 64 float32 image
  G = hip.depthwise_groups(1, S, S, C)
  x = torch.zeros(1, S, S, C, device='cuda')
  w = torch.zeros(C, 3, 3, device='cuda')
  y = torch.full((1, S, S, C), 12345.0, device='cuda')
  dw = torch.full((C, 3, 3), 12345.0, device='cuda')
  partial = torch.full((G, 4, C), 12345.0, device='cuda')
  slabs = torch.full(((G + 32) * C * 9,), 12345.0, device='cuda')
  ptr = lambda t: c_void_p(t.data_ptr())

  def geom(B, H, stride):
    (p, _, Ho) = _same(H, 3, stride)
    return [c_int(v) for v in (B, H, H, C, 3, stride, p, p, Ho, Ho)] + [c_void_p(0)]

  def fwd(dt, B, H, stride):
    return lib.pf_depthwise_fwd(ptr(x), ptr(w), ptr(y), c_int(dt), ptr(partial), *geom(B, H, stride))

  def bwd(dt, B, H, stride):                              # x stands in for dY, y for dX
    return lib.pf_depthwise_bwd_data(ptr(x), ptr(w), ptr(y), c_int(dt), *geom(B, H, stride))

  def wrw(dt, B, H, stride):
    return lib.pf_depthwise_wrw(ptr(x), ptr(x), ptr(dw), c_int(dt), c_int(hip.PF_F32), ptr(slabs), *geom(B, H, stride))

  # 4096 x 112 x 112 x 64 float32: 1.3e10 bytes; 4096 x 64 x 64 x 64 bf16: 2^31 bytes exactly, the first size refused (at stride 2 the
  # gradient read by backward-data is a quarter of it: that entry is called at stride 1 there)
  for dt, B, H in ((hip.PF_F32, 4096, 112), (hip.PF_BF16, 4096, 64)):
    assert B * H * H * C * (4 if dt == hip.PF_F32 else 2) >= 2 ** 31
    for stride in (1, 2):
      assert fwd(dt, B, H, stride) != 0
      assert wrw(dt, B, H, stride) != 0
    assert bwd(dt, B, H, 1) != 0
  assert 4096 * 56 * 56 * C * 4 >= 2 ** 31 and bwd(hip.PF_F32, 4096, 112, 2) != 0   # k_dw_bwd_data's entry: dY is 56 x 56
  torch.cuda.synchronize()
  for t in (y, dw, partial, slabs):
    assert bool((t == 12345.0).all())
  # the same calls at a size the buffers hold are taken: the refusals above were for the size and nothing else
  assert fwd(hip.PF_F32, 1, S, 1) == 0
  assert wrw(hip.PF_F32, 1, S, 1) == 0
  torch.cuda.synchronize()
  assert bool((y == 0.0).all()) and bool((dw == 0.0).all()) and not bool((partial == 12345.0).any())
  y.fill_(12345.0)
  assert bwd(hip.PF_F32, 1, S, 1) == 0
  torch.cuda.synchronize()
  assert bool((y == 0.0).all())
