"""pf_depthwise.hip at channel counts whose groups of 8 do not divide the 256-lane workgroup (C = 24 ... 2040, the widths of
MobileNet-v1 0.75 and of MobileNet-v2 among them): SPB = 256 // (C / 8) strips per workgroup, the left-over lanes idle.  The body and the
bars are those of tests/test_depthwise_gpu.py::test_depthwise_strip_loops_and_edges_match_float64: float64 torch on the same rounded
operands, the statistics within the rounding of the kernel's own float32 chain, exact min / max, bit-equal repeats.  A left-over lane
that worked would redo the first strip of the next workgroup: the statistics would count it twice and miss their bound by orders."""
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
  """reference on logical NCHW tensors, TF 'SAME' padding"""
  ph0, ph1, _ = _same(x.shape[2], 3, stride)
  pw0, pw1, _ = _same(x.shape[3], 3, stride)
  return F.conv2d(F.pad(x, (pw0, pw1, ph0, ph1)), w, stride=stride, groups=x.shape[1])


# lanes in use of 256: 255 (C = 24), 252 (48, 96, 144), 240 (384, 960), 192 (768), 129 (1032), 255 (2040); odd and even sizes, strip tails,
# an image narrower than a strip, one strip per workgroup (C > 1024)
SMALL_CASES = [(3, 15, 13, 24, 1), (2, 16, 20, 48, 2), (2, 9, 6, 96, 2), (2, 14, 14, 144, 1), (2, 14, 14, 384, 2), (3, 7, 7, 768, 1),
               (2, 7, 7, 960, 1), (1, 5, 3, 1032, 2), (1, 6, 6, 2040, 1)]
# strip counts beyond one pass of the capped grid: 22016 strips against 1024 x 21, 2356 against 1024 x 2
LOOP_CASES = [(4, 64, 344, 96, 1), (4, 61, 150, 768, 2)]
GRID_CAP = 1024                                           # dw_groups (pf_depthwise.hip)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('B,H,W,C,stride', SMALL_CASES + LOOP_CASES)
def test_depthwise_odd_channel_counts_match_float64(hip, dtype, B, H, W, C, stride):
  assert hip.depthwise_supported(C, 3, stride)
  assert 256 % (C // 8) != 0                              # every case leaves lanes over
  ph, _, Ho = _same(H, 3, stride)
  pw, _, Wo = _same(W, 3, stride)
  SPB = 256 // (C // 8)                                   # strips (pixels in k_dw_bwd_data) per workgroup, rounded down
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
  # determinism: fixed-order slab reduction; the forward pass and its statistics repeat bit for bit as well
  dw2 = torch.empty((C, 3, 3), device='cuda', dtype=torch.float32)
  dw3 = torch.empty_like(dw2)
  hip.depthwise_wrw(dy, x, dw2, slabs, B, H, W, C, 3, stride, ph, pw, Ho, Wo)
  hip.depthwise_wrw(dy, x, dw3, slabs, B, H, W, C, 3, stride, ph, pw, Ho, Wo)
  assert torch.equal(dw2, dw3)
  y2 = torch.full_like(y, float('nan'))
  partial2 = torch.full_like(partial, float('nan'))
  hip.depthwise_fwd(x, w.reshape(C, 3, 3), y2, B, H, W, C, 3, stride, ph, pw, Ho, Wo, partial=partial2)
  assert torch.equal(y2, y) and torch.equal(partial2, partial)


def test_depthwise_layer_of_96_channels_never_enters_the_library(hip, monkeypatch):
  """graph.DepthwiseConv2D at 96 channels, stride 2, through the executor (as test_depthwise_layer_through_the_executor_matches_torch):
  forward value, statistics left for the BatchNorm, autograd gradients -- all on pf_depthwise.hip."""
  from pocketflow_amd import graph as G
  entered = []
  library = G.DepthwiseConv2D._call_library
  monkeypatch.setattr(G.DepthwiseConv2D, '_call_library', lambda self, r, want_stats: (entered.append(self.kernel.name), library(self, r, want_stats))[1])
  gr = G.Graph('model', 'cuda', torch.float32)
  layer = G.DepthwiseConv2D(gr, 'dw', 96, 3, 2)
  gr.finalize(seed=3)
  x = torch.randn(4, 96, 20, 20, device='cuda').contiguous(memory_format=torch.channels_last).requires_grad_(True)
  with gr.as_default():
    y = layer(x, want_stats=True)
  assert y.shape == (4, 96, 10, 10) and hasattr(y, '_pf_stats')
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
  got = st.w_grad[layer.kernel.offset:layer.kernel.offset + layer.kernel.numel].view(96, 1, 3, 3)
  torch.testing.assert_close(got, wr.grad, rtol=1e-4, atol=1e-4)
  assert entered == []
