"""The three-channel 3x3 stems of pf_stem3x.hip (stride 1 | 2, any N % 8 == 0 up to 64) through graph.Conv2D, in exact integer
arithmetic as in test_conv3x3_narrow_gpu.py: x in {-3..3}, the kernel and dy in {-2..2} stored as bf16, so every float32 partial sum is
an integer far below 2**24 (forward: <= 27 * 6; backward-filter: wrw_exact.assert_exact_regime) and the results must EQUAL the float64
reference of torch.nn.functional.conv2d on the CPU, rounded once."""
import pytest
import torch
import torch.nn.functional as F

from wrw_exact import assert_exact_regime, expected, int_inputs, seed_of

pytestmark = pytest.mark.gpu

# stride 1, pad 1: both halo rows are padding | rows no multiple of the 4 / 8 per item | Wd % 16 != 0, a ragged last fragment | the CIFAR map
S1 = [(1, 1, 16), (3, 5, 16), (2, 9, 40), (2, 32, 32)]
# stride 2, 'SAME': odd H, front pad 1 | even size, front pad 0, Wo = 12 | Wo = 20, three strips
S2 = [(2, 7, 16), (2, 8, 24), (1, 33, 40)]
CASES = [(1, 1, N, geom) for N in (8, 16, 24) for geom in S1] + [(2, 'SAME', N, geom) for N in (8, 24, 48) for geom in S2]
# 1025 one-row images: more (image, strip) items than the 1024 workgroups of the forward and the 768 of the backward-filter launch
CASES += [(1, 1, 16, (1025, 1, 16))]


def _same(size, stride):
  out = -(-size // stride)
  total = max((out - 1) * stride + 3 - size, 0)
  return total // 2, total - total // 2


def _layer(N, stride, padding, seed):
  from pocketflow_amd.graph import Conv2D, Graph
  g = Graph('model', 'cuda', torch.bfloat16)
  with g.as_default():
    conv = Conv2D(g, 'c', 3, N, 3, stride, padding=padding, use_bias=False)
  g.finalize(seed=11)
  w, _ = int_inputs(seed, (N, 3, 3, 3), (1,))
  with torch.no_grad():
    conv.kernel.tensor.copy_(w.cuda())
  g.begin_step()
  return g, conv, w


def _reference(x_l, w, dy_l, stride):
  """(y, dW as [N][3][3][3] over KRSC) in float64 ('SAME' at stride 1 is the symmetric pad 1)."""
  (ph, ph1), (pw, pw1) = _same(x_l.shape[1], stride), _same(x_l.shape[2], stride)
  wr = w.double().requires_grad_(True)
  yr = F.conv2d(F.pad(x_l.double().permute(0, 3, 1, 2), (pw, pw1, ph, ph1)), wr, None, stride=stride)
  yr.backward(dy_l.double().permute(0, 3, 1, 2))
  return yr.detach(), wr.grad.permute(0, 2, 3, 1)


@pytest.mark.parametrize('stride,padding,N,geom', CASES)
def test_layer_is_exact_on_the_stem_route(stride, padding, N, geom):
  imgs, H, Wd = geom
  seed = seed_of(stride, N, geom)
  g, conv, w = _layer(N, stride, padding, seed)
  Ho, Wo = -(-H // stride), -(-Wd // stride)
  dy_l, x_l = int_inputs(seed + 1, (imgs, Ho, Wo, N), (imgs, H, Wd, 3))
  x = x_l.cuda().permute(0, 3, 1, 2)
  route = conv._route(x, None, None)
  assert route[0] == 'stem' and route[5].wide and route[5].stride == stride
  assert_exact_regime(imgs * Ho * Wo)
  with g.as_default():
    y = conv(x)
  y.backward(dy_l.cuda().permute(0, 3, 1, 2))
  yr, dwr = _reference(x_l, w, dy_l, stride)
  assert torch.equal(y.detach().cpu(), expected(yr, torch.bfloat16)), 'forward'
  v = conv.kernel
  gw = g.store.w_grad[v.offset:v.offset + v.numel].view(N, 3, 3, 3)
  assert torch.equal(gw.cpu(), expected(dwr, gw.dtype)), 'backward-filter'


def test_what_the_mobilenet_stem_kernels_take_stays_theirs(monkeypatch):
  """N = 16 at stride 2 with Wo % 16 == 0 is pf_stem3.hip's: the same geometry with the new family switched off."""
  import pocketflow_amd.graph as G
  g, conv, _ = _layer(16, 2, 'SAME', 1)
  x = torch.zeros(2, 3, 8, 32, dtype=torch.bfloat16, device='cuda').contiguous(memory_format=torch.channels_last)
  ph, pw, out_hw = conv._geometry(x.shape)
  on = conv._stem_geom(x, ph, pw, out_hw)
  monkeypatch.setattr(G, 'OWN_STEM3X', False)
  assert on is not None and not on.wide and on == conv._stem_geom(x, ph, pw, out_hw)


@pytest.mark.parametrize('stride,N', [(2, 24), (1, 8)])
def test_nothing_behind_the_last_channel_is_read_or_written(stride, N):
  """Every operand is a view into a larger NaN-filled buffer that ends right behind it: the bytes behind channel N - 1 of the last pixel
  of y, behind W[N - 1], behind the image, behind dy and behind dW stay NaN, and no NaN reaches a result."""
  from pocketflow_amd import hip
  imgs, H, Wd = 2, 7, 16
  seed = seed_of('nan', stride, N)
  Ho, Wo = -(-H // stride), -(-Wd // stride)
  w_l, x_l = int_inputs(seed, (N, 3, 3, 3), (imgs, H, Wd, 3))
  dy_l, _ = int_inputs(seed + 1, (imgs, Ho, Wo, N), (1,))
  yr, dwr = _reference(x_l, w_l.permute(0, 3, 1, 2), dy_l, stride)
  dims = (imgs, H, Wd, N, stride, _same(H, stride)[0], _same(Wd, stride)[0], Ho, Wo)

  def view(src, dtype=torch.bfloat16):
    buf = torch.full((src.numel() + 64,), float('nan'), dtype=dtype, device='cuda')
    buf[:src.numel()] = src.reshape(-1).to(dtype)
    return buf, buf[:src.numel()].view(src.shape)

  (xb, x), (wb, w), (dyb, dy) = (view(t) for t in (x_l, w_l, dy_l))
  nan = float('nan')
  (yb, y), (dwb, dw) = view(torch.full((imgs, Ho, Wo, N), nan)), view(torch.full((N, 3, 3, 3), nan), torch.float32)
  ws = torch.full((hip.wrw_workspace_floats(hip.conv_stem3x_wrw_slabs(*dims), N * 27),), nan, device='cuda')
  hip.conv_stem3x_fwd(x, w, y, *dims)
  hip.conv_stem3x_wrw(dy, x, dw, ws, *dims)
  assert torch.equal(y.cpu(), expected(yr.permute(0, 2, 3, 1), torch.bfloat16))
  assert torch.equal(dw.cpu(), expected(dwr, torch.float32))
  for buf, t in ((xb, x), (wb, w), (dyb, dy), (yb, y), (dwb, dw)):
    assert torch.isnan(buf[t.numel():]).all()


def test_resnet20_step_runs_its_stem_on_the_route(tmp_path, monkeypatch):
  """ResNet-20 @ CIFAR-10, one training step at batch 4: the 3 -> 16 stem is on the stem route, and on pf_convg.hip with the switch off."""
  import pocketflow_amd.graph as G
  from pocketflow_amd.flags import FLAGS
  from pocketflow_amd.nets.resnet_at_cifar10 import ModelHelper
  from pocketflow_amd.learners.full_precision.learner import FullPrecLearner
  import pocketflow_amd.datasets.abstract_dataset  # noqa: F401  (synthetic_pool)
  for k, v in dict(save_path=str(tmp_path / 'models' / 'model.ckpt'), save_path_eval=str(tmp_path / 'models_eval' / 'model.ckpt'),
                   synthetic_pool=2, batch_size=4, resnet_size=20, nb_classes=10, compute_dtype='bfloat16').items():
    setattr(FLAGS, k, v)
  learner = FullPrecLearner(None, ModelHelper())
  routes = []
  route = G.Conv2D._route

  def spy(self, x, residual, out_bn):
    r = route(self, x, residual, out_bn)
    if self.kernel.ref_shape[2] == 3:
      routes.append(r[0])
    return r
  monkeypatch.setattr(G.Conv2D, '_route', spy)
  for own, want in ((True, 'stem'), (False, 'general')):
    monkeypatch.setattr(G, 'OWN_STEM3X', own)
    del routes[:]
    loss = learner.train_step()[1]
    assert torch.isfinite(loss.detach().float()).all()
    assert routes and set(routes) == {want}
