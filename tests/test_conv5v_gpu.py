"""The biased 5x5 'VALID' convolutions of pf_conv5v.hip (LeNet @ CIFAR-10) through graph.Conv2D, in exact integer arithmetic: operands
are small integers stored as bf16 (x and the bias in {-3..3}, the kernel and dy in {-2..2}), so every float32 partial sum of every
pass is an integer far below 2**24 (forward: <= 25 * 32 * 6 + 3; backward-data: <= 25 * 64 * 4; backward-filter and the bias gradient:
wrw_exact.assert_exact_regime) and the kernels' results must EQUAL the float64 reference of torch.nn.functional.conv2d on the CPU,
rounded once to the output's dtype."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from wrw_exact import assert_exact_regime, expected, int_inputs, seed_of

pytestmark = pytest.mark.gpu

# (imgs, H, Wd): one output pixel, the fragment 15 / 16 empty | rows no multiple of the tile height, Wo = 10 straddles fragments and
# rows | LeNet's conv2 | odd width, Wo = 17 is one pixel into a second fragment | more tiles than any launch has workgroups
GEOMS = [(1, 5, 5), (3, 9, 14), (2, 14, 14), (2, 11, 21), (1030, 5, 5)]
CASES = [(C, N, geom, bias) for (C, N), geom, bias in itertools.product(((3, 32), (32, 64), (32, 32)), GEOMS, (True, False))]
CASES += [(3, 32, (2, 32, 32), True), (3, 32, (2, 32, 32), False)]                    # LeNet's conv1


def _layer(C, N, seed, bias=True, stride=1, padding='VALID'):
  """(graph, Conv2D, kernel, bias) with an integer kernel in {-2..2} and an integer bias in {-3..3}."""
  from pocketflow_amd.graph import Conv2D, Graph
  g = Graph('model', 'cuda', torch.bfloat16)
  with g.as_default():
    conv = Conv2D(g, 'c', C, N, 5, stride, padding=padding, use_bias=bias)
  g.finalize(seed=11)
  w, b = int_inputs(seed, (N, C, 5, 5), (N,))
  with torch.no_grad():
    conv.kernel.tensor.copy_(w.cuda())
    if bias:
      conv.bias.tensor.copy_(b.cuda())
  g.begin_step()                                 # (the backward-data copy of the kernels is refreshed from the new values)
  return g, conv, w, (b if bias else None)


def _nchw(t_nhwc):
  """NHWC memory as the logical-NCHW tensor the layers take."""
  return t_nhwc.cuda().permute(0, 3, 1, 2)


@pytest.mark.parametrize('C,N,geom,bias', CASES)
def test_layer_is_exact_on_its_route(C, N, geom, bias):
  imgs, H, Wd = geom
  seed = seed_of(C, N, geom, bias)
  g, conv, w, b = _layer(C, N, seed, bias)
  dy_l, x_l = int_inputs(seed + 1, (imgs, H - 4, Wd - 4, N), (imgs, H, Wd, C))
  x = _nchw(x_l).requires_grad_(C != 3)          # (an image asks for no gradient)
  assert conv._route(x, None, None)[0] == 'conv5v'
  assert_exact_regime(imgs * (H - 4) * (Wd - 4))
  with g.as_default():
    y = conv(x)
  y.backward(_nchw(dy_l))
  xr = x_l.double().permute(0, 3, 1, 2).requires_grad_(True)
  wr = w.double().requires_grad_(True)
  br = b.double().requires_grad_(True) if bias else None
  yr = F.conv2d(xr, wr, br)
  yr.backward(dy_l.double().permute(0, 3, 1, 2))
  assert torch.equal(y.detach().cpu(), expected(yr.detach(), torch.bfloat16)), 'forward'
  if C != 3:
    assert torch.equal(x.grad.cpu(), expected(xr.grad, torch.bfloat16)), 'backward-data'
  v = conv.kernel
  gw = g.store.w_grad[v.offset:v.offset + v.numel].view(N, 5, 5, C)
  assert torch.equal(gw.cpu(), expected(wr.grad.permute(0, 2, 3, 1), gw.dtype)), 'backward-filter'
  if bias:
    assert torch.equal(conv.bias.tensor.grad.cpu(), expected(br.grad, torch.float32)), 'bias gradient'


@pytest.mark.parametrize('iy,ix', [(4, 6), (8, 13)])
def test_inf_pixel_reaches_the_outputs_whose_window_holds_it_and_no_other(iy, ix):
  """C = 3: the fourth k-step has tap 24 alone, and a fragment's lanes behind the tile's end read its last pixel again (the image's
  last pixel, (8, 13), is in that window).  Neither the zero tail nor those lanes reach another stored output."""
  imgs, H, Wd = 2, 9, 14
  seed = seed_of('inf', iy, ix)
  g, conv, w, b = _layer(3, 32, seed)
  _, x_l = int_inputs(seed + 1, (1,), (imgs, H, Wd, 3))
  x_l[0, iy, ix, :] = float('inf')
  with torch.no_grad(), g.as_default():
    y = conv(_nchw(x_l)).cpu()
  clean = x_l.clone()
  clean[0, iy, ix, :] = 0
  ref = expected(F.conv2d(clean.double().permute(0, 3, 1, 2), w.double(), b.double()), torch.bfloat16)
  away = torch.ones_like(ref, dtype=torch.bool)
  away[0, :, max(iy - 4, 0):iy + 1, max(ix - 4, 0):ix + 1] = False
  assert torch.isfinite(y[away]).all() and torch.equal(y[away], ref[away])
  assert not torch.isfinite(y[~away]).any()


@pytest.mark.parametrize('C,geom,stride,padding,grad,route', [
    (32, (2, 14, 14), 2, 'VALID', True, 'library'), (32, (2, 14, 14), 1, 2, True, 'library'),
    (3, (2, 9, 80), 1, 'VALID', False, 'general'), (3, (2, 32, 32), 1, 'VALID', True, 'general')])
def test_what_the_kernels_refuse_keeps_its_route(C, geom, stride, padding, grad, route):
  imgs, H, Wd = geom
  g, conv, _, _ = _layer(C, 32, 1, True, stride, padding)
  x = _nchw(torch.zeros(imgs, H, Wd, C, dtype=torch.bfloat16)).requires_grad_(grad)
  assert conv._route(x, None, None)[0] == route


def test_lenet_step_runs_both_convolutions_on_the_route(tmp_path, monkeypatch):
  """LeNet @ CIFAR-10, one bf16 training step at batch 4: conv1 and conv2 on pf_conv5v.hip; with the switch off neither."""
  import pocketflow_amd.graph as G
  from pocketflow_amd import profiling
  from pocketflow_amd.flags import FLAGS
  from pocketflow_amd.nets.lenet_at_cifar10 import ModelHelper
  from pocketflow_amd.learners.full_precision.learner import FullPrecLearner
  import pocketflow_amd.datasets.abstract_dataset  # noqa: F401  (synthetic_pool)
  for k, v in dict(save_path=str(tmp_path / 'models' / 'model.ckpt'), save_path_eval=str(tmp_path / 'models_eval' / 'model.ckpt'),
                   synthetic_pool=2, batch_size=4, nb_classes=10, compute_dtype='bfloat16').items():
    setattr(FLAGS, k, v)
  learner = FullPrecLearner(None, ModelHelper())
  names = ('conv5v_fwd', 'conv5v_bwd_data', 'conv5v_wrw')
  try:
    for own, counts in ((True, (2, 1, 2)), (False, (0, 0, 0))):
      monkeypatch.setattr(G, 'OWN_CONV5V', own)
      for n in names:
        profiling.enable(n)
      loss = learner.train_step()[1]
      assert torch.isfinite(loss.detach().float()).all()
      assert tuple(profiling.count(n) for n in names) == counts
  finally:
    profiling.disable_all()
