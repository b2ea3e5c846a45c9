"""The narrow 3x3 convolutions (pf_conv3x3_narrow.hip) through graph.Conv2D, in exact integer arithmetic: operands are small integers
stored as bf16 (x and the residual in {-3..3}, the kernel and dy in {-2..2}), so every float32 partial sum of every pass is an
integer far below 2**24 (forward: <= 9 * 32 * 6 + 3; backward-filter: wrw_exact.assert_exact_regime) and the kernels' results must
EQUAL the float64 reference of torch.nn.functional.conv2d on the CPU, rounded once to the output's dtype."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from wrw_exact import assert_exact_regime, expected, int_inputs, seed_of

pytestmark = pytest.mark.gpu

# (imgs, H, Wd): rows not a multiple of any tile height, one fragment per row | both halo rows are padding | three fragments per
# row, not a power of two | the benchmarked map
GEOMS = [(3, 5, 16), (1, 1, 16), (2, 7, 48), (2, 32, 32)]
CASES = [(C, N, geom, 1, res, 'conv3x3n') for (C, N), geom, res in itertools.product(itertools.product((16, 32), repeat=2), GEOMS, (False, True))]
# what the kernels refuse keeps the route it had
CASES += [(16, 32, (2, 32, 32), 2, False, 'im2col'), (48, 16, (2, 32, 32), 1, False, 'im2col'), (16, 16, (2, 32, 20), 1, False, 'im2col')]


def _layer(C, N, stride, seed):
  """(graph, Conv2D) with an integer kernel in {-2..2}."""
  from pocketflow_amd.graph import Conv2D, Graph
  g = Graph('model', 'cuda', torch.bfloat16)
  with g.as_default():
    conv = Conv2D(g, 'c', C, N, 3, stride, padding=1, use_bias=False)
  g.finalize(seed=11)
  w, _ = int_inputs(seed, (N, C, 3, 3), (1,))
  with torch.no_grad():
    conv.kernel.tensor.copy_(w.cuda())
  g.begin_step()                                 # (the backward-data copy of the kernels is refreshed from the new values)
  return g, conv, w


def _nchw(t_nhwc):
  """NHWC memory as the logical-NCHW tensor the layers take."""
  return t_nhwc.cuda().permute(0, 3, 1, 2)


@pytest.mark.parametrize('C,N,geom,stride,res,route', CASES)
def test_layer_is_exact_on_its_route(C, N, geom, stride, res, route):
  imgs, H, Wd = geom
  seed = seed_of(C, N, geom, stride, res)
  g, conv, w = _layer(C, N, stride, seed)
  dy_l, x_l = int_inputs(seed + 1, (imgs, H, Wd, N), (imgs, H, Wd, C))
  _, r_l = int_inputs(seed + 2, (1,), (imgs, H, Wd, N))
  x = _nchw(x_l).requires_grad_(True)
  r = _nchw(r_l).requires_grad_(True) if res else None
  assert conv._route(x, r, None)[0] == route
  if route != 'conv3x3n':
    return
  assert_exact_regime(imgs * H * Wd)
  with g.as_default():
    y = conv(x, residual=r)
  y.backward(_nchw(dy_l))
  xr = x_l.double().permute(0, 3, 1, 2).requires_grad_(True)
  wr = w.double().requires_grad_(True)
  yr = F.conv2d(xr, wr, None, stride=1, padding=1)
  if res:
    yr = yr + r_l.double().permute(0, 3, 1, 2)
  yr.backward(dy_l.double().permute(0, 3, 1, 2))
  assert torch.equal(y.detach().cpu(), expected(yr.detach(), torch.bfloat16)), 'forward'
  assert torch.equal(x.grad.cpu(), expected(xr.grad, torch.bfloat16)), 'backward-data'
  v = conv.kernel
  gw = g.store.w_grad[v.offset:v.offset + v.numel].view(N, 3, 3, C)
  assert torch.equal(gw.cpu(), expected(wr.grad.permute(0, 2, 3, 1), gw.dtype)), 'backward-filter'
  if res:
    assert torch.equal(r.grad.cpu(), dy_l.permute(0, 3, 1, 2)), "the residual's gradient is dy"


@pytest.mark.parametrize('N', [16, 32])
def test_fifth_k_step_multiplies_zeros_not_a_neighbouring_pixel(N):
  """C = 16: the upper half of the fifth k-step has no tap.  An Inf pixel reaches the outputs whose window holds it and no other."""
  imgs, H, Wd = 3, 5, 16
  seed = seed_of('inf', N)
  g, conv, w = _layer(16, N, 1, seed)
  _, x_l = int_inputs(seed + 1, (1,), (imgs, H, Wd, 16))
  x_l[0, 2, 5, :] = float('inf')
  with torch.no_grad(), g.as_default():
    y = conv(_nchw(x_l)).cpu()
  clean = x_l.clone()
  clean[0, 2, 5, :] = 0
  ref = expected(F.conv2d(clean.double().permute(0, 3, 1, 2), w.double(), None, padding=1), torch.bfloat16)
  away = torch.ones_like(ref, dtype=torch.bool)
  away[0, :, 1:4, 4:7] = False
  assert torch.isfinite(y[away]).all() and torch.equal(y[away], ref[away])
  assert not torch.isfinite(y[~away]).any()


def test_resnet20_step_runs_its_narrow_layers_on_the_route(tmp_path, monkeypatch):
  """ResNet-20 @ CIFAR-10, one training step at batch 4: of its 13 few-channel 3x3 layers, 11 are 16 -> 16 at 32 x 32 or 32 -> 32 at
  16 x 16 (pf_conv3x3_narrow.hip) and 2 are strided (im2col); with the switch off all 13 are im2col."""
  import pocketflow_amd.graph as G
  from pocketflow_amd import profiling
  from pocketflow_amd.flags import FLAGS
  from pocketflow_amd.nets.resnet_at_cifar10 import ModelHelper
  from pocketflow_amd.learners.full_precision.learner import FullPrecLearner
  import pocketflow_amd.datasets.abstract_dataset  # noqa: F401  (synthetic_pool)
  for k, v in dict(save_path=str(tmp_path / 'models' / 'model.ckpt'), save_path_eval=str(tmp_path / 'models_eval' / 'model.ckpt'),
                   synthetic_pool=2, batch_size=4, resnet_size=20, nb_classes=10, compute_dtype='bfloat16').items():
    setattr(FLAGS, k, v)
  learner = FullPrecLearner(None, ModelHelper())
  names = ('conv3x3n_fwd', 'conv_im2col_fwd')
  try:
    for own, counts in ((True, (11, 2)), (False, (0, 13))):
      monkeypatch.setattr(G, 'OWN_CONV3X3_NARROW', own)
      for n in names:
        profiling.enable(n)
      loss = learner.train_step()[1]
      assert torch.isfinite(loss.detach().float()).all()
      assert tuple(profiling.count(n) for n in names) == counts
  finally:
    profiling.disable_all()
