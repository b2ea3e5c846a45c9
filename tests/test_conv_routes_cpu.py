"""Which route ONE call of a convolution layer takes (graph.Conv2D, DepthwiseConv2D, Dense) and what it counts on its producer:
tests/test_fused_plumbing_cpu.py::test_step_launch_census pins the launches of whole networks, this file pins single layer calls --
the multiset of emulated entry points one forward + backward calls, and `n_consumers` of the BnSums record of the training-mode
BatchNormAct in front of the layer ("a consumer that fuses the BN-backward sums counts once, any other twice": what lets ONE
backward-data kernel skip a BN statistics pass).  The HIP entry points are the float32 doubles of tests/fake_hip.py.

Every case runs a batch of 2 over at most 144 pixels: 8 x 8 maps, and 4 x 32 images for the two stem kernels, whose doubles -- like
the kernels -- take no image narrower than 32 pixels."""
import pytest
import torch
import torch.nn.functional as F

from fake_hip import FakeHip  # noqa: F401  (tests/fake_hip.py)
from test_proj_join_cpu import _Counting, _JoinHip


class _Spy(object):
  """Tells the backward-data launches of the 1x1 route apart: `conv1x1_res` = a plain launch with a residual operand (the second of
  two joined consumers), `conv1x1_ymap` (test_proj_join_cpu._Counting) = the row scatter of a strided layer, whose target must
  arrive zero-filled; and keeps the tensor the MobileNet stem kernel was handed."""
  stem3_input = None
  ymap_into_zeros = None

  def conv1x1_fwd(self, X, W, Y, M, N, K, R=None, scale_shift=None, **kw):
    if scale_shift is None and R is not None:
      self._n('conv1x1_res')
    if kw.get('ymap'):
      self.ymap_into_zeros = not bool(Y.any())
    return super(_Spy, self).conv1x1_fwd(X, W, Y, M, N, K, R=R, scale_shift=scale_shift, **kw)

  def conv_stem3_fwd(self, X, *args):
    self.stem3_input = X
    return super(_Spy, self).conv_stem3_fwd(X, *args)


class _Hip(_Spy, _Counting):
  """A library WITHOUT the projection join entry."""


class _HipJoin(_Spy, _JoinHip):
  """... and one with it."""


def _graph(monkeypatch, fake=None, **switches):
  from pocketflow_amd import graph as G
  fake = fake if fake is not None else _Hip()
  monkeypatch.setattr(G, 'hip', fake)
  monkeypatch.setattr(G, 'fusable_tensor', lambda t: True)
  monkeypatch.setattr(G, 'DEPTHWISE_ANY_DEVICE', True)
  for name, value in switches.items():
    assert hasattr(G, name), name
    monkeypatch.setattr(G, name, value)
  g = G.Graph('model', 'cpu', torch.float32)
  g.begin_step = lambda: None
  return G, g, fake


def _ready(g, fake):
  g.finalize(seed=3, requires_grad=True)
  fake.minmax_slots_init(g.act_slots)
  fake.calls.clear()


def _image(c, h=8, w=8, seed=0, grad=True):
  torch.manual_seed(seed)
  x = torch.randn(2, c, h, w).contiguous(memory_format=torch.channels_last)
  return x.requires_grad_() if grad else x


def _bn(G, g, c, lazy, name='bn', act='Relu'):
  return G.BatchNormAct(g, name, c, act, 0.9, 1e-5, lazy_ok=lazy)


def _sums(y):
  """The BnSums record a training-mode BatchNormAct left on its output (a tensor and a LazyAct alike)."""
  rec = getattr(y, '_pf_bn', None)
  assert rec is not None
  return rec


BN_FWD = dict(bn_stats=1, bn_finalize=1)                         # a lazy training-mode BN: statistics + finalize
BN_FWD_MAT = dict(BN_FWD, bn_apply=1)                            # ... a materialised one: + the apply pass
BN_BWD = dict(bn_bwd_stats=1, bn_bwd_apply=1)                    # BN backward with its own statistics pass
BN_BWD_FUSED = dict(bn_bwd_apply=1)                              # ... with the sums the consumer's backward-data kernel left


# -- the fused 1x1 route ------------------------------------------------------------------------------------------------------

def test_1x1_on_a_lazy_act_single_consumer_fuses_the_bn_backward_sums(monkeypatch):
  G, g, fake = _graph(monkeypatch)
  bn, conv = _bn(G, g, 8, True), G.Conv2D(g, 'conv', 8, 16, 1)
  _ready(g, fake)
  q = bn(_image(8))
  assert isinstance(q, G.LazyAct)
  y = conv(q)
  assert _sums(q).n_consumers == 1 and q.n_grad_consumers == 1 and q.dense_out == 16
  assert type(y.grad_fn).__name__ == '_FusedConv1x1Backward'
  y.sum().backward()
  assert fake.calls == dict(BN_FWD, conv1x1_fwd=1, conv1x1_wrw=1, conv1x1_bwd_data_bnstats=1, **BN_BWD_FUSED)


def test_1x1_stride_2_scatters_rows_into_a_zero_filled_gradient(monkeypatch):
  G, g, fake = _graph(monkeypatch)
  bn, conv = _bn(G, g, 8, True), G.Conv2D(g, 'conv', 8, 16, 1, stride=2)
  _ready(g, fake)
  q = bn(_image(8))
  y = conv(q)
  assert tuple(y.shape) == (2, 16, 4, 4)
  assert _sums(q).n_consumers == 1 and q.n_grad_consumers == 1 and q.dense_out is None
  y.sum().backward()
  assert fake.calls == dict(BN_FWD, conv1x1_fwd=1, conv1x1_wrw=1, conv1x1_plain=1, conv1x1_ymap=1, **BN_BWD)
  assert fake.ymap_into_zeros is True


def _two_consumers(monkeypatch, fake, proj_stride, proj_first=False, **switches):
  """bn1 of a projection block: conv1 (dense) and the shortcut convolution read one LazyAct, marked `join_ok` as the block marks it.
  The consumer called LAST runs its backward first."""
  G, g, fake = _graph(monkeypatch, fake, **switches)
  bn = _bn(G, g, 8, True)
  conv1, proj = G.Conv2D(g, 'conv1', 8, 16, 1), G.Conv2D(g, 'proj', 8, 32, 1, stride=proj_stride)
  _ready(g, fake)
  x = _image(8)
  q = bn(x)
  ys = [proj(q), conv1(q)] if proj_first else [conv1(q), proj(q)]
  q.join_ok = True
  # (`dense_out`: the stride-1 consumer called last)
  assert _sums(q).n_consumers == 2 and q.n_grad_consumers == 2 and q.dense_out == (32 if proj_stride == 1 and not proj_first else 16)
  torch.manual_seed(1)
  sum((y * torch.randn_like(y)).sum() for y in ys).backward()
  assert q.pending is None and q.pending_geom is None
  return dict(fake.calls), x.grad.clone(), fake


FWD_2 = dict(BN_FWD, conv1x1_fwd=2, conv1x1_wrw=2)


@pytest.mark.parametrize('proj_stride', [1, 2])
def test_1x1_two_consumers_park_then_deliver(monkeypatch, proj_stride):
  """Without the join two plain launches and autograd's add; with it the first parks and the dense second takes the parked gradient
  as its residual operand -- the same gradient either way."""
  scatter = dict(conv1x1_ymap=1) if proj_stride == 2 else {}
  off, dx_off, _ = _two_consumers(monkeypatch, _Hip(), proj_stride, JOIN_TWO_CONSUMERS=False)
  assert off == dict(FWD_2, conv1x1_plain=2, **scatter, **BN_BWD)
  on, dx_on, fake = _two_consumers(monkeypatch, _Hip(), proj_stride, JOIN_TWO_CONSUMERS=True)
  assert on == dict(FWD_2, conv1x1_plain=2, conv1x1_res=1, **scatter, **BN_BWD)
  assert proj_stride == 1 or fake.ymap_into_zeros is True
  assert float((dx_on - dx_off).abs().max()) <= 1e-5 * float(dx_off.abs().max())


def test_1x1_two_consumers_strided_second_adds_the_parked_gradient_itself(monkeypatch):
  """The strided consumer's backward runs second: no residual operand under a row map, the sum is formed behind the launch."""
  off, dx_off, _ = _two_consumers(monkeypatch, _Hip(), 2, proj_first=True, JOIN_TWO_CONSUMERS=False)
  on, dx_on, _ = _two_consumers(monkeypatch, _Hip(), 2, proj_first=True, JOIN_TWO_CONSUMERS=True)
  assert on == off == dict(FWD_2, conv1x1_plain=2, conv1x1_ymap=1, **BN_BWD)
  assert float((dx_on - dx_off).abs().max()) <= 1e-5 * float(dx_off.abs().max())


@pytest.mark.parametrize('stats', [False, True])
def test_1x1_two_consumers_on_the_projection_join_entry(monkeypatch, stats):
  """A library with pf_conv1x1_bwd_data_join: the strided first consumer parks a COMPACT gradient (a plain GEMM, no scatter), the
  second reads it through the row map -- and leaves the BN-backward sums with PROJ_JOIN_STATS."""
  ref, dx_ref, _ = _two_consumers(monkeypatch, _Hip(), 2, JOIN_TWO_CONSUMERS=False)
  got, dx, fake = _two_consumers(monkeypatch, _HipJoin(), 2, JOIN_TWO_CONSUMERS=True, PROJ_JOIN=True, PROJ_JOIN_STATS=stats)
  if stats:
    assert got == dict(FWD_2, conv1x1_plain=1, conv1x1_join_stats=1, **BN_BWD_FUSED)
  else:
    assert got == dict(FWD_2, conv1x1_plain=1, conv1x1_join=1, **BN_BWD)
  assert fake.ymap_into_zeros is None
  assert float((dx - dx_ref).abs().max()) <= 1e-5 * float(dx_ref.abs().max())
  # both stride 1: the parked gradient is dense, the joined launch still leaves the sums
  got, _, _ = _two_consumers(monkeypatch, _HipJoin(), 1, JOIN_TWO_CONSUMERS=True, PROJ_JOIN=True, PROJ_JOIN_STATS=stats)
  if stats:
    assert got == dict(FWD_2, conv1x1_plain=1, conv1x1_join_stats=1, **BN_BWD_FUSED)
  else:
    assert got == dict(FWD_2, conv1x1_plain=2, conv1x1_res=1, **BN_BWD)
  # PROJ_JOIN off: the entry is not asked for
  got, _, _ = _two_consumers(monkeypatch, _HipJoin(), 2, JOIN_TWO_CONSUMERS=True, PROJ_JOIN=False, PROJ_JOIN_STATS=stats)
  assert got == dict(FWD_2, conv1x1_plain=2, conv1x1_res=1, conv1x1_ymap=1, **BN_BWD)


def test_1x1_on_a_materialised_bn_output_counts_twice(monkeypatch):
  G, g, fake = _graph(monkeypatch)
  bn, conv = _bn(G, g, 8, False), G.Conv2D(g, 'conv', 8, 16, 1)
  _ready(g, fake)
  q = bn(_image(8))
  assert isinstance(q, torch.Tensor)
  y = conv(q)
  assert _sums(q).n_consumers == 2
  assert type(y.grad_fn).__name__ == '_FusedConv1x1Backward'
  y.sum().backward()
  assert fake.calls == dict(BN_FWD_MAT, conv1x1_plain=2, conv1x1_wrw=1, **BN_BWD)


# -- R x S convolutions ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('own', [True, False])
def test_3x3_with_64_channels_runs_on_the_implicit_gemm_entry(monkeypatch, own):
  G, g, fake = _graph(monkeypatch, OWN_CONV2D=own)
  bn, conv = _bn(G, g, 64, False), G.Conv2D(g, 'conv', 64, 64, 3)      # (64 outputs: backward-data contracts over them)
  _ready(g, fake)
  q = bn(_image(64))
  y = conv(q, want_stats=True)
  if own:
    assert _sums(q).n_consumers == 1 and y._pf_stats[1] == 3
    assert type(y.grad_fn).__name__ == '_Conv2dIgemmBackward'
    y.sum().backward()
    assert fake.calls == dict(BN_FWD_MAT, conv2d_fwd=1, conv2d_wrw=1, conv2d_bwd_data_bnstats=1, **BN_BWD_FUSED)
  else:                                       # nothing of ours takes a CPU tensor of 64 channels: the library
    assert _sums(q).n_consumers == 2 and not hasattr(y, '_pf_stats')
    y.sum().backward()
    assert fake.calls == dict(BN_FWD_MAT, **BN_BWD)


def test_3x3_with_8_channels_runs_as_im2col(monkeypatch):
  G, g, fake = _graph(monkeypatch)
  bn, conv = _bn(G, g, 8, False), G.Conv2D(g, 'conv', 8, 16, 3, stride=2)
  _ready(g, fake)
  q = bn(_image(8, 7, 7))                      # odd size, stride 2
  y = conv(q)
  assert _sums(q).n_consumers == 2 and tuple(y.shape) == (2, 16, 4, 4)
  assert type(y.grad_fn).__name__ == '_ConvIm2colBackward'
  y.sum().backward()
  assert fake.calls == dict(BN_FWD_MAT, im2col=2, col2im=1, conv1x1_plain=2, conv1x1_wrw=1, **BN_BWD)


def test_3x3_with_4_channels_on_a_cpu_tensor_runs_in_the_library(monkeypatch):
  G, g, fake = _graph(monkeypatch)
  bn, conv = _bn(G, g, 4, False), G.Conv2D(g, 'conv', 4, 16, 3, use_bias=True)
  _ready(g, fake)
  x = _image(4)
  q = bn(x)
  y = conv(q)
  assert _sums(q).n_consumers == 2
  assert torch.equal(y, F.conv2d(q, conv.kernel.tensor, conv.bias.tensor, padding=1))
  y.sum().backward()
  assert fake.calls == dict(BN_FWD_MAT, **BN_BWD)


# -- the stems -------------------------------------------------------------------------------------------------------------------

def test_resnet_stem(monkeypatch):
  G, g, fake = _graph(monkeypatch)
  conv = G.Conv2D(g, 'conv', 3, 64, 7, stride=2, padding=3)
  _ready(g, fake)
  y = conv(_image(3, 4, 32, grad=False))
  assert tuple(y.shape) == (2, 64, 2, 16) and type(y.grad_fn).__name__ == '_StemConvBackward'
  y.sum().backward()
  assert fake.calls == dict(conv_stem_fwd=1, conv_stem_wrw=1)


def test_resnet_stem_as_the_network_calls_it(monkeypatch):
  """resnet_model._ConvFixedPadding hands the pad of an odd strided kernel to the layer: the stem kernel.  fixed_padding() itself in
  front of a 'VALID' layer (what it does for an even kernel) leaves a padded copy the stem kernel does not take: the library."""
  from pocketflow_amd.utils.external import resnet_model as R
  G, g, fake = _graph(monkeypatch)
  stem = R._ConvFixedPadding(g, 3, 64, 7, 2)
  valid = G.Conv2D(g, 'valid', 3, 64, 7, stride=2, padding='VALID')
  _ready(g, fake)
  x = _image(3, 4, 32, grad=False)
  y = stem(x)
  assert type(y.grad_fn).__name__ == '_StemConvBackward'
  y.sum().backward()
  assert fake.calls == dict(conv_stem_fwd=1, conv_stem_wrw=1)
  fake.calls.clear()
  y2 = valid(G.fixed_padding(x, 7))
  assert tuple(y2.shape) == tuple(y.shape)
  y2.sum().backward()
  assert fake.calls == {}


def test_mobilenet_stem_reads_the_image_itself(monkeypatch):
  """3x3 / 2 'SAME' over an even size: pads (0, 1), asymmetric -- the stem kernel is asked BEFORE the padded copy would be made."""
  G, g, fake = _graph(monkeypatch)
  conv = G.Conv2D(g, 'conv', 3, 16, 3, stride=2)
  _ready(g, fake)
  x = _image(3, 4, 32, grad=False)
  assert conv._geometry(x.shape)[:2] == ((0, 1), (0, 1))
  y = conv(x)
  assert fake.stem3_input is x
  assert tuple(y.shape) == (2, 16, 2, 16) and type(y.grad_fn).__name__ == '_Stem3ConvBackward'
  y.sum().backward()
  assert fake.calls == dict(conv_stem3_fwd=1, conv_stem3_wrw=1)
  # an image that asks for its gradient is not the stem's: the padded copy and the library
  fake.calls.clear()
  fake.stem3_input = None
  conv(_image(3, 4, 32)).sum().backward()
  assert fake.calls == {} and fake.stem3_input is None


# -- no gradients ----------------------------------------------------------------------------------------------------------------

def _fold_bn(G, g, c):
  bn = G.BatchNormAct(g, 'out_bn', c, 'Relu', 0.9, 1e-5)
  return bn


@pytest.mark.parametrize('cin,k,lazy,calls', [
    (8, 1, True, dict(conv1x1_fwd=1)),                      # the producer BN in the prologue (an inference-mode LazyAct)
    (8, 1, False, dict(bn_apply=1, conv1x1_plain=1)),
    (64, 3, False, dict(bn_apply=1, conv2d_fwd=1)),
])
def test_no_grad_1x1_and_implicit_gemm_fold_the_consumers_bn(monkeypatch, cin, k, lazy, calls):
  G, g, fake = _graph(monkeypatch)
  bn, conv, out_bn = _bn(G, g, cin, lazy), G.Conv2D(g, 'conv', cin, 16, k), _fold_bn(G, g, 16)
  _ready(g, fake)
  x = _image(cin, grad=False)
  with torch.no_grad():
    assert out_bn.folds_into_producer()
    y = conv(bn(x), out_bn=out_bn)
    assert y.grad_fn is None and y._pf_bn_done is out_bn and not hasattr(y, '_pf_stats')
    assert out_bn(y) is y
    assert fake.calls == dict(calls, conv_out_affine=1)
    fake.calls.clear()
    y = conv(bn(x), residual=torch.zeros_like(y), want_stats=True, out_bn=out_bn)     # a residual: the hint is dropped
    assert y.grad_fn is None and not hasattr(y, '_pf_bn_done')
    assert hasattr(y, '_pf_stats') == (k == 1)     # (the implicit-GEMM route adds the residual behind the launch: a new tensor)
    assert fake.calls == (dict(calls, conv1x1_res=1) if (k == 1 and not lazy) else calls)
  # under gradients the hint is ignored (the layer does not fold: its input must exist)
  assert not out_bn.folds_into_producer()
  y = conv(bn(x), out_bn=out_bn)
  assert y.grad_fn is not None and not hasattr(y, '_pf_bn_done')


@pytest.mark.parametrize('cin,cout,k,stride,padding,size,calls', [
    (8, 16, 3, 1, 'SAME', (8, 8), dict(bn_apply=1, im2col=1, conv1x1_plain=1)),
    (4, 16, 3, 1, 'SAME', (8, 8), dict(bn_apply=1)),
    (3, 64, 7, 2, 3, (4, 32), dict(bn_apply=1, conv_stem_fwd=1)),
    (3, 16, 3, 2, 'SAME', (4, 32), dict(bn_apply=1, conv_stem3_fwd=1)),
])
def test_no_grad_routes_make_no_autograd_node(monkeypatch, cin, cout, k, stride, padding, size, calls):
  """(The producer BN in front of the stems only serves to hand every route an output of the same kind.)"""
  G, g, fake = _graph(monkeypatch)
  bn, conv, out_bn = _bn(G, g, cin, False), G.Conv2D(g, 'conv', cin, cout, k, stride=stride, padding=padding), _fold_bn(G, g, cout)
  _ready(g, fake)
  with torch.no_grad():
    y = conv(bn(_image(cin, *size, grad=False)), out_bn=out_bn)
  assert y.grad_fn is None and not y.requires_grad
  assert not hasattr(y, '_pf_bn_done')          # honoured by the 1x1 (strided or not), implicit-GEMM and gather routes alone
  assert fake.calls == calls


def test_no_grad_strided_1x1_folds_too(monkeypatch):
  G, g, fake = _graph(monkeypatch)
  conv, out_bn = G.Conv2D(g, 'conv', 8, 16, 1, stride=2), _fold_bn(G, g, 16)
  _ready(g, fake)
  with torch.no_grad():
    y = conv(_image(8, grad=False), out_bn=out_bn)
  assert y._pf_bn_done is out_bn and fake.calls == dict(conv1x1_plain=1, conv_out_affine=1)


# -- depthwise ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('own', [True, False])
def test_depthwise_3x3(monkeypatch, stride, own):
  G, g, fake = _graph(monkeypatch, OWN_DEPTHWISE=own)
  bn, dw = _bn(G, g, 8, False, act='Relu6'), G.DepthwiseConv2D(g, 'dw', 8, 3, stride)
  _ready(g, fake)
  q = bn(_image(8))
  y = dw(q, want_stats=True)
  assert tuple(y.shape) == (2, 8, 8 // stride, 8 // stride)
  if own:
    assert _sums(q).n_consumers == 2 and y._pf_stats[1] == 2
    assert type(y.grad_fn).__name__ == '_DepthwiseBackward'
    y.sum().backward()
    assert fake.calls == dict(BN_FWD_MAT, depthwise_fwd=1, depthwise_wrw=1, depthwise_bwd_data=1, **BN_BWD)
  else:
    assert _sums(q).n_consumers == 0 and not hasattr(y, '_pf_stats')      # the library fallback counts nothing
    y.sum().backward()
    assert fake.calls == dict(BN_FWD_MAT, **BN_BWD)
  with torch.no_grad():
    fake.calls.clear()
    y0 = dw(q.detach())
    assert y0.grad_fn is None and fake.calls == (dict(depthwise_fwd=1) if own else {})
    assert float((y0 - y).abs().max()) <= 1e-5 * float(y.abs().max())


# -- dense -----------------------------------------------------------------------------------------------------------------------------

def test_dense_on_a_cpu_tensor_is_the_library(monkeypatch):
  G, g, fake = _graph(monkeypatch)
  dense = G.Dense(g, 'dense', 8, 5)
  _ready(g, fake)
  with torch.no_grad():
    dense.bias.tensor.copy_(torch.arange(5.0))
  torch.manual_seed(0)
  x = torch.randn(2, 8)
  assert torch.equal(dense(x), F.linear(x, dense.kernel.tensor, dense.bias.tensor))
  assert torch.equal(dense.plain(x), F.linear(x, dense.kernel.tensor))
  assert fake.calls == {}


# -- taps and packed layers ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('lazy', [True, False])
def test_tapped_conv2d(monkeypatch, lazy):
  """A tap materialises a LazyAct (a consumer that counts twice) and hands the plain call an untagged tensor; a materialised BN
  output is counted by the plain call behind the tap (the library route: twice)."""
  G, g, fake = _graph(monkeypatch)
  bn, conv = _bn(G, g, 8, lazy), G.Conv2D(g, 'conv', 8, 16, 1)
  _ready(g, fake)
  g.taps = {}
  q = bn(_image(8))
  assert isinstance(q, G.LazyAct) == lazy
  res = torch.ones(2, 16, 8, 8)
  y = conv(q, residual=res)
  assert _sums(q).n_consumers == 2
  assert g.taps is not None and g.fuse_conv1x1 is True          # plain() put the switches back
  x_tap, y_tap, src, y_add, r_tap = g.taps[conv]
  assert x_tap is G.materialize(q) or not lazy
  assert isinstance(x_tap, torch.Tensor) and src is None and r_tap is res and y is y_add
  assert torch.equal(y_tap, F.conv2d(x_tap, conv.kernel.tensor)) and torch.equal(y_add, y_tap + res)
  assert y_tap._pf_src is conv
  assert fake.calls == dict(BN_FWD, bn_apply=1)                 # the convolution itself ran in the library


def test_tapped_depthwise(monkeypatch):
  G, g, fake = _graph(monkeypatch)
  bn, dw = _bn(G, g, 8, False), G.DepthwiseConv2D(g, 'dw', 8, 3, 1)
  _ready(g, fake)
  g.taps = {}
  q = bn(_image(8))
  y = dw(q)
  assert _sums(q).n_consumers == 2
  x_tap, y_tap, src, y_add, r_tap = g.taps[dw]
  assert x_tap is q and y_tap is y and src is None and y_add is None and r_tap is None and y._pf_src is dw
  assert g.taps is not None
  assert fake.calls == dict(BN_FWD_MAT, depthwise_fwd=1)


def test_a_packed_conv2d_refuses_gradients(monkeypatch):
  G, g, fake = _graph(monkeypatch)
  conv, dw = G.Conv2D(g, 'conv', 8, 16, 1), G.DepthwiseConv2D(g, 'dw', 8, 3, 1)
  _ready(g, fake)
  conv.int8 = {}
  dw.int8 = {}
  with pytest.raises(RuntimeError, match='conv/kernel: a convolution packed for int8 runs in inference only'):
    conv(_image(8, grad=False))
  with pytest.raises(RuntimeError, match='dw/depthwise_weights: a depthwise convolution packed for int8 runs in inference only'):
    dw(_image(8, grad=False))
  assert fake.calls == {}
