"""ResNet v1 with bottleneck blocks (utils/external/resnet_model.py:202-254 of the reference) and the layer of its block tail,
graph.BatchNormAddAct, on the CPU.

tests/golden/resnet_v1_50_vars.json was made in the build container by EXECUTING the reference's own resnet_model.py
(Model(50, True, 10, 64, 7, 2, 3, 2, [3, 4, 6, 3], [1, 2, 2, 2], resnet_version=1)) over oracle/tf_stub.py: the stub's tf.layers
stand-ins were wrapped so that every variable the network asks for is created on demand with the seeded recipe `_value_of` below
repeats, in the order asked (= TF's creation order).  It holds the variable names and shapes in that order, the number of
tf.nn.relu calls, and the inference-mode logits of one seeded input (RandomState(7).randn(2, 32, 32, 3)).  Training-mode logits are
not part of it: at batch 2 and 32 x 32 pixels the last stage normalises over TWO values per channel, so its output is +-1 with a
sign that round-off decides wherever the two are close, and float32 and the stub's float64 normalisation disagree at the 0.5 level.
(The same comparison at 96 x 96 pixels, 18 values per channel, was run once in the build container: 3.2e-5 of the largest logit.)

The HIP entry points are doubles here (tests/fake_hip.py); `JoinFakeHip` adds float32 emulations of the three new ones, with which
the host logic of the join -- autograd plumbing, slots, the two aliases of a block output -- is checked against torch autograd."""
import hashlib
import json
import os
import types

import numpy as np
import pytest
import torch

from fake_hip import FakeHipFull, _act, _mask, _rows  # noqa: E402  (tests/fake_hip.py)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'resnet_v1_50_vars.json')
V1_50 = (50, True, 10, 64, 7, 2, 3, 2, [3, 4, 6, 3], [1, 2, 2, 2])


class JoinFakeHip(FakeHipFull):
  """... plus pf_bn_add_act_groups / pf_bn_add_act_fwd / pf_bn_add_act_bwd_gate[_add] (include/pocketflow_hip.h)."""

  def bn_add_act_groups(self, rows, C):
    return 3

  def bn_add_act_fwd(self, x, r, u, rows, C, ss, act, slot=None):
    self._n('bn_add_act_fwd')
    y = _act(_rows(x, C).float() * ss[0] + ss[1] + _rows(r, C).float(), act)
    _rows(u, C).copy_(y)
    if slot is not None:
      cur = slot.view(torch.float32)
      stored = _rows(u, C).float()
      cur[0], cur[1] = min(float(cur[0]), float(stored.min())), max(float(cur[1]), float(stored.max()))

  def bn_add_act_bwd_gate(self, dq, x, r, g, rows, C, ss, mi, act, partial, addend=None):
    self._n('bn_add_act_bwd_gate_add' if addend is not None else 'bn_add_act_bwd_gate')
    xr = _rows(x, C).float()
    d = _rows(dq, C).float()
    if addend is not None:
      d = d + _rows(addend, C).float()
    gv = d * _mask(xr * ss[0] + ss[1] + _rows(r, C).float(), act)
    _rows(g, C).copy_(gv)
    p = partial[:3 * 2 * C].view(3, 2, C)
    p.zero_()
    p[1, 0], p[1, 1] = gv.sum(0), (gv * (xr - mi[0]) * mi[1]).sum(0)


def _value_of(index, name, shape):
  """The recipe of the fixture's variables: variable number `index` in creation order."""
  rng = np.random.RandomState(1000 + index)
  leaf = name.rsplit('/', 1)[1]
  if leaf == 'kernel' and len(shape) == 4:
    v = rng.randn(*shape) * np.sqrt(2.0 / (shape[0] * shape[1] * shape[2]))
  elif leaf == 'kernel':
    v = rng.randn(*shape) * 0.05
  elif leaf in ('gamma', 'moving_variance'):
    v = rng.rand(*shape) + 0.5
  else:                                            # beta, moving_mean, bias
    v = rng.randn(*shape) * 0.1
  return v.astype(np.float32)


def _patch(monkeypatch, fake, any_device):
  from pocketflow_amd import graph as G
  monkeypatch.setattr(G, 'hip', fake)
  monkeypatch.setattr(G, 'BN_JOIN_ANY_DEVICE', any_device)
  return G


def _build_v1_50(G, seed=3):
  from pocketflow_amd.utils.external import resnet_model as R
  g = G.Graph('model', 'cpu', torch.float32)
  net = R.Model(*V1_50, resnet_version=1, graph=g)
  return g, net


@pytest.fixture(scope='module')
def golden():
  return json.load(open(GOLDEN))


def _run_v1_50(monkeypatch, golden, fake, any_device, act_bits=None):
  """Forward in inference mode, then a training-mode forward and backward, of ResNet-50 v1 on the fixture's variables and input."""
  G = _patch(monkeypatch, fake, any_device)
  g, net = _build_v1_50(G)
  assert [[v.name, list(v.ref_shape)] for v in g.store.vars] == golden['vars']
  g.finalize(seed=3, requires_grad=True)
  g.store.load_numpy({n: _value_of(i, n, tuple(s)) for i, (n, s) in enumerate(golden['vars'])}, strict=True)
  for op in g.activation_ops:
    op.bits = act_bits
  g.begin_step = lambda: None
  fake.minmax_slots_init(g.act_slots)
  images = np.random.RandomState(golden['input']['seed']).randn(*golden['input']['shape']).astype(np.float32)
  x = G.to_device_images(images, g)
  with torch.no_grad(), g.as_default():
    ev = net(x, False)
  fake.minmax_slots_init(g.act_slots)              # a new step: the quantisers' ranges start over
  with g.as_default():
    tr = net(x, True)
  wts = torch.from_numpy(np.random.RandomState(11).randn(*tr.shape).astype(np.float32))
  (tr * wts).sum().backward()
  st = g.store
  return dict(eval=ev.detach().clone(), train=tr.detach().clone(), w_grad=st.w_grad.clone(), o_grad=st.o_grad.clone(),
              state=st.state.clone(), calls=dict(fake.calls), graph=g)


def _rel(a, b):
  a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
  return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def test_resnet50_v1_builds_runs_and_matches_the_reference(monkeypatch, golden):
  """The network of the reference: same variables in the same order, same inference-mode logits (the stub normalises in float64
  and this executor in float32: 16 blocks of float32 round-off, 1e-3 of the largest logit), a finite training-mode forward, and a backward pass that reaches every
  variable.  On the CPU the join runs the composition of the v1 basic block (BatchNormAct, add, Activation)."""
  out = _run_v1_50(monkeypatch, golden, FakeHipFull(), False)
  assert len(golden['vars']) == 267
  assert _rel(out['eval'], golden['logits_eval']) < 1e-3, _rel(out['eval'], golden['logits_eval'])
  assert torch.isfinite(out['train']).all()
  assert 'bn_add_act_fwd' not in out['calls']
  for k in ('w_grad', 'o_grad'):
    assert torch.isfinite(out[k]).all() and float(out[k].abs().max()) > 0.0
  g = out['graph']
  for v in g.store.trainable_vars:
    assert float(v.tensor.grad.abs().max()) > 0.0, v.name


@pytest.mark.parametrize('act_bits', [None, 6])
def test_join_plumbing_in_the_network_equals_the_composition(monkeypatch, golden, act_bits):
  """The same network with the join on the (emulated) entry points: logits, every gradient and the BN state as with the
  composition, to float32 round-off; one forward launch per block and mode, one gate launch per block -- the 15 block outputs that
  feed another block hand it the gradients of their two consumers separately (the addend form), the last one has one consumer."""
  a = _run_v1_50(monkeypatch, golden, JoinFakeHip(), False, act_bits)
  b = _run_v1_50(monkeypatch, golden, JoinFakeHip(), True, act_bits)
  for k in ('eval', 'train', 'w_grad', 'o_grad', 'state'):
    assert _rel(b[k], a[k]) < 5e-5, (k, _rel(b[k], a[k]))
  assert b['calls']['bn_add_act_fwd'] == 2 * 16 + 1        # + the fork's sum in front of the first block
  assert b['calls']['bn_add_act_bwd_gate_add'] == 15 and b['calls']['bn_add_act_bwd_gate'] == 1


def _layer_case(monkeypatch, act_bits, seed=0):
  G = _patch(monkeypatch, JoinFakeHip(), True)
  g = G.Graph('model', 'cpu', torch.float32)
  C = 16
  layer = G.BatchNormAddAct(g, 'resnet_model/batch_normalization', C, 'Relu', 0.997, 1e-5, act_name='resnet_model/Relu')
  g.finalize(seed=3, requires_grad=True)
  layer.op.bits = act_bits
  G.hip.minmax_slots_init(g.act_slots)
  gen = torch.Generator().manual_seed(seed)
  with torch.no_grad():
    layer.bn.gamma.tensor.copy_(0.5 + torch.rand(C, generator=gen))
    layer.bn.beta.tensor.copy_(0.3 * torch.randn(C, generator=gen))
  x = torch.randn(4, C, 5, 3, generator=gen).contiguous(memory_format=torch.channels_last).requires_grad_(True)
  s = torch.randn(4, C, 5, 3, generator=gen).contiguous(memory_format=torch.channels_last).requires_grad_(True)
  w = torch.randn(4, C, 5, 3, generator=gen)
  g.store.zero_grad()
  g.training = True
  with g.as_default():
    u = layer(x, s)
  (u * w).sum().backward()
  return G, g, layer, x, s, w, u


@pytest.mark.parametrize('act_bits', [None, 6])
def test_layer_forward_and_gradients_equal_autograd(monkeypatch, act_bits):
  """forward, dx, dshortcut, dgamma, dbeta of BatchNormAddAct against torch autograd of relu(bn(x) + s) in float64; the quantiser
  is straight-through, so the backward is the same with and without it."""
  G, g, layer, x, s, w, u = _layer_case(monkeypatch, act_bits)
  xd, sd = x.detach().double().requires_grad_(True), s.detach().double().requires_grad_(True)
  gam = layer.bn.gamma.tensor.detach().double().requires_grad_(True)
  bet = layer.bn.beta.tensor.detach().double().requires_grad_(True)
  mean = xd.mean(dim=(0, 2, 3), keepdim=True)
  var = ((xd - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
  y = (xd - mean) / torch.sqrt(var + 1e-5) * gam.view(1, -1, 1, 1) + bet.view(1, -1, 1, 1)
  ref = torch.relu(y + sd)
  (ref * w.double()).sum().backward()
  want = ref.detach()
  if act_bits is not None:
    lo, hi = want.min(), want.max()
    alpha, k = (hi - lo) + 1e-10, float(2 ** act_bits - 1)
    want = alpha * (torch.round((want - lo) / alpha * k) / k) + lo
    mn, mx = G.hip._slot_get(g.act_slots[layer.op.index])
    assert abs(mn - float(lo)) < 1e-6 and abs(mx - float(hi)) < 1e-5
  assert _rel(u.detach(), want) < 1e-5
  assert _rel(x.grad, xd.grad) < 1e-5 and _rel(s.grad, sd.grad) < 1e-6
  assert _rel(layer.bn.gamma.tensor.grad, gam.grad) < 1e-5 and _rel(layer.bn.beta.tensor.grad, bet.grad) < 1e-5
  # the moving averages are a BatchNormAct's: moving -= (moving - batch) * (1 - momentum), the unbiased variance
  n = x.numel() // 16
  assert _rel(layer.bn.moving_mean.tensor, 0.003 * mean.detach().view(-1)) < 1e-4
  assert _rel(layer.bn.moving_var.tensor, 0.997 + 0.003 * var.detach().view(-1) * n / (n - 1)) < 1e-5


def test_two_consumers_of_a_join_output_are_summed_in_the_gate_pass(monkeypatch):
  """The output carries a second alias for its second consumer; their gradients reach the gate pass separately (addend form) and
  the result equals the gradient of the sum."""
  G, g, layer, x, s, w, u = _layer_case(monkeypatch, None, seed=1)
  gx, gs = x.grad.clone(), s.grad.clone()
  x.grad = s.grad = None
  g.store.zero_grad()
  with g.as_default():
    u2 = layer(x, s)
  assert u2._pf_skip.data_ptr() == u2.data_ptr()
  (u2 * (0.25 * w) + u2._pf_skip * (0.75 * w)).sum().backward()
  assert G.hip.calls['bn_add_act_bwd_gate_add'] == 1
  assert _rel(x.grad, gx) < 1e-5 and _rel(s.grad, gs) < 1e-5


def test_join_falls_back_to_the_composition(monkeypatch):
  """No GPU tensor (the switch of the doubles off), or C % 8 != 0: BatchNormAct, add, Activation -- nothing of the join kernels."""
  fake = JoinFakeHip()
  G = _patch(monkeypatch, fake, True)
  g = G.Graph('model', 'cpu', torch.float32)
  layer = G.BatchNormAddAct(g, 'resnet_model/batch_normalization', 12, 'Relu', 0.997, 1e-5, act_name='resnet_model/Relu')
  g.finalize(seed=3, requires_grad=True)
  x, s = torch.randn(2, 12, 3, 3, requires_grad=True), torch.randn(2, 12, 3, 3)
  with g.as_default():
    u = layer(x, s)
  u.sum().backward()
  assert 'bn_add_act_fwd' not in fake.calls and fake.calls['bn_apply'] == 1 and not hasattr(u, '_pf_skip')
  assert torch.isfinite(x.grad).all()


def test_one_quantised_activation_per_relu_of_the_reference(monkeypatch, golden):
  G = _patch(monkeypatch, FakeHipFull(), False)
  g, net = _build_v1_50(G)
  names = [op.name for op in g.activation_ops]
  assert len(names) == golden['relu_ops'] == 49 and len(set(names)) == 49
  assert all(op.type == 'Relu' for op in g.activation_ops)
  assert names == ['model/resnet_model/Relu'] + ['model/resnet_model/Relu_%d' % i for i in range(1, 49)]
  assert len(g.join_layers) == 16
  join_ops = [j.op for j in g.join_layers]
  assert all(g.activation_ops[op.index] is op for op in join_ops) and len({op.index for op in join_ops}) == 16
  # creation order inside a block: Relu behind bn1, behind bn2, behind the sum
  assert [op.index for op in join_ops] == [3 * i + 3 for i in range(16)]


def _set_flags(**kw):
  import pocketflow_amd.nets.resnet_at_ilsvrc12 as N  # noqa: F401
  from pocketflow_amd.flags import FLAGS
  old = {k: getattr(FLAGS, k) for k in kw}
  for k, v in kw.items():
    setattr(FLAGS, k, v)
  return N, FLAGS, old


def test_load_int8_refuses_a_v1_bottleneck_graph(monkeypatch, tmp_path):
  from pocketflow_amd import inference
  N, FLAGS, old = _set_flags(resnet_size=50, nb_classes=10, resnet_version=1)
  try:
    mh = types.SimpleNamespace(dataset_train=types.SimpleNamespace(batch_size=2, image_shape=(32, 32, 3)),
                               forward_eval=lambda inputs: N.forward_fn(inputs, False, 'channels_last'))
    path = str(tmp_path / 'model_int8.npz')
    np.savez(path, **{'model/resnet_model/dense/bias': np.zeros(10, np.float32)})
    for kw in (dict(int8='on'), dict(int8='off'), dict(int8='auto', depthwise='on')):
      with pytest.raises(ValueError, match=r'model/resnet_model/batch_normalization_4: .*not covered by the int8 / static-range loaders'):
        inference.load_int8(mh, path, 'cpu', torch.float32, 8, **kw)
  finally:
    for k, v in old.items():
      setattr(FLAGS, k, v)


def test_join_refuses_static_ranges_and_the_int8_route(monkeypatch):
  G = _patch(monkeypatch, JoinFakeHip(), True)
  g = G.Graph('model', 'cpu', torch.float32)
  layer = G.BatchNormAddAct(g, 'resnet_model/batch_normalization_7', 16, 'Relu', 0.997, 1e-5, act_name='resnet_model/Relu')
  g.finalize(seed=3, requires_grad=False)
  x = torch.randn(2, 16, 3, 3)
  for attr, value in (('act_static', torch.zeros(1, 2)), ('int8', True)):
    setattr(g, attr, value)
    with pytest.raises(ValueError, match='batch_normalization_7.*not covered'):
      with torch.no_grad(), g.as_default():
        layer(x, x)
    setattr(g, attr, None if attr == 'act_static' else False)


# the variables of ResNet-50 v2, in creation order, as the constructor made them before the v1 bottleneck block existed: c<k>x<cin>x<cout>
# a convolution kernel, b<C> the four variables of a BatchNorm
V2_50 = ('c7x3x64 b64 c1x64x256 c1x64x64 b64 c3x64x64 b64 c1x64x256 b256 c1x256x64 b64 c3x64x64 b64 c1x64x256 b256 c1x256x64 b64 '
         'c3x64x64 b64 c1x64x256 b256 c1x256x512 c1x256x128 b128 c3x128x128 b128 c1x128x512 b512 c1x512x128 b128 c3x128x128 b128 '
         'c1x128x512 b512 c1x512x128 b128 c3x128x128 b128 c1x128x512 b512 c1x512x128 b128 c3x128x128 b128 c1x128x512 b512 c1x512x1024 '
         'c1x512x256 b256 c3x256x256 b256 c1x256x1024 b1024 c1x1024x256 b256 c3x256x256 b256 c1x256x1024 b1024 c1x1024x256 b256 '
         'c3x256x256 b256 c1x256x1024 b1024 c1x1024x256 b256 c3x256x256 b256 c1x256x1024 b1024 c1x1024x256 b256 c3x256x256 b256 '
         'c1x256x1024 b1024 c1x1024x256 b256 c3x256x256 b256 c1x256x1024 b1024 c1x1024x2048 c1x1024x512 b512 c3x512x512 b512 '
         'c1x512x2048 b2048 c1x2048x512 b512 c3x512x512 b512 c1x512x2048 b2048 c1x2048x512 b512 c3x512x512 b512 c1x512x2048 b2048')
V2_50_SHA256 = 'cf9153cabd5856882d697a53a1611e5949a04808e078abad5197e024c87c9cfb'    # of the 'name:shape' lines, taken on the parent


def _v2_50_expected():
  out, nc, nb = [], 0, 0
  for tok in V2_50.split():
    if tok[0] == 'c':
      k, cin, cout = (int(t) for t in tok[1:].split('x'))
      out.append(['model/resnet_model/conv2d%s/kernel' % ('_%d' % nc if nc else ''), [k, k, cin, cout]])
      nc += 1
    else:
      for leaf in ('gamma', 'beta', 'moving_mean', 'moving_variance'):
        out.append(['model/resnet_model/batch_normalization%s/%s' % ('_%d' % nb if nb else '', leaf), [int(tok[1:])]])
      nb += 1
  return out + [['model/resnet_model/dense/kernel', [2048, 10]], ['model/resnet_model/dense/bias', [10]]]


def test_flag_defaults_to_v2_and_the_v2_network_is_unchanged(monkeypatch):
  N, FLAGS, old = _set_flags(resnet_size=50, nb_classes=10)
  try:
    assert FLAGS.resnet_version == 2 and FLAGS._defs['resnet_version'][1] == 2
    helper = types.SimpleNamespace()
    assert N.ModelHelper.model_name.fget(helper) == 'resnet_50'
    G = _patch(monkeypatch, FakeHipFull(), False)
    g = G.Graph('model', 'cpu', torch.float32)
    with g.as_default():
      N.forward_fn(torch.empty((2, 32, 32, 3), device='meta'), True, 'channels_last')
    got = [[v.name, list(v.ref_shape)] for v in g.store.vars]
    assert got == _v2_50_expected()
    lines = ['%s:%s' % (n, 'x'.join(map(str, s))) for n, s in got]
    assert hashlib.sha256('\n'.join(lines).encode()).hexdigest() == V2_50_SHA256
    assert len(g.join_layers) == 0 and len(g.activation_ops) == 49
    FLAGS.resnet_version = 1
    assert N.ModelHelper.model_name.fget(helper) == 'resnet_v1_50'
    g1 = G.Graph('model', 'cpu', torch.float32)
    with g1.as_default():
      N.forward_fn(torch.empty((2, 32, 32, 3), device='meta'), True, 'channels_last')
    assert len(g1.join_layers) == 16
  finally:
    FLAGS.resnet_version = 2
    for k, v in old.items():
      setattr(FLAGS, k, v)
