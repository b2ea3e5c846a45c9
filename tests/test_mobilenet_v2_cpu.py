"""MobileNet-v2 (pocketflow_amd/utils/external/mobilenet_v2.py) on the CPU: the variables of the reference in its creation order
(tests/golden/mobilenet_v2_vars.json: derived by READING the reference, not by executing it -- the slim stand-ins under oracle/ cover what
MobileNet-v1 uses and cannot import the v2 modules as they are; tests/mobilenet_v2_ref.py is the derivation and writes the file), the parameter counts, the ops the
learners see, the forward pass of the composition against a float64 restatement in plain torch (tests/mobilenet_v2_ref.py), the model
helper's learning-rate schedule, and the activation-free BatchNormAddAct on emulated kernels.

The HIP entry points are doubles here (tests/fake_hip.py); `V2FakeHip` adds emulations of the join entries and of the two new
depthwise entries (pf_depthwise_fwd_act / pf_depthwise_wrw_act: the apply pass composed with the plain emulation)."""
import json
import os

import numpy as np
import pytest
import torch

import mobilenet_v2_ref as R
from fake_hip import FakeHipFull, _act, _mask, _rows  # noqa: E402  (tests/fake_hip.py)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mobilenet_v2_vars.json')


class V2FakeHip(FakeHipFull):
  """... plus pf_bn_add_act_* (as tests/test_resnet_v1_cpu.py's) and pf_depthwise_fwd_act / pf_depthwise_wrw_act."""

  def depthwise_supported(self, C, k, stride):      # pf_depthwise_supported as it stands: any C % 8 == 0
    return k == 3 and C % 8 == 0 and 8 <= C <= 2048 and stride in (1, 2)

  def bn_add_act_groups(self, rows, C):
    return 3

  def bn_add_act_fwd(self, x, r, u, rows, C, ss, act, slot=None):
    self._n('bn_add_act_fwd')
    assert slot is None or act is not None
    _rows(u, C).copy_(_act(_rows(x, C).float() * ss[0] + ss[1] + _rows(r, C).float(), act))

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

  def _applied(self, X, ss, act, slot, bits):
    q = torch.empty_like(X)
    C = X.shape[1]
    FakeHipFull.bn_act_quant_apply(self, X, q, X.numel() // C, C, ss, act, slot, bits, slot is not None)
    self.calls['bn_apply'] -= 1          # (the emulation's own use of the apply pass is not a launch of it)
    return q

  def depthwise_fwd_act(self, X, ss, act, slot, bits, W, Y, B, H, Wd, C, k, stride, pad_h, pad_w, Ho, Wo, partial=None):
    self._n('depthwise_fwd_act')
    FakeHipFull.depthwise_fwd(self, self._applied(X, ss, act, slot, bits), W, Y, B, H, Wd, C, k, stride, pad_h, pad_w, Ho, Wo, partial=partial)
    self.calls['depthwise_fwd'] -= 1

  def depthwise_wrw_act(self, dY, X, ss, act, slot, bits, dW, slabs, B, H, Wd, C, k, stride, pad_h, pad_w, Ho, Wo):
    self._n('depthwise_wrw_act')
    FakeHipFull.depthwise_wrw(self, dY, self._applied(X, ss, act, slot, bits), dW, slabs, B, H, Wd, C, k, stride, pad_h, pad_w, Ho, Wo)
    self.calls['depthwise_wrw'] -= 1


@pytest.fixture(scope='module')
def golden():
  return json.load(open(GOLDEN))


def _build(G, mult, num_classes=1001, keep=1.0):
  from pocketflow_amd.utils.external.mobilenet_v2 import MobilenetV2
  g = G.Graph('model', 'cpu', torch.float32)
  return g, MobilenetV2(g, num_classes=num_classes, depth_multiplier=mult, dropout_keep_prob=keep)


@pytest.mark.parametrize('mult,params,last', [(1.0, 3506153, 1280), (0.5, 1225641, 640)])
def test_variables_ops_and_parameter_counts_are_the_reference_s(golden, mult, params, last):
  from pocketflow_amd import graph as G
  g, net = _build(G, mult)
  want = golden['multipliers']['%.1f' % mult]
  assert [[v.name, list(v.ref_shape)] for v in g.store.vars] == [['model/' + n, s] for n, s in want['vars']]
  assert want['vars'] == R.var_list(mult, 1001)               # the fixture is what its generator writes
  assert sum(v.numel for v in g.store.trainable_vars) == params == want['trainable_parameters']
  assert net.features == last == net.last.kernel.ref_shape[3]
  # what the learners enumerate: 35 ReLU6 and nothing else; ten joins, none with an activation op, slot or quantiser
  assert len(g.activation_ops) == 35 and {op.type for op in g.activation_ops} == {'Relu6'}
  assert len(g.join_layers) == 10 == sum(b.residual for b in net.blocks)
  assert all(j.op is None and j.relu is None and j.act is None and j.bn.op is None for j in g.join_layers)
  assert all(b.project_bn.op is None for b in net.blocks)
  assert [op.type for op in g.matmul_ops].count('DepthwiseConv2dNative') == 17 and len(g.matmul_ops) == 53
  assert net.blocks[0].expand is None and all(b.expand is not None for b in net.blocks[1:])
  # laziness: the stem's and every expansion's BN feed a depthwise layer alone, a depthwise BN its projection
  assert net.stem_bn.lazy_ok and net.stem_bn.consumer is net.blocks[0].depthwise and not net.last_bn.lazy_ok
  for b in net.blocks:
    assert b.depthwise_bn.lazy_ok and b.depthwise_bn.consumer is b.project
    assert b.expand_bn is None or (b.expand_bn.lazy_ok and b.expand_bn.consumer is b.depthwise)


def test_parameter_count_at_1000_classes():
  from pocketflow_amd import graph as G
  g, _ = _build(G, 1.0, num_classes=1000)
  assert sum(v.numel for v in g.store.trainable_vars) == 3504872
  # the sixteen expanded tensors of one 224 x 224 image
  h, total = 112, 0
  for name, cin, inner, cout, stride, has_expand, residual in R.blocks(1.0)[1]:
    total += inner * h * h if has_expand else 0
    h = -(-h // stride)
  assert total == 3339840


def _values(names_shapes, seed=5):
  rng = np.random.RandomState(seed)
  vals = {}
  for name, shape in names_shapes:
    leaf = name.rsplit('/', 1)[1]
    if leaf in ('weights', 'depthwise_weights'):
      fan_in = shape[0] * shape[1] * (shape[2] if leaf == 'weights' else 1)
      v = rng.randn(*shape) * np.sqrt(2.0 / fan_in)
    elif leaf in ('gamma', 'moving_variance'):
      v = rng.rand(*shape) + 0.5
    else:
      v = rng.randn(*shape) * 0.1
    vals['model/' + name] = v.astype(np.float32)
  return vals


def _dist(a, b):
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  return float(np.abs(a - b).max() / np.abs(b).max())


def _first_1x1_block(size):
  """Index of the first block whose depthwise OUTPUT is a 1 x 1 map for a size x size image (None: there is none)."""
  h = -(-size // 2)
  for index, (name, cin, inner, cout, stride, has_expand, residual) in enumerate(R.blocks(0.5)[1]):
    h = -(-h // stride)
    if h == 1:
      return index
  return None


@pytest.mark.parametrize('batch,size,training', [(2, 32, True), (2, 32, False), (8, 64, True)])
def test_forward_of_the_composition_against_the_float64_restatement(monkeypatch, batch, size, training):
  """Multiplier 0.5, 11 classes, on the CPU composition (library convolutions, emulated BN passes) against the float64 restatement.
  The bar is the distance of ONE float32 run of the same restatement (the plain one) to its float64 run, times 2: the executor is
  another float32 evaluation of the same function in another operation order (BN folded to scale / shift), and two such evaluations
  are held to d_a <= 2 d_b throughout this project.  (A factor of 1 would be a coin flip between two orderings of equal accuracy:
  over input seeds 7, 8, 9 the executor's distance is 0.4 to 1.7 times the plain run's, and a reordered float32 run of the
  restatement itself 0.7 to 2.6 times.)  Every compared quantity must also sit at float32 rounding level, below 1e-4.
  What is compared: the logits -- except in TRAINING mode at 32 x 32 and batch 2, where the last five BatchNorms see 1 x 1 maps, two
  values per channel, and x -> d / sqrt(d * d + eps) amplifies rounding by up to 1 / sqrt(eps) = 31.6 per layer: there the plain
  float32 run itself is 0.198 from float64 (executor 0.436) and the logits check nothing.  That case compares the last
  well-conditioned tensor instead, the depthwise output of block 13 in front of the first 1 x 1-map BatchNorm (13 blocks, 40
  training-mode BatchNorms and 4 residuals deep; measured 3.1e-5 against 2.0e-5), and asks only finiteness of the logits; the layers
  behind it are checked by the inference case (moving statistics) and by the 64 x 64 / batch 8 training case, whose smallest map is
  2 x 2 (measured: executor 2.0e-5, plain float32 run 1.2e-5; inference 2.5e-6 against 3.3e-6)."""
  from pocketflow_amd import graph as G
  fake = FakeHipFull()
  monkeypatch.setattr(G, 'hip', fake)
  g, net = _build(G, 0.5, num_classes=11)
  g.finalize(seed=1, requires_grad=training)
  vals = _values(R.var_list(0.5, 11))
  g.store.load_numpy(vals, strict=True)
  images = np.random.RandomState(7).randn(batch, 3, size, size).astype(np.float32)
  x = torch.from_numpy(images).contiguous(memory_format=torch.channels_last)
  cut = _first_1x1_block(size) if training else None
  assert cut == (13 if (training and size == 32) else None)
  fake.minmax_slots_init(g.act_slots)
  with g.as_default():
    if cut is not None:
      g.training = True
      y = net.stem_bn(net.stem(x))
      for blk in net.blocks[:cut]:
        y = blk(y)
      blk = net.blocks[cut]
      got = blk.depthwise(blk.expand_bn(blk.expand(y, want_stats=True)), want_stats=True)
      g.store.load_numpy(vals, strict=True)                      # (the moving statistics as they were)
      logits = net(x, True)
      assert tuple(logits.shape) == (batch, 11) and bool(torch.isfinite(logits).all())
    elif training:
      got = net(x, True)
    else:
      with torch.no_grad():
        got = net(x, False)
  ref64 = R.forward(vals, images, 0.5, training, raw_depthwise_of=cut).numpy()
  ref32 = R.forward(vals, images, 0.5, training, dtype=torch.float32, raw_depthwise_of=cut).numpy()
  assert tuple(got.shape) == ref64.shape == ((batch, 11) if cut is None else (batch, 288, 1, 1))
  d_net, d_f32 = _dist(got.detach().numpy(), ref64), _dist(ref32, ref64)
  print('batch %d, %d x %d, training=%s, %s: executor against float64 %.3e, float32 run of the restatement %.3e'
        % (batch, size, size, training, 'logits' if cut is None else 'depthwise output of block %d' % cut, d_net, d_f32))
  assert d_f32 < 1e-4 and d_net < 1e-4                        # float32 rounding level
  assert d_net <= 2.0 * d_f32, (d_net, d_f32)
  assert 'bn_add_act_fwd' not in fake.calls                   # the composition: BatchNormAct, torch add


def test_forward_check_sees_a_dropped_activation(monkeypatch):
  """The comparison above is a real one: the same network with ONE late ReLU6 left out (block 12's expansion) misses the bar of the
  inference case by orders."""
  from pocketflow_amd import graph as G
  fake = FakeHipFull()
  monkeypatch.setattr(G, 'hip', fake)
  g, net = _build(G, 0.5, num_classes=11)
  g.finalize(seed=1, requires_grad=False)
  vals = _values(R.var_list(0.5, 11))
  g.store.load_numpy(vals, strict=True)
  images = np.random.RandomState(7).randn(2, 3, 32, 32).astype(np.float32)
  net.blocks[12].expand_bn.act = None
  fake.minmax_slots_init(g.act_slots)
  with torch.no_grad(), g.as_default():
    got = net(torch.from_numpy(images).contiguous(memory_format=torch.channels_last), False)
  ref64 = R.forward(vals, images, 0.5, False).numpy()
  ref32 = R.forward(vals, images, 0.5, False, dtype=torch.float32).numpy()
  assert _dist(got.numpy(), ref64) > 100.0 * 2.0 * _dist(ref32, ref64)


def test_learning_rate_schedules(monkeypatch):
  from pocketflow_amd.flags import FLAGS
  import pocketflow_amd.nets.mobilenet_at_ilsvrc12 as net
  import pocketflow_amd.datasets.abstract_dataset  # noqa: F401
  vals, explicit = dict(FLAGS._vals), set(FLAGS._explicit)
  try:
    FLAGS.batch_size, FLAGS.nb_smpls_train, FLAGS.enbl_multi_gpu = 96, 1281167, False
    FLAGS.lrn_rate_init, FLAGS.batch_size_norm, FLAGS.nb_epochs_rat = 0.045, 96, 1.0
    mh = object.__new__(net.ModelHelper)
    FLAGS.mobilenet_version = 2
    lr, iters = mh.setup_lrn_rate(0)
    assert iters == int(1281167 * 412 * 1.0 / 96)
    batch_step = int(1281167 * 2.5 / 96)
    for step in (0, 1, batch_step - 1, batch_step, 7 * batch_step + 3, iters - 1):
      want = 0.045 * 96 / 96 * (0.98 ** 2.5) ** (step // batch_step)       # the reference's staircase exponential decay
      assert lr(step) == pytest.approx(want, rel=1e-12), step
    FLAGS.mobilenet_version = 1                                # unchanged: 100 epochs, x 0.1 at 30 / 60 / 80 / 90
    lr1, iters1 = mh.setup_lrn_rate(0)
    assert iters1 == int(1281167 * 100 / 96)
    per_epoch = 1281167 / 96
    for epoch, want in ((0, 0.045), (29, 0.045), (31, 0.0045), (61, 0.00045), (81, 0.000045), (95, 0.0000045)):
      assert lr1(int(epoch * per_epoch)) == pytest.approx(want, rel=1e-9), epoch
    FLAGS.mobilenet_version = 3
    with pytest.raises(ValueError, match='invalid MobileNet version: 3'):
      mh.setup_lrn_rate(0)
    with pytest.raises(ValueError, match='invalid MobileNet version: 3'):
      net.forward_fn(torch.zeros(1, 3, 8, 8), True)
  finally:
    FLAGS._vals.clear()
    FLAGS._vals.update(vals)
    FLAGS._explicit.clear()
    FLAGS._explicit.update(explicit)


def _join_run(monkeypatch, fake, any_device, two_consumers):
  """conv-free harness: y = join(x, s) with x, s leaves; the output read once or twice (through the `_pf_skip` alias)."""
  from pocketflow_amd import graph as G
  monkeypatch.setattr(G, 'hip', fake)
  monkeypatch.setattr(G, 'BN_JOIN_ANY_DEVICE', any_device)
  g = G.Graph('model', 'cpu', torch.float32)
  join = G.BatchNormAddAct(g, 'blk/project/BatchNorm', 16, None, 0.997, 1e-3, l2=True, beta_first=True)
  assert join.op is None and g.activation_ops == [] and g.join_layers == [join]
  g.finalize(seed=1, requires_grad=True)
  rng = np.random.RandomState(3)
  g.store.load_numpy({'model/blk/project/BatchNorm/gamma': rng.rand(16).astype(np.float32) + 0.5,
                      'model/blk/project/BatchNorm/beta': rng.randn(16).astype(np.float32)}, strict=False)
  x = torch.from_numpy(rng.randn(2, 16, 5, 3).astype(np.float32)).contiguous(memory_format=torch.channels_last).requires_grad_(True)
  s = torch.from_numpy(rng.randn(2, 16, 5, 3).astype(np.float32)).contiguous(memory_format=torch.channels_last).requires_grad_(True)
  w1 = torch.from_numpy(rng.randn(2, 16, 5, 3).astype(np.float32))
  w2 = torch.from_numpy(rng.randn(2, 16, 5, 3).astype(np.float32))
  g.training = True
  with g.as_default():
    u = join(x, s)
  loss = (u * w1).sum()
  if two_consumers:
    loss = loss + (getattr(u, '_pf_skip', u) * w2).sum()
  loss.backward()
  return dict(u=u.detach().clone(), dx=x.grad.clone(), ds=s.grad.clone(), o_grad=g.store.o_grad.clone(), calls=dict(fake.calls),
              want_ds=w1 + w2 if two_consumers else w1)


@pytest.mark.parametrize('two_consumers', [False, True])
def test_activation_free_join_on_emulated_kernels(monkeypatch, two_consumers):
  """BatchNormAddAct(act=None): no op registered; forward on pf_bn_add_act_fwd(act none); the shortcut receives the arriving gradient
  (the sum of the two aliases') unchanged; one reader: no gate launch at all, two: the ADD form; values as the composition's."""
  fused = _join_run(monkeypatch, V2FakeHip(), True, two_consumers)
  comp = _join_run(monkeypatch, FakeHipFull(), False, two_consumers)
  assert fused['calls'].get('bn_add_act_fwd') == 1 and 'bn_add_act_fwd' not in comp['calls']
  assert fused['calls'].get('bn_add_act_bwd_gate', 0) == 0
  assert fused['calls'].get('bn_add_act_bwd_gate_add', 0) == (1 if two_consumers else 0)
  assert fused['calls'].get('bn_bwd_stats', 0) == (0 if two_consumers else 1)
  assert torch.equal(fused['ds'], fused['want_ds'])            # the shortcut's gradient: g as it stands
  torch.testing.assert_close(fused['u'], comp['u'], rtol=1e-6, atol=1e-6)
  torch.testing.assert_close(fused['dx'], comp['dx'], rtol=1e-5, atol=1e-6)
  torch.testing.assert_close(fused['ds'], comp['ds'], rtol=0, atol=0)
  torch.testing.assert_close(fused['o_grad'], comp['o_grad'], rtol=1e-5, atol=1e-5)


def test_lazy_depthwise_route_on_emulated_kernels(monkeypatch):
  """The plumbing of the `lazy` route on float32 CPU tensors: with the switch on the expansion BN stays un-materialised, the depthwise
  layer runs the two fused entries and no apply pass runs for that BN; logits and every gradient equal the materialised route's."""
  from pocketflow_amd import graph as G
  runs = {}
  for lazy in (True, False):
    fake = V2FakeHip()
    monkeypatch.setattr(G, 'hip', fake)
    monkeypatch.setattr(G, 'DEPTHWISE_ANY_DEVICE', True)
    monkeypatch.setattr(G, 'BN_JOIN_ANY_DEVICE', True)
    monkeypatch.setattr(G, 'DW_LAZY', lazy)
    g, net = _build(G, 0.5, num_classes=11)
    g.finalize(seed=1, requires_grad=True)
    g.store.load_numpy(_values(R.var_list(0.5, 11)), strict=True)
    for op in g.activation_ops:
      op.bits = 8
    fake.minmax_slots_init(g.act_slots)
    x = torch.from_numpy(np.random.RandomState(7).randn(2, 3, 32, 32).astype(np.float32)).contiguous(memory_format=torch.channels_last)
    with g.as_default():
      out = net(x, True)
    (out * torch.from_numpy(np.random.RandomState(9).randn(2, 11).astype(np.float32))).sum().backward()
    runs[lazy] = dict(out=out.detach().clone(), w=g.store.w_grad.clone(), o=g.store.o_grad.clone(), calls=dict(fake.calls))
  on, off = runs[True]['calls'], runs[False]['calls']
  assert on.get('depthwise_fwd_act') == 17 == on.get('depthwise_wrw_act') and on.get('depthwise_fwd', 0) == 0 == on.get('depthwise_wrw', 0)
  assert off.get('depthwise_fwd') == 17 == off.get('depthwise_wrw') and 'depthwise_fwd_act' not in off
  assert off['bn_apply'] - on['bn_apply'] == 17
  assert on['depthwise_bwd_data'] == off['depthwise_bwd_data'] == 17
  for k in ('out', 'w', 'o'):
    assert torch.equal(runs[True][k], runs[False][k]), k


@pytest.mark.parametrize('lazy', [False, True])
def test_finished_steps_leave_no_tensor_alive(monkeypatch, lazy):
  """As tests/test_fused_plumbing_cpu.py asks of the other networks: with the cyclic collector off, steps of the network on the join
  and lazy-depthwise plumbing must not grow the set of live tensors.  (The join node used to return its output and a VIEW of it, and the
  layer hung the view on the output as `_pf_skip`: a cycle through the view's base that no collector sees.  At batch 256 every step's
  block outputs stayed allocated and the device ran out of memory after some thirty steps.)"""
  import gc
  from pocketflow_amd import graph as G
  fake = V2FakeHip()
  monkeypatch.setattr(G, 'hip', fake)
  monkeypatch.setattr(G, 'DEPTHWISE_ANY_DEVICE', True)
  monkeypatch.setattr(G, 'BN_JOIN_ANY_DEVICE', True)
  monkeypatch.setattr(G, 'DW_LAZY', lazy)
  g, net = _build(G, 0.5, num_classes=11)
  g.finalize(seed=1, requires_grad=True)
  g.begin_step = lambda: None
  fake.minmax_slots_init(g.act_slots)
  x = torch.randn(2, 3, 32, 32).contiguous(memory_format=torch.channels_last)
  wts = torch.randn(2, 11)

  def step():
    with g.as_default():
      logits = net(x, True)
    (logits * wts).sum().backward()
    g.store.zero_grad()

  def live_tensor_bytes():
    return sum(o.numel() * o.element_size() for o in gc.get_objects() if isinstance(o, torch.Tensor))
  step()
  gc.collect()
  gc.disable()
  try:
    step()
    base = live_tensor_bytes()
    for _ in range(3):
      step()
    grown = live_tensor_bytes() - base
  finally:
    gc.enable()
  assert fake.calls.get('bn_add_act_fwd', 0) > 0 and (fake.calls.get('depthwise_fwd_act', 0) > 0) == lazy
  assert grown <= 0, 'tensors of finished steps are still alive without the cyclic collector: +%d bytes' % grown


def test_relu_join_leaves_no_tensor_alive(monkeypatch):
  """The same for the join WITH its ReLU, the tail of the ResNet-v1 bottleneck blocks, where the cycle was found too: two joins in a
  row, the second reading both aliases of the first one's output."""
  import gc
  from pocketflow_amd import graph as G
  fake = V2FakeHip()
  monkeypatch.setattr(G, 'hip', fake)
  monkeypatch.setattr(G, 'BN_JOIN_ANY_DEVICE', True)
  g = G.Graph('model', 'cpu', torch.float32)
  j1 = G.BatchNormAddAct(g, 'j1', 16, 'Relu', 0.9, 1e-3, act_name='j1/Relu')
  j2 = G.BatchNormAddAct(g, 'j2', 16, 'Relu', 0.9, 1e-3, act_name='j2/Relu')
  g.finalize(seed=1, requires_grad=True)
  g.training = True
  fake.minmax_slots_init(g.act_slots)
  x = torch.randn(2, 16, 8, 8).contiguous(memory_format=torch.channels_last)

  def step():
    xi = x.clone().requires_grad_(True)
    with g.as_default():
      u = j1(xi * 2.0, xi * 3.0)
      assert hasattr(u, '_pf_skip')
      v = j2(u, u._pf_skip)
    v.sum().backward()
    g.store.zero_grad()

  def live_tensor_bytes():
    return sum(o.numel() * o.element_size() for o in gc.get_objects() if isinstance(o, torch.Tensor))
  step()
  gc.collect()
  gc.disable()
  try:
    step()
    base = live_tensor_bytes()
    for _ in range(3):
      step()
    grown = live_tensor_bytes() - base
  finally:
    gc.enable()
  assert fake.calls.get('bn_add_act_bwd_gate_add', 0) > 0
  assert grown <= 0, 'tensors of finished steps are still alive without the cyclic collector: +%d bytes' % grown
