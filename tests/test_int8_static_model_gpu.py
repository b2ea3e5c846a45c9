"""Whole quantised models with FIXED activation ranges: the artefact of tools/conversion/export_quant_int8_model.py, calibrated over two
evaluation batches (calibrate_act_ranges), loaded with inference.load_int8(act_ranges='static') on the float kernels ('off'), with
the Conv2D layers on codes ('on') and with the depthwise layers on codes as well; and tools/benchmark/calc_inference_time end to end.

Setup is that of tests/test_int8_mobilenet_gpu.py (MobileNet-v1 0.5 at 64 x 64, batch 4, bf16) and tests/test_int8_model_gpu.py
(ResNet-20 at CIFAR size).  The bar is theirs: with d = max |logit - logit64| / max |logit64| against a float64 forward of the same
network -- written here, with the static, clamping quantiser on the artefact's ranges -- a route on codes may be twice as far from
it as the static float route is: d_static_on <= 2 d_static_off.  The distances are printed; measured lines are kept in
profiles/int8_model_parity.txt."""
import importlib
import json
import os
from unittest import mock

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BATCH = 4
_ARTEFACTS = {}


@pytest.fixture(autouse=True)
def _restore_flags():
  """The flag registry is one per process: leave it as it was found."""
  from pocketflow_amd.flags import FLAGS
  vals, explicit = dict(FLAGS._vals), set(FLAGS._explicit)
  yield
  FLAGS._vals.clear()
  FLAGS._vals.update(vals)
  FLAGS._explicit.clear()
  FLAGS._explicit.update(explicit)


def _setup(tmp_path_factory, net):
  """Flags for `net` ('mobilenet': MobileNet-v1 0.5, 64 x 64, batch 4; 'resnet20': ResNet-20 at CIFAR size, batch 16), bf16, 8 / 8
  bits, tensor buckets, and -- once per net -- a synthetic checkpoint exported through the UniformQuantLearner and calibrated over two
  evaluation batches.  Returns (model helper, path of model_int8.npz, batch size, keys of the file before calibration)."""
  from pocketflow_amd.flags import FLAGS
  import pocketflow_amd.learners.learner_utils  # noqa: F401
  import pocketflow_amd.learners.abstract_learner  # noqa: F401
  import pocketflow_amd.learners.uniform_quantization.learner  # noqa: F401
  mod = importlib.import_module('pocketflow_amd.nets.' + ('mobilenet_at_ilsvrc12' if net == 'mobilenet' else 'resnet_at_cifar10'))
  if net not in _ARTEFACTS:
    _ARTEFACTS[net] = [str(tmp_path_factory.mktemp('static_' + net)), None, None]
  root = _ARTEFACTS[net][0]
  batch = BATCH if net == 'mobilenet' else 16
  FLAGS.save_path = os.path.join(root, 'models', 'model.ckpt')
  FLAGS.uql_save_quant_model_path = os.path.join(root, 'uql', 'model.ckpt')
  FLAGS.synthetic_pool, FLAGS.nb_eval_batches_override = 2, 2
  FLAGS.uql_weight_bits = FLAGS.uql_activation_bits = 8
  FLAGS.batch_size = FLAGS.batch_size_eval = batch
  FLAGS.compute_dtype, FLAGS.uql_use_buckets, FLAGS.uql_bucket_type = 'bfloat16', False, 'channel'
  if net == 'mobilenet':
    FLAGS.mobilenet_version, FLAGS.mobilenet_depth_mult, FLAGS.nb_classes, FLAGS.image_size = 1, 0.5, 1001, 64
  else:
    FLAGS.resnet_size, FLAGS.nb_classes = 20, 10
  mh = mod.ModelHelper()
  if _ARTEFACTS[net][1] is None:
    from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
    from pocketflow_amd.learners.uniform_quantization.learner import UniformQuantLearner
    from pocketflow_amd.tools.conversion import export_quant_int8_model as E
    from pocketflow_amd.utils import checkpoint
    create_synthetic_checkpoint(mh)
    learner = UniformQuantLearner(None, mh)
    learner.restore_vars(checkpoint.latest_checkpoint(os.path.dirname(FLAGS.save_path)))
    path = os.path.join(root, 'uql', 'model_int8.npz')
    E.export_from_learner(learner, path)
    del learner
    torch.cuda.empty_cache()
    keys = sorted(np.load(path).files)
    assert not any(key.endswith('/act_range') for key in keys)         # written without calibration: the key set it always had
    ranges = E.calibrate_act_ranges(mh, path, 2, 8, 'cuda', torch.bfloat16)
    assert ranges == E.load_act_ranges(path) and len(ranges) >= 1
    _ARTEFACTS[net][1], _ARTEFACTS[net][2] = path, keys
  return mh, _ARTEFACTS[net][1], batch, _ARTEFACTS[net][2]


def forward64(graph, mh, images, bits, ranges):
  """float64 forward of `graph`'s network on its float32 master variables (the decoded kernels), every activation quantised by the
  STATIC quantiser on the artefact's range of its op: t = clip((y - min) / ((max - min) + 1e-10) * k, 0, k), round half to even.  The
  network structure is the product's own forward_eval."""
  import pocketflow_amd.graph as G
  k = float(2 ** bits - 1)

  def same(x, ksz, stride):
    ph, pw = G._same_pads(x.shape[2], ksz, stride), G._same_pads(x.shape[3], ksz, stride)
    return F.pad(x, (pw[0], pw[1], ph[0], ph[1]))

  def conv(self, x, residual=None, want_stats=False, out_bn=None):
    x = x.double()
    pad = 0
    if isinstance(self.padding, int):
      pad = self.padding
    elif self.padding == 'SAME' and self.k > 1:
      x = same(x, self.k, self.stride)
    w = self.kernel.master.detach().double().permute(0, 3, 1, 2)
    b = self.bias.tensor.detach().double() if self.bias is not None else None
    y = F.conv2d(x, w, b, stride=self.stride, padding=pad)
    return y if residual is None else y + residual.double()

  def depthwise(self, x, want_stats=False, out_bn=None):
    w = self.kernel.master.detach().double().view(self.channels, 1, self.k, self.k)
    return F.conv2d(same(x.double(), self.k, self.stride), w, None, stride=self.stride, groups=self.channels)

  def dense(self, x):
    return F.linear(x.double(), self.kernel.master.detach().double(), self.bias.tensor.detach().double())

  def bn(self, x, with_skip=False):
    v = lambda t: t.detach().double().view(1, -1, 1, 1)
    y = (x.double() - v(self.moving_mean.tensor)) / torch.sqrt(v(self.moving_var.tensor) + self.eps) * v(self.gamma.tensor) + v(self.beta.tensor)
    if self.act is not None:
      y = torch.relu(y) if self.act == 'Relu' else torch.clamp(y, 0, 6)
      mn, mx = ranges[self.op.name]
      alpha = (float(np.float32(mx)) - float(np.float32(mn))) + 1e-10
      y = alpha * (torch.round(torch.clamp((y - mn) / alpha * k, 0.0, k)) / k) + mn          # torch.round: half to even
    return (y, x) if with_skip else y

  with mock.patch.object(G.Conv2D, '__call__', conv), mock.patch.object(G.DepthwiseConv2D, '__call__', depthwise), \
      mock.patch.object(G.Dense, '__call__', dense), mock.patch.object(G.BatchNormAct, '__call__', bn), \
      mock.patch.object(G.BatchNormAct, 'pooled', lambda self, x: None), torch.no_grad(), graph.as_default():
    return mh.forward_eval(G.to_device_images(images, graph).double())


def _dist(a, ref):
  return float((a.double() - ref).abs().max()) / float(ref.abs().max())


def _two_batches(mh, batch):
  a, _ = mh.dataset_train.make_batch(np.random.RandomState(5), batch)
  b, _ = mh.dataset_train.make_batch(np.random.RandomState(6), batch)
  return np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32) * np.float32(0.5)


def test_static_slots_hold_the_artefacts_ranges_and_no_forward_touches_them(tmp_path_factory):
  from pocketflow_amd.inference import load_int8
  from pocketflow_amd.tools.conversion import export_quant_int8_model as E
  mh, path, batch, keys_before = _setup(tmp_path_factory, 'mobilenet')
  g, fwd = load_int8(mh, path, 'cuda', torch.bfloat16, 8, int8='on', depthwise='on', act_ranges='static')
  ranges = E.load_act_ranges(path)
  ops = [op for op in g.activation_ops if op.type in ('Relu', 'Relu6')]
  assert sorted(ranges) == sorted(op.name for op in ops) and len(ops) == 27
  assert sorted(set(np.load(path).files) - set(keys_before)) == sorted(n + '/act_range' for n in ranges)
  slots0 = g.act_slots.clone()
  mn, mx = E.decode_slots(slots0.cpu().numpy())
  for op in ops:
    assert (mn[op.index], mx[op.index]) == tuple(np.float32(v) for v in ranges[op.name]), op.name
  ab = g.act_static.cpu().numpy()
  assert np.array_equal(ab[:, 1], mn) and np.array_equal(ab[:, 0], (mx - mn).astype(np.float32) + np.float32(1e-10))
  a, b = _two_batches(mh, batch)
  ya, yb = fwd(a), fwd(b)
  torch.cuda.synchronize()
  assert torch.equal(g.act_slots, slots0) and not torch.equal(ya, yb)
  # per-batch ranges, the default: the slots follow the batch
  g_b, fwd_b = load_int8(mh, path, 'cuda', torch.bfloat16, 8, int8='on', depthwise='on')
  assert g_b.act_static is None
  fwd_b(a)
  sa = g_b.act_slots.clone()
  fwd_b(b)
  torch.cuda.synchronize()
  assert not torch.equal(sa, g_b.act_slots) and len(g_b.requant_ran) == 0


def test_static_mobilenet_launch_structure_determinism_and_parity(tmp_path_factory):
  from pocketflow_amd.inference import load_int8
  from pocketflow_amd.tools.conversion import export_quant_int8_model as E
  mh, path, batch, _ = _setup(tmp_path_factory, 'mobilenet')
  images, _ = _two_batches(mh, batch)
  ranges = E.load_act_ranges(path)
  g_off, fwd_off = load_int8(mh, path, 'cuda', torch.bfloat16, 8, int8='off', act_ranges='static')
  g_pw, fwd_pw = load_int8(mh, path, 'cuda', torch.bfloat16, 8, int8='on', act_ranges='static')
  g_on, fwd_on = load_int8(mh, path, 'cuda', torch.bfloat16, 8, int8='on', depthwise='on', act_ranges='static')
  ref = forward64(g_off, mh, images, 8, ranges)
  off, pw, on = fwd_off(images), fwd_pw(images), fwd_on(images)
  torch.cuda.synchronize()
  assert torch.isfinite(on).all() and torch.isfinite(off).all() and torch.isfinite(pw).all()
  assert torch.equal(on, fwd_on(images)) and torch.equal(off, fwd_off(images)) and torch.equal(pw, fwd_pw(images))
  # launch structure: every depthwise layer and every pointwise layer in front of one requantised in its own epilogue
  dw_names = {dw.kernel.name for dw in g_on.depthwise_layers}
  pw_before_dw = {net_layer.kernel.name for net_layer in g_on.conv_layers if net_layer.k == 1 and 'pointwise' in net_layer.kernel.name
                  and 'Conv2d_13_' not in net_layer.kernel.name}
  assert len(dw_names) == 13 and len(pw_before_dw) == 12
  assert dw_names <= g_on.requant_ran and pw_before_dw <= g_on.requant_ran
  assert g_on.requant_ran <= g_on.int8_ran and len(g_on.int8_ran) == g_on.nb_int8
  assert g_off.nb_int8 == 0 and not g_off.requant_ran and not g_off.int8_ran
  assert not (dw_names & g_pw.int8_ran) and len(g_pw.int8_ran) == g_pw.nb_int8 >= 1
  d_off, d_pw, d_on = _dist(off, ref), _dist(pw, ref), _dist(on, ref)
  print('mobilenet_at_ilsvrc12 0.5 bf16 tensor buckets, STATIC ranges: %d int8 layers, %d requantising; static float path vs float64 %.3e; '
        'static int8 pointwise only vs float64 %.3e; static int8 with depthwise vs float64 %.3e; with depthwise vs static float path %.3e'
        % (g_on.nb_int8, len(g_on.requant_ran), d_off, d_pw, d_on, _dist(on, off.double())))
  assert d_on <= 2.0 * d_off, (d_on, d_off)
  assert d_pw <= 2.0 * d_off, (d_pw, d_off)


def test_static_resnet20_requantises_behind_the_int8_convolution(tmp_path_factory):
  from pocketflow_amd.inference import load_int8
  from pocketflow_amd.tools.conversion import export_quant_int8_model as E
  mh, path, batch, _ = _setup(tmp_path_factory, 'resnet20')
  images, other = _two_batches(mh, batch)
  ranges = E.load_act_ranges(path)
  g_off, fwd_off = load_int8(mh, path, 'cuda', torch.bfloat16, 8, int8='off', act_ranges='static')
  g_on, fwd_on = load_int8(mh, path, 'cuda', torch.bfloat16, 8, int8='on', act_ranges='static')
  slots0 = g_on.act_slots.clone()
  ref = forward64(g_off, mh, images, 8, ranges)
  off, on = fwd_off(images), fwd_on(images)
  fwd_on(other)
  torch.cuda.synchronize()
  assert torch.equal(g_on.act_slots, slots0)
  assert torch.isfinite(on).all() and torch.isfinite(off).all()
  assert torch.equal(on, fwd_on(images)) and torch.equal(off, fwd_off(images))
  assert g_on.nb_int8 >= 1 and len(g_on.int8_ran) == g_on.nb_int8
  # conv1 of every block hands bn2 to its epilogue (out_bn behind pf_conv_i8_fwd_q): 9 blocks
  assert len(g_on.requant_ran) == 9 and g_on.requant_ran <= g_on.int8_ran
  d_off, d_on = _dist(off, ref), _dist(on, ref)
  print('resnet_at_cifar10 20 bf16 tensor buckets, STATIC ranges: %d int8 layers, %d requantising; static float path vs float64 %.3e; '
        'static int8 path vs float64 %.3e; int8 vs static float path %.3e'
        % (g_on.nb_int8, len(g_on.requant_ran), d_off, d_on, _dist(on, off.double())))
  assert d_on <= 2.0 * d_off, (d_on, d_off)


def test_static_needs_ranges_and_a_packed_layer_still_raises_with_gradients(tmp_path_factory, tmp_path):
  from pocketflow_amd.inference import load_int8
  mh, path, batch, keys_before = _setup(tmp_path_factory, 'mobilenet')
  z = dict(np.load(path))
  bare = str(tmp_path / 'bare.npz')
  np.savez(bare, **{k: v for k, v in z.items() if k in keys_before})
  with pytest.raises(ValueError, match='bare.npz'):
    load_int8(mh, bare, 'cuda', torch.bfloat16, 8, int8='on', act_ranges='static')
  g_bare, fwd_bare = load_int8(mh, bare, 'cuda', torch.bfloat16, 8, int8='on')                    # without the keyword: as before
  g_full, fwd_full = load_int8(mh, path, 'cuda', torch.bfloat16, 8, int8='on')
  images, _ = _two_batches(mh, batch)
  assert torch.equal(fwd_bare(images), fwd_full(images)) and g_bare.act_static is None
  name = sorted(k for k in z if k.endswith('/act_range'))[3]
  short = str(tmp_path / 'short.npz')
  np.savez(short, **{k: v for k, v in z.items() if k != name})
  with pytest.raises(ValueError, match=name[:-len('/act_range')]):
    load_int8(mh, short, 'cuda', torch.bfloat16, 8, int8='on', act_ranges='static')
  z[name] = np.array([2.0, 1.0], np.float32)
  np.savez(short, **z)
  with pytest.raises(ValueError, match=name[:-len('/act_range')]):
    load_int8(mh, short, 'cuda', torch.bfloat16, 8, int8='on', act_ranges='static')
  with pytest.raises(ValueError, match="'batch' or 'static'"):
    load_int8(mh, path, 'cuda', torch.bfloat16, 8, act_ranges='fixed')
  g, _ = load_int8(mh, path, 'cuda', torch.bfloat16, 8, int8='on', depthwise='on', act_ranges='static')
  dw = next(d for d in g.depthwise_layers if d.int8 is not None)
  x = torch.zeros((2, dw.channels, 8, 8), device='cuda', dtype=torch.bfloat16, requires_grad=True)
  with pytest.raises(RuntimeError, match='inference only'), g.as_default():
    dw(x)
  conv = next(c for c in g.conv_layers if c.int8 is not None)
  x = torch.zeros((2, conv.kernel.ref_shape[2], 8, 8), device='cuda', dtype=torch.bfloat16, requires_grad=True)
  with pytest.raises(RuntimeError, match='inference only'), g.as_default():
    conv(x)


def test_codes_only_activation_still_materialises(tmp_path_factory):
  """A requantising producer's codes, handed to a consumer that refuses them at call time: decoded with alpha * (code / k) + beta in
  float32 and rounded once -- the value the producer would have written as a tensor."""
  import pocketflow_amd.graph as G
  codes = torch.randint(0, 256, (2, 16, 5, 3), dtype=torch.uint8, device='cuda').contiguous(memory_format=torch.channels_last)
  ab = torch.tensor([2.75, 0.125], device='cuda')
  act = G.StaticCodesAct(None, None, 'Relu6', ab, 8, 2 * 5 * 3, 16, codes=codes, dtype=torch.bfloat16)
  q = act.materialize()
  from pocketflow_amd import int8
  want = int8.static_value(codes.cpu().numpy(), 2.75, 0.125, 8)
  assert q.dtype == torch.bfloat16 and q.shape == codes.shape and act.dtype == torch.bfloat16
  assert torch.equal(q.cpu(), torch.from_numpy(want).to(torch.bfloat16))
  assert act.codes()[0] is codes and act.materialize() is q


@pytest.mark.parametrize('shape', [(6, 10), (3, 24, 5, 7), (40,)], ids=['dense', 'nhwc', 'vector'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_stand_alone_activation_of_any_rank_takes_the_static_pass(shape, dtype):
  """A quantising `Activation` on a graph with fixed ranges (LeNet's ReLU behind a Dense layer is 2-D): whatever the rank, the slots
  are bit-identical after the call, the range does not follow the data, and the output is static_value(static_codes(relu(x))) on
  the fixed range -- which lies inside the data, so both ends clamp."""
  import pocketflow_amd.graph as G
  from pocketflow_amd import hip, int8
  g = G.Graph('model', 'cuda', dtype)
  other = G.Activation(g, 'relu_a', 'Relu')
  act = G.Activation(g, 'relu_b', 'Relu')
  other.op.bits = act.op.bits = 8
  g.act_slots = torch.empty((2, 2), dtype=torch.int32, device='cuda')
  hip.minmax_slots_init(g.act_slots)
  lo, hi = 0.25, 1.5
  hip.minmax_tensor(torch.tensor([lo, hi], device='cuda'), g.act_slots[act.op.index], None)
  hip.minmax_tensor(torch.tensor([0.0, 9.0], device='cuda'), g.act_slots[other.op.index], None)
  g.act_static = g.act_alpha_beta()
  slots0 = g.act_slots.clone()
  gen = torch.Generator(device='cuda').manual_seed(len(shape))
  alpha, beta = int8.range_alpha_beta(lo, hi)
  for scale in (2.0, 40.0):                                            # the second batch would widen a per-batch range
    x = (torch.randn(shape, device='cuda', generator=gen) * scale).to(dtype)
    with torch.no_grad(), g.as_default():
      y = act(x)
    torch.cuda.synchronize()
    assert torch.equal(g.act_slots, slots0)
    u = np.maximum(x.float().cpu().numpy(), np.float32(0))
    assert (u < lo).mean() >= 0.05 and (u > hi).mean() >= 0.05
    want = int8.static_value(int8.static_codes(u, alpha, beta, 8), alpha, beta, 8)
    assert y.shape == x.shape and y.dtype == dtype
    assert torch.equal(y.cpu(), torch.from_numpy(want).to(dtype))
    assert float(y.float().min()) == lo and float(y.float().max()) <= hi + 1e-6


def test_calc_inference_time_with_static_ranges(tmp_path_factory, capsys):
  from pocketflow_amd.tools.benchmark import calc_inference_time as T
  _, path, batch, _ = _setup(tmp_path_factory, 'mobilenet')
  common = ['--net', 'mobilenet_at_ilsvrc12', '--mobilenet_depth_mult', '0.5', '--nb_classes', '1001', '--image_size', '64', '--batch_size',
            str(batch), '--compute_dtype', 'bfloat16', '--nb_repts_warmup', '1', '--nb_repts', '2', '--json', '--model_file', path,
            '--uql_activation_bits', '8', '--int8', 'on', '--int8_depthwise', 'on']
  assert T.main(common + ['--act_ranges', 'static']) == 0
  line = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{')][-1])
  assert line['ms_per_batch'] > 0 and line['act_ranges'] == 'static' and line['nb_requant_layers'] == 26
  assert line['nb_int8_layers_ran'] == line['nb_int8_layers']
  assert T.main(common + ['--act_ranges', 'batch']) == 0          # (the flag registry is one per process: say it)
  line = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{')][-1])
  assert line['act_ranges'] == 'batch' and line['nb_requant_layers'] == 0
