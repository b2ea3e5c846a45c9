"""MobileNet-v1 on the int8 route with its depthwise layers on pf_dw_i8_fwd: the artefact of
tools/conversion/export_quant_int8_model.py loaded with inference.load_int8(int8='on', depthwise='on'), against the same artefact
decoded and run on the float kernels ('off'), and tools/benchmark/calc_inference_time end to end.

The bar is the one of tests/test_int8_model_gpu.py: with d = max |logit - logit64| / max |logit64| against a float64 forward of the
same network (written here: that file's forward64 plus a float64 depthwise convolution under 'SAME' pads and the biased logits
layer), the int8 route may be twice as far from it as the existing path is: d_on <= 2 d_off.  Both distances are printed; measured
lines are kept in profiles/int8_model_parity.txt."""
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
  """The flag registry is one per process: leave it as it was found (depth multiplier, image size, --int8_depthwise ...)."""
  from pocketflow_amd.flags import FLAGS
  vals, explicit = dict(FLAGS._vals), set(FLAGS._explicit)
  yield
  FLAGS._vals.clear()
  FLAGS._vals.update(vals)
  FLAGS._explicit.clear()
  FLAGS._explicit.update(explicit)


def _setup(tmp_path_factory, buckets):
  """Flags for MobileNet-v1 0.5 at 64 x 64, batch 4, bf16, and (once per bucket mode) a synthetic checkpoint exported through the
  UniformQuantLearner as tests/test_int8_model_gpu.py::_export does.  Returns (model helper, path of model_int8.npz)."""
  from pocketflow_amd.flags import FLAGS
  import pocketflow_amd.learners.learner_utils  # noqa: F401
  import pocketflow_amd.learners.abstract_learner  # noqa: F401
  import pocketflow_amd.nets.mobilenet_at_ilsvrc12 as net
  import pocketflow_amd.learners.uniform_quantization.learner  # noqa: F401
  if buckets not in _ARTEFACTS:
    _ARTEFACTS[buckets] = [str(tmp_path_factory.mktemp('mobilenet_%s' % ('channel' if buckets else 'tensor'))), None]
  root = _ARTEFACTS[buckets][0]
  FLAGS.save_path = os.path.join(root, 'models', 'model.ckpt')
  FLAGS.uql_save_quant_model_path = os.path.join(root, 'uql', 'model.ckpt')
  FLAGS.synthetic_pool, FLAGS.nb_eval_batches_override = 2, 2
  FLAGS.uql_weight_bits = FLAGS.uql_activation_bits = 8
  FLAGS.batch_size = FLAGS.batch_size_eval = BATCH
  FLAGS.compute_dtype, FLAGS.uql_use_buckets, FLAGS.uql_bucket_type = 'bfloat16', buckets, 'channel'
  FLAGS.mobilenet_version, FLAGS.mobilenet_depth_mult, FLAGS.nb_classes, FLAGS.image_size = 1, 0.5, 1001, 64
  mh = net.ModelHelper()
  if _ARTEFACTS[buckets][1] is None:
    from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
    from pocketflow_amd.learners.uniform_quantization.learner import UniformQuantLearner
    from pocketflow_amd.tools.conversion import export_quant_int8_model as E
    from pocketflow_amd.utils import checkpoint
    create_synthetic_checkpoint(mh)
    learner = UniformQuantLearner(None, mh)
    learner.restore_vars(checkpoint.latest_checkpoint(os.path.dirname(FLAGS.save_path)))
    path = os.path.join(root, 'uql', 'model_int8.npz')
    summ = E.export_from_learner(learner, path)
    assert summ['quantised_tensors'] >= 1
    del learner
    torch.cuda.empty_cache()
    _ARTEFACTS[buckets][1] = path
  return mh, _ARTEFACTS[buckets][1]


def forward64(graph, mh, images, bits):
  """float64 forward of `graph`'s network on its float32 master variables (the decoded kernels), every ReLU6 output quantised as the
  learner quantises activations; the network structure is the product's own forward_eval."""
  import pocketflow_amd.graph as G
  k = float(2 ** bits - 1)

  def same(x, ksz, stride):
    ph, pw = G._same_pads(x.shape[2], ksz, stride), G._same_pads(x.shape[3], ksz, stride)
    return F.pad(x, (pw[0], pw[1], ph[0], ph[1]))

  def conv(self, x, residual=None, want_stats=False, out_bn=None):
    x = x.double()
    if self.padding == 'SAME' and self.k > 1:
      x = same(x, self.k, self.stride)
    w = self.kernel.master.detach().double().permute(0, 3, 1, 2)
    b = self.bias.tensor.detach().double() if self.bias is not None else None
    return F.conv2d(x, w, b, stride=self.stride)

  def depthwise(self, x, want_stats=False):
    w = self.kernel.master.detach().double().view(self.channels, 1, self.k, self.k)
    return F.conv2d(same(x.double(), self.k, self.stride), w, None, stride=self.stride, groups=self.channels)

  def bn(self, x, with_skip=False):
    v = lambda t: t.detach().double().view(1, -1, 1, 1)
    y = (x.double() - v(self.moving_mean.tensor)) / torch.sqrt(v(self.moving_var.tensor) + self.eps) * v(self.gamma.tensor) + v(self.beta.tensor)
    if self.act is not None:
      y = torch.relu(y) if self.act == 'Relu' else torch.clamp(y, 0, 6)
      beta = y.min()
      alpha = (y.max() - beta) + 1e-10
      y = alpha * (torch.round((y - beta) / alpha * k) / k) + beta          # torch.round: half to even
    return (y, x) if with_skip else y

  with mock.patch.object(G.Conv2D, '__call__', conv), mock.patch.object(G.DepthwiseConv2D, '__call__', depthwise), \
      mock.patch.object(G.BatchNormAct, '__call__', bn), mock.patch.object(G.BatchNormAct, 'pooled', lambda self, x: None), \
      torch.no_grad(), graph.as_default():
    return mh.forward_eval(G.to_device_images(images, graph).double())


def _dist(a, ref):
  return float((a.double() - ref).abs().max()) / float(ref.abs().max())


def _images(mh):
  images, _ = mh.dataset_train.make_batch(np.random.RandomState(5), BATCH)
  return np.asarray(images, dtype=np.float32)


@pytest.mark.parametrize('buckets', [False, True], ids=['tensor', 'channel'])
def test_mobilenet_logits_with_depthwise_on_int8(tmp_path_factory, buckets):
  from pocketflow_amd.inference import load_int8
  import pocketflow_amd.graph as G
  mh, path = _setup(tmp_path_factory, buckets)
  images = _images(mh)
  g_off, fwd_off = load_int8(mh, path, 'cuda', torch.bfloat16, 8, int8='off', depthwise='on')          # ignored with int8 = 'off'
  g_pw, fwd_pw = load_int8(mh, path, 'cuda', torch.bfloat16, 8, int8='on')
  g_on, fwd_on = load_int8(mh, path, 'cuda', torch.bfloat16, 8, int8='on', depthwise='on')
  dw_names = {dw.kernel.name for dw in g_on.depthwise_layers}
  assert len(dw_names) == 13 and g_off.nb_int8 == 0
  ref = forward64(g_off, mh, images, 8)
  off, pw, on = fwd_off(images), fwd_pw(images), fwd_on(images)
  torch.cuda.synchronize()
  assert torch.isfinite(on).all() and torch.isfinite(off).all() and torch.isfinite(pw).all()
  assert torch.equal(on, fwd_on(images)) and torch.equal(off, fwd_off(images)) and torch.equal(pw, fwd_pw(images))
  # every depthwise layer took the kernel, and every packed layer met codes
  assert dw_names <= g_on.int8_ran and len(g_on.int8_ran) == g_on.nb_int8 and len(g_off.int8_ran) == 0
  # without the keyword: today's behaviour -- the packed Conv2D layers alone
  nb_conv = sum(c.int8 is not None for c in g_pw.conv_layers)
  assert not (dw_names & g_pw.int8_ran) and all(dw.int8 is None for dw in g_pw.depthwise_layers)
  assert g_pw.nb_int8 == nb_conv >= 1 and len(g_pw.int8_ran) == nb_conv and g_on.nb_int8 == nb_conv + 13
  d_off, d_pw, d_on = _dist(off, ref), _dist(pw, ref), _dist(on, ref)
  print('mobilenet_at_ilsvrc12 0.5 bf16 %s buckets: %d int8 layers (13 depthwise); float path vs float64 %.3e; int8 pointwise only vs '
        'float64 %.3e; int8 with depthwise vs float64 %.3e; int8 with depthwise vs float path %.3e'
        % ('channel' if buckets else 'tensor', g_on.nb_int8, d_off, d_pw, d_on, _dist(on, off.double())))
  assert d_on <= 2.0 * d_off, (d_on, d_off)
  assert isinstance(G.int8_dw_pays(512, 1, torch.bfloat16), bool)


def test_packed_depthwise_raises_with_gradients_and_bad_keyword(tmp_path_factory):
  from pocketflow_amd.inference import load_int8
  mh, path = _setup(tmp_path_factory, False)
  g, _ = load_int8(mh, path, 'cuda', torch.bfloat16, 8, int8='on', depthwise='on')
  dw = next(d for d in g.depthwise_layers if d.int8 is not None)
  x = torch.zeros((2, dw.channels, 8, 8), device='cuda', dtype=torch.bfloat16, requires_grad=True)
  with pytest.raises(RuntimeError, match='inference only'), g.as_default():
    dw(x)
  with pytest.raises(ValueError, match="'auto', 'on' or 'off'"):
    load_int8(mh, path, 'cuda', torch.bfloat16, 8, int8='on', depthwise='yes')
  g_auto, _ = load_int8(mh, path, 'cuda', torch.bfloat16, 8, int8='on', depthwise='auto')
  import pocketflow_amd.graph as G
  want = sum(G.int8_dw_pays(d.channels, d.stride, torch.bfloat16) for d in g_auto.depthwise_layers)
  assert sum(d.int8 is not None for d in g_auto.depthwise_layers) == want


def test_load_int8_names_the_depthwise_variable_it_rejects(tmp_path_factory, tmp_path):
  from pocketflow_amd.inference import load_int8
  mh, path = _setup(tmp_path_factory, False)
  z = dict(np.load(path))
  name = sorted(k for k in z if k.endswith('depthwise_weights/alpha'))[0]
  z[name] = np.concatenate([z[name].reshape(-1), z[name].reshape(-1)])          # two pairs for the one bucket
  bad = str(tmp_path / 'bad.npz')
  np.savez(bad, **z)
  with pytest.raises(ValueError, match=name[:-len('/alpha')]):
    load_int8(mh, bad, 'cuda', torch.bfloat16, 8, int8='on', depthwise='on')


def test_calc_inference_time_with_int8_depthwise(tmp_path_factory, capsys):
  from pocketflow_amd.tools.benchmark import calc_inference_time as T
  _, path = _setup(tmp_path_factory, False)
  common = ['--net', 'mobilenet_at_ilsvrc12', '--mobilenet_depth_mult', '0.5', '--nb_classes', '1001', '--image_size', '64', '--batch_size',
            str(BATCH), '--compute_dtype', 'bfloat16', '--nb_repts_warmup', '1', '--nb_repts', '2', '--json', '--model_file', path,
            '--uql_activation_bits', '8', '--int8', 'on']
  nb = {}
  for mode in ('on', 'off'):
    assert T.main(common + ['--int8_depthwise', mode]) == 0
    line = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{')][-1])
    assert line['ms_per_batch'] > 0 and line['int8'] == 'on' and line['int8_depthwise'] == mode
    assert line['nb_int8_layers_ran'] == line['nb_int8_layers']
    nb[mode] = line['nb_int8_layers']
  assert nb['on'] == nb['off'] + 13
