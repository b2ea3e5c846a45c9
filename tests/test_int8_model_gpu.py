"""Whole quantised models on the int8 route: the artefact of tools/conversion/export_quant_int8_model.py loaded with
inference.load_int8, every eligible convolution on pf_conv_i8_fwd ('on'), against the same artefact decoded and run on the float
kernels ('off', the existing path), and tools/benchmark/calc_inference_time end to end.

The bar is not a constant.  The reference is a float64 torch forward of the same network, written here: the DECODED float32 kernels,
inference-mode BN, and the learner's activation quantiser restated in float64 (per-tensor min / max of the batch, alpha = max - min
+ 1e-10, round half to even).  With d = max |logit - logit64| / max |logit64|, the int8 route may be twice as far from it as the
existing path is: d_on <= 2 d_off, the precedent of tests/test_shrunk_model_gpu.py (one set of rounded sums replaces another; the
integer sums are exact and the kernels are not rounded to bf16, so d_on should come out below d_off).  Both distances are printed;
measured lines are kept in profiles/int8_model_parity.txt."""
import importlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _flags(tmp_path, **kw):
  from pocketflow_amd.flags import FLAGS
  import pocketflow_amd.learners.learner_utils  # noqa: F401
  import pocketflow_amd.learners.abstract_learner  # noqa: F401
  import pocketflow_amd.nets.resnet_at_cifar10  # noqa: F401
  import pocketflow_amd.nets.resnet_at_ilsvrc12  # noqa: F401
  import pocketflow_amd.learners.uniform_quantization.learner  # noqa: F401
  FLAGS.save_path = str(tmp_path / 'models' / 'model.ckpt')
  FLAGS.uql_save_quant_model_path = str(tmp_path / 'uql' / 'model.ckpt')
  FLAGS.synthetic_pool, FLAGS.nb_eval_batches_override = 2, 2
  FLAGS.uql_weight_bits = FLAGS.uql_activation_bits = 8
  for k, v in kw.items():
    setattr(FLAGS, k, v)
  return FLAGS


def _export(tmp_path, mh):
  """A synthetic checkpoint through the UniformQuantLearner, as export_quant_int8_model.main builds it, into model_int8.npz."""
  from pocketflow_amd.flags import FLAGS
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  from pocketflow_amd.learners.uniform_quantization.learner import UniformQuantLearner
  from pocketflow_amd.tools.conversion import export_quant_int8_model as E
  from pocketflow_amd.utils import checkpoint
  create_synthetic_checkpoint(mh)
  learner = UniformQuantLearner(None, mh)
  learner.restore_vars(checkpoint.latest_checkpoint(os.path.dirname(FLAGS.save_path)))
  path = str(tmp_path / 'uql' / 'model_int8.npz')
  summ = E.export_from_learner(learner, path)
  assert summ['quantised_tensors'] >= 1
  del learner
  torch.cuda.empty_cache()
  return path


def forward64(graph, mh, images, bits):
  """float64 forward of `graph`'s network on its float32 master variables (the decoded kernels), every Relu output quantised as the
  learner quantises activations; the network structure is the product's own forward_eval."""
  import pocketflow_amd.graph as G
  from unittest import mock
  k = float(2 ** bits - 1)

  def conv(self, x, residual=None, want_stats=False, out_bn=None):
    x = x.double()
    pad = 0
    if isinstance(self.padding, int):
      pad = self.padding
    elif self.padding == 'SAME' and self.k > 1:
      ph, pw = G._same_pads(x.shape[2], self.k, self.stride), G._same_pads(x.shape[3], self.k, self.stride)
      x = F.pad(x, (pw[0], pw[1], ph[0], ph[1]))
    w = self.kernel.master.detach().double().permute(0, 3, 1, 2)
    y = F.conv2d(x, w, None, stride=self.stride, padding=pad)
    return y if residual is None else y + residual.double()

  def dense(self, x):
    return F.linear(x.double(), self.kernel.master.detach().double(), self.bias.tensor.detach().double())

  def bn(self, x, with_skip=False):
    v = lambda t: t.detach().double().view(1, -1, 1, 1)
    y = (x.double() - v(self.moving_mean.tensor)) / torch.sqrt(v(self.moving_var.tensor) + self.eps) * v(self.gamma.tensor) + v(self.beta.tensor)
    if self.act is not None:
      y = torch.relu(y) if self.act == 'Relu' else torch.clamp(y, 0, 6)
      beta = y.min()
      alpha = (y.max() - beta) + 1e-10
      y = alpha * (torch.round((y - beta) / alpha * k) / k) + beta          # torch.round: half to even
    return (y, x) if with_skip else y

  with mock.patch.object(G.Conv2D, '__call__', conv), mock.patch.object(G.Dense, '__call__', dense), \
      mock.patch.object(G.BatchNormAct, '__call__', bn), mock.patch.object(G.BatchNormAct, 'pooled', lambda self, x: None), \
      torch.no_grad(), graph.as_default():
    return mh.forward_eval(G.to_device_images(images, graph).double())


def _dist(a, ref):
  return float((a.double() - ref).abs().max()) / float(ref.abs().max())


@pytest.mark.parametrize('buckets', [False, True], ids=['tensor', 'channel'])
@pytest.mark.parametrize('net,batch,kw', [
    ('resnet_at_cifar10', 16, dict(resnet_size=20, nb_classes=10)),
    ('resnet_at_ilsvrc12', 4, dict(resnet_size=50, nb_classes=1001, image_size=64))], ids=['resnet20', 'resnet50'])
def test_int8_logits_against_the_float_path(tmp_path, net, batch, kw, buckets):
  from pocketflow_amd.inference import load_int8
  _flags(tmp_path, batch_size=batch, batch_size_eval=batch, compute_dtype='bfloat16', uql_use_buckets=buckets, uql_bucket_type='channel', **kw)
  mh = importlib.import_module('pocketflow_amd.nets.' + net).ModelHelper()
  path = _export(tmp_path, mh)
  images, _ = mh.dataset_train.make_batch(np.random.RandomState(5), batch)
  images = np.asarray(images, dtype=np.float32)
  g_off, fwd_off = load_int8(mh, path, 'cuda', torch.bfloat16, 8, int8='off')
  g_on, fwd_on = load_int8(mh, path, 'cuda', torch.bfloat16, 8, int8='on')
  assert g_off.nb_int8 == 0 and g_on.nb_int8 >= 1
  ref = forward64(g_off, mh, images, 8)
  off, on = fwd_off(images), fwd_on(images)
  torch.cuda.synchronize()
  assert torch.isfinite(on).all() and torch.isfinite(off).all()
  assert torch.equal(on, fwd_on(images)) and torch.equal(off, fwd_off(images))
  assert len(g_off.int8_ran) == 0 and len(g_on.int8_ran) == g_on.nb_int8          # every packed layer met codes
  d_off, d_on = _dist(off, ref), _dist(on, ref)
  print('%s bf16 %s buckets: %d int8 layers; float path vs float64 %.3e; int8 path vs float64 %.3e; int8 vs float path %.3e'
        % (net, 'channel' if buckets else 'tensor', g_on.nb_int8, d_off, d_on, _dist(on, off.double())))
  assert d_on <= 2.0 * d_off, (d_on, d_off)


def test_packed_layer_raises_with_gradients_enabled(tmp_path):
  from pocketflow_amd.inference import load_int8
  import pocketflow_amd.graph as G
  _flags(tmp_path, batch_size=16, batch_size_eval=16, compute_dtype='bfloat16', resnet_size=20, nb_classes=10)
  mh = importlib.import_module('pocketflow_amd.nets.resnet_at_cifar10').ModelHelper()
  g, _ = load_int8(mh, _export(tmp_path, mh), 'cuda', torch.bfloat16, 8, int8='on')
  conv = next(c for c in g.conv_layers if c.int8 is not None)
  x = torch.zeros((2, conv.kernel.ref_shape[2], 8, 8), device='cuda', dtype=torch.bfloat16, requires_grad=True)
  with pytest.raises(RuntimeError, match='inference only'), g.as_default():
    conv(x)
  with pytest.raises(ValueError, match="'auto', 'on' or 'off'"):
    load_int8(mh, str(tmp_path / 'uql' / 'model_int8.npz'), 'cuda', torch.bfloat16, 8, int8='yes')
  assert isinstance(G.int8_pays(1, 256, 64, 1, torch.bfloat16), bool)


def test_load_int8_names_the_variable_it_rejects(tmp_path):
  from pocketflow_amd.inference import load_int8
  _flags(tmp_path, batch_size=16, batch_size_eval=16, compute_dtype='bfloat16', resnet_size=20, nb_classes=10)
  mh = importlib.import_module('pocketflow_amd.nets.resnet_at_cifar10').ModelHelper()
  path = _export(tmp_path, mh)
  z = dict(np.load(path))
  name = sorted(k for k in z if k.endswith('/meta'))[0]
  z[name] = np.concatenate([z[name][:3], [1, 1, 8, 8]])
  bad = str(tmp_path / 'bad.npz')
  np.savez(bad, **z)
  with pytest.raises(ValueError, match=name[:-len('/meta')]):
    load_int8(mh, bad, 'cuda', torch.bfloat16, 8, int8='on')


def test_calc_inference_time_on_the_int8_artefact(tmp_path, capsys):
  from pocketflow_amd.tools.benchmark import calc_inference_time as T
  _flags(tmp_path, batch_size=16, batch_size_eval=16, compute_dtype='bfloat16', resnet_size=20, nb_classes=10)
  mh = importlib.import_module('pocketflow_amd.nets.resnet_at_cifar10').ModelHelper()
  path = _export(tmp_path, mh)
  common = ['--net', 'resnet_at_cifar10', '--resnet_size', '20', '--nb_classes', '10', '--batch_size', '16', '--compute_dtype', 'bfloat16',
            '--nb_repts_warmup', '1', '--nb_repts', '2', '--json', '--model_file', path, '--uql_activation_bits', '8']
  for mode, some in (('on', True), ('off', False)):
    assert T.main(common + ['--int8', mode]) == 0
    line = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{')][-1])
    assert line['ms_per_batch'] > 0 and line['int8'] == mode and (line['nb_int8_layers'] > 0) == some
    assert line['nb_int8_layers_ran'] == line['nb_int8_layers']
