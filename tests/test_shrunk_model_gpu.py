"""Whole shrunk models on the GPU: logits of a `model_shrunk.npz` loaded with inference.load_shrunk (every shrunk layer on
pf_conv_gather.hip) against the same weights in full shape, and tools/benchmark/calc_inference_time end to end.

The bar is not a constant.  Per net the test measures how far the FULL-SHAPE product path (existing code) is from a float64 torch
forward of the same network on the same (compute-dtype-rounded) weights and input, and allows the shrunk path twice that distance to
float64: it replaces one set of rounded sums by another of the same kind.  Distances are max |logit - logit64| / max |logit64|.
Measured on one MI355X (profiles/shrunk_model_parity.txt), full-shape / shrunk: ResNet-20 float32 6.5e-7 / 6.5e-7 (logits bit-identical:
the zero channels add exact zeros in the same order), MobileNet-v1 bf16 1.65e-2 / 1.65e-2, ResNet-50 bf16 3.4e-3 / 3.2e-3, ResNet-20 pruned by
chn-pruned-gpu 2.2e-7 / 2.2e-7.  The test prints both distances."""
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
  import pocketflow_amd.nets.mobilenet_at_ilsvrc12  # noqa: F401
  import pocketflow_amd.nets.resnet_at_ilsvrc12  # noqa: F401
  import pocketflow_amd.learners.channel_pruning_gpu.learner  # noqa: F401
  FLAGS.save_path = str(tmp_path / 'models' / 'model.ckpt')
  FLAGS.save_path_eval = str(tmp_path / 'models_eval' / 'model.ckpt')
  FLAGS.synthetic_pool, FLAGS.nb_eval_batches_override = 2, 2
  for k, v in kw.items():
    setattr(FLAGS, k, v)
  return FLAGS


def forward64(graph, mh, images):
  """float64 torch forward of `graph`'s network: the layer calls replaced by plain float64 torch on the graph's own compute-dtype
  kernels and float32 BN / bias variables; the network structure is the product's own forward_eval."""
  import pocketflow_amd.graph as G
  from unittest import mock

  def conv(self, x, residual=None, want_stats=False, out_bn=None):
    assert self.kernel.gather_host is None
    x = G.materialize(x).double()
    pad = 0
    if isinstance(self.padding, int):
      pad = self.padding
    elif self.padding == 'SAME' and self.k > 1:
      ph, pw = G._same_pads(x.shape[2], self.k, self.stride), G._same_pads(x.shape[3], self.k, self.stride)
      x = F.pad(x, (pw[0], pw[1], ph[0], ph[1]))
    b = self.bias.tensor.detach().double() if self.bias is not None else None
    y = F.conv2d(x, self.kernel.tensor.detach().double(), b, stride=self.stride, padding=pad)
    return y if residual is None else y + residual.double()

  def depthwise(self, x, want_stats=False):
    x = x.double()
    ph, pw = G._same_pads(x.shape[2], self.k, self.stride), G._same_pads(x.shape[3], self.k, self.stride)
    x = F.pad(x, (pw[0], pw[1], ph[0], ph[1]))
    return F.conv2d(x, self.kernel.tensor.detach().double(), None, stride=self.stride, groups=self.channels)

  def dense(self, x):
    return F.linear(x.double(), self.kernel.tensor.detach().double(), self.bias.tensor.detach().double())

  def bn(self, x, with_skip=False):
    v = lambda t: t.detach().double().view(1, -1, 1, 1)
    y = (x.double() - v(self.moving_mean.tensor)) / torch.sqrt(v(self.moving_var.tensor) + self.eps) * v(self.gamma.tensor) + v(self.beta.tensor)
    y = torch.relu(y) if self.act == 'Relu' else (torch.clamp(y, 0, 6) if self.act == 'Relu6' else y)
    return (y, x) if with_skip else y            # the bottleneck block asks for its identity shortcut in inference too

  with mock.patch.object(G.Conv2D, '__call__', conv), mock.patch.object(G.DepthwiseConv2D, '__call__', depthwise), \
      mock.patch.object(G.Dense, '__call__', dense), mock.patch.object(G.BatchNormAct, '__call__', bn), torch.no_grad(), graph.as_default():
    return mh.forward_eval(G.to_device_images(images, graph).double())


def _dist(a, ref):
  return float((a.double() - ref).abs().max()) / float(ref.abs().max())


def _parity(mh, shrunk_path, dtype, images, what):
  from pocketflow_amd.inference import load_shrunk
  g_full, fwd_full = load_shrunk(mh, shrunk_path, 'cuda', dtype, reinflate='all')      # the same weights in full shape (parent's path)
  g, fwd = load_shrunk(mh, shrunk_path, 'cuda', dtype, reinflate='none')               # every shrunk layer on the gather kernel
  assert g_full.nb_gathered == 0 and g.nb_gathered >= 1
  ref = forward64(g_full, mh, images)
  full, got = fwd_full(images), fwd(images)
  torch.cuda.synchronize()
  assert torch.isfinite(got).all() and torch.equal(got, fwd(images))
  d_full, d_shrunk = _dist(full, ref), _dist(got, ref)
  print('%s: %d gathered layers; full-shape path vs float64 %.3e; shrunk path vs float64 %.3e; shrunk vs full-shape %.3e'
        % (what, g.nb_gathered, d_full, d_shrunk, _dist(got, full.double())))
  assert d_shrunk <= 2.0 * d_full, (what, d_shrunk, d_full)
  return g


@pytest.mark.parametrize('net,dtype,batch,kw', [
    ('resnet_at_cifar10', 'float32', 128, dict(resnet_size=20, nb_classes=10)),
    ('mobilenet_at_ilsvrc12', 'bfloat16', 32, dict(mobilenet_depth_mult=1.0, nb_classes=1001, image_size=224)),
    ('resnet_at_ilsvrc12', 'bfloat16', 32, dict(resnet_size=50, nb_classes=1001, image_size=224))],
    ids=['resnet20-float32', 'mobilenet-bf16', 'resnet50-bf16'])
def test_shrunk_logits_against_full_shape(tmp_path, net, dtype, batch, kw):
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  from pocketflow_amd.tools.conversion import export_chn_pruned_model as E
  FLAGS = _flags(tmp_path, batch_size=batch, batch_size_eval=batch, compute_dtype=dtype, **kw)
  mh = importlib.import_module('pocketflow_amd.nets.' + net).ModelHelper()
  create_synthetic_checkpoint(mh)
  model_dir = str(tmp_path / 'models')
  assert E.main(['--model_dir', model_dir, '--enbl_fake_prune', '--fake_prune_ratio', '0.5']) == 0
  images, _ = mh.dataset_train.make_batch(np.random.RandomState(5), batch)
  images = np.asarray(images, dtype=np.float32)
  _parity(mh, os.path.join(model_dir, 'model_shrunk.npz'), torch.float32 if dtype == 'float32' else torch.bfloat16, images, net + ' ' + dtype)


def test_pruned_by_the_learner_exported_and_run(tmp_path):
  """The whole way a user goes: chn-pruned-gpu on ResNet-20 (a few selection and fine-tune steps; the proximal step at ratio 0.5
  zeroes channels within 6 iterations per layer, as tests/test_zz_search_gpu.py pins), export WITHOUT fake pruning, load_shrunk."""
  from pocketflow_amd.nets.resnet_at_cifar10 import ModelHelper
  from pocketflow_amd.learners.learner_utils import create_learner, create_synthetic_checkpoint
  from pocketflow_amd.tools.conversion import export_chn_pruned_model as E
  from pocketflow_amd.inference import read_model_file, split_gathers
  FLAGS = _flags(tmp_path, batch_size=16, batch_size_eval=16, resnet_size=20, nb_classes=10, learner='chn-pruned-gpu',
                 compute_dtype='float32', cpg_prune_ratio=0.5, cpg_nb_iters_layer=6, cpg_lrn_rate_pgd_init=1e-6,
                 cpg_save_path=str(tmp_path / 'cpg' / 'model.ckpt'), cpg_save_path_eval=str(tmp_path / 'cpg_eval' / 'model.ckpt'),
                 nb_iters_override=3, summ_step=2)
  mh = ModelHelper()
  create_synthetic_checkpoint(mh)
  lrn = create_learner(None, mh)
  lrn.train()
  model_dir = str(tmp_path / 'cpg_eval')
  assert E.main(['--model_dir', model_dir]) == 0
  path = os.path.join(model_dir, 'model_shrunk.npz')
  variables, gathers = split_gathers(read_model_file(path))
  assert len(gathers) >= 1 and all(variables[k].shape[2] == len(v) for k, v in gathers.items())     # really shrunk
  images, _ = mh.dataset_train.make_batch(np.random.RandomState(6), 16)
  g = _parity(mh, path, torch.float32, np.asarray(images, dtype=np.float32), 'resnet20 pruned by chn-pruned-gpu')
  assert g.nb_gathered == len(gathers) and g.kernel_params_kept < g.kernel_params


def test_calc_inference_time_end_to_end(tmp_path, capsys):
  from pocketflow_amd.nets.resnet_at_cifar10 import ModelHelper
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  from pocketflow_amd.tools.conversion import export_chn_pruned_model as E
  from pocketflow_amd.tools.benchmark import calc_inference_time as T
  _flags(tmp_path, batch_size=64, batch_size_eval=64, resnet_size=20, nb_classes=10, compute_dtype='float32')
  create_synthetic_checkpoint(ModelHelper())
  model_dir = str(tmp_path / 'models')
  assert E.main(['--model_dir', model_dir, '--enbl_fake_prune', '--fake_prune_ratio', '0.5']) == 0
  common = ['--net', 'resnet_at_cifar10', '--resnet_size', '20', '--nb_classes', '10', '--batch_size', '64', '--compute_dtype', 'float32',
            '--nb_repts_warmup', '3', '--nb_repts', '5', '--json']
  for extra, gathered in ((['--model_file', os.path.join(model_dir, 'model_shrunk.npz'), '--reinflate', 'none'], True),
                          (['--model_file', model_dir], False)):
    assert T.main(common + extra) == 0
    line = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{')][-1])
    assert line['ms_per_batch'] > 0 and line['ms_per_image'] > 0 and line['batch_size'] == 64
    assert (line['nb_gathered_layers'] > 0) == gathered
