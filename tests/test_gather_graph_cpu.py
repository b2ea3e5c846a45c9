"""Shrunk channel-pruned models without a GPU: Graph.apply_gathers, Conv2D's gather route, inference.load_shrunk and
tools/benchmark/calc_inference_time on emulated entry points; the emulation against the export tool's own definition of how to run
the artefact; the register budget of pf_conv_gather.hip."""
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fake_hip import FakeHipFull, _act, _rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeHipGather(FakeHipFull):
  """FakeHipFull + conv_gather_fwd on CPU tensors: gather the kept channels, then the smaller float32 convolution."""

  def __init__(self):
    super(FakeHipGather, self).__init__()
    self.gather_calls = []                       # data_ptr of the gather vector of every call

  def conv_gather_fwd(self, X, Wk, gather, Y, B, H, Wd, C, N, R, S, stride, pad_h, pad_w, Ho, Wo, bias=None, residual=None,
                      scale_shift=None, act=None):
    self._n('conv_gather_fwd')
    self.gather_calls.append(gather.data_ptr())
    assert X.shape == (B, C, H, Wd) and Wk.shape == (N, R, S, gather.numel()) and Y.shape == (B, N, Ho, Wo)
    y = F.conv2d(X.float().index_select(1, gather.long()), Wk.float().permute(0, 3, 1, 2), stride=stride, padding=(pad_h, pad_w))
    yr = y.permute(0, 2, 3, 1).reshape(-1, N)
    if bias is not None:
      yr = yr + bias
    if residual is not None:
      yr = yr + _rows(residual, N).float()
    if scale_shift is not None:
      yr = _act(yr * scale_shift[0] + scale_shift[1], act)
    _rows(Y, N).copy_(yr)


@pytest.fixture
def gather_cpu(monkeypatch, tmp_path):
  import pocketflow_amd.graph as G
  import pocketflow_amd.learners.abstract_learner as AL
  import pocketflow_amd.learners.learner_utils  # noqa: F401
  import pocketflow_amd.nets.lenet_at_cifar10  # noqa: F401
  import pocketflow_amd.nets.resnet_at_cifar10  # noqa: F401
  from pocketflow_amd.flags import FLAGS
  fake = FakeHipGather()
  monkeypatch.setattr(G, 'hip', fake)
  monkeypatch.setattr(AL, 'require_gpu', lambda: torch.device('cpu'))
  FLAGS.save_path = str(tmp_path / 'models' / 'model.ckpt')
  FLAGS.synthetic_pool, FLAGS.compute_dtype, FLAGS.batch_size, FLAGS.batch_size_eval, FLAGS.nb_classes = 2, 'float32', 4, 4, 10
  return FLAGS, fake, tmp_path


def _export(FLAGS, net, tmp):
  """Synthetic checkpoint -> export with random pruning at 0.5 -> (ModelHelper, path of model_shrunk.npz)."""
  import importlib
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  from pocketflow_amd.tools.conversion import export_chn_pruned_model as E
  if net == 'resnet_at_cifar10':
    FLAGS.resnet_size = 20
  mh = importlib.import_module('pocketflow_amd.nets.' + net).ModelHelper()
  create_synthetic_checkpoint(mh)
  model_dir = str(tmp / 'models')
  assert E.main(['--model_dir', model_dir, '--enbl_fake_prune', '--fake_prune_ratio', '0.5']) == 0
  return mh, os.path.join(model_dir, 'model_shrunk.npz')


@pytest.mark.parametrize('net', ['resnet_at_cifar10', 'lenet_at_cifar10'])
def test_load_shrunk_matches_the_full_shape_model(gather_cpu, net):
  from pocketflow_amd.inference import load_shrunk, read_model_file, split_gathers
  FLAGS, fake, tmp = gather_cpu
  mh, path = _export(FLAGS, net, tmp)
  variables, gathers = split_gathers(read_model_file(path))
  assert gathers and all(variables[k].shape[2] == len(g) for k, g in gathers.items())
  images = np.random.RandomState(3).randn(4, 32, 32, 3).astype(np.float32)
  g_full, fwd_full = load_shrunk(mh, path, 'cpu', torch.float32, reinflate='all')      # the fake-pruned kernels in full shape
  assert g_full.nb_gathered == 0 and sorted(g_full.reinflated) == sorted(gathers) and g_full.kernel_params_kept == g_full.kernel_params
  ref = fwd_full(images)
  assert fake.calls.get('conv_gather_fwd', 0) == 0
  g, fwd = load_shrunk(mh, path, 'cpu', torch.float32, reinflate='none')
  assert g.nb_gathered == len(gathers) and g.reinflated == []
  assert g.kernel_params == g_full.kernel_params and g.kernel_params_kept == sum(
      v.size for k, v in variables.items() if k in g.store.by_name and g.store.by_name[k].kind == 'conv')
  for name, vec in gathers.items():               # the stored kernel shapes are the shrunk ones
    var = g.store.by_name[name]
    assert var.ref_shape == variables[name].shape and var.ref_shape[2] == len(vec) < var.cin_full
    assert tuple(var.tensor.shape) == (var.ref_shape[3], len(vec), var.ref_shape[0], var.ref_shape[1])
    assert var.gather.dtype == torch.int32 and var.gather.tolist() == list(vec)
  got = fwd(images)
  # every shrunk convolution called the gather entry exactly once, and no other convolution did
  ptrs = sorted(g.store.by_name[name].gather.data_ptr() for name in gathers)
  assert sorted(fake.gather_calls) == ptrs and fake.calls['conv_gather_fwd'] == len(gathers)
  err = float((got - ref).abs().max()) / float(ref.abs().max())
  assert err <= 2e-5, err
  # the default keeps the layers graph.gather_pays accepts and re-inflates the others: same logits either way
  g_auto, fwd_auto = load_shrunk(mh, path, 'cpu', torch.float32)
  assert g_auto.nb_gathered + len(g_auto.reinflated) == len(gathers)
  assert float((fwd_auto(images) - ref).abs().max()) / float(ref.abs().max()) <= 2e-5
  # a plain checkpoint directory loads through the same function
  g_dir, fwd_dir = load_shrunk(mh, os.path.dirname(path), 'cpu', torch.float32)
  assert g_dir.nb_gathered == 0 and torch.isfinite(fwd_dir(images)).all()


def _small_graph():
  import pocketflow_amd.graph as G
  g = G.Graph('model', 'cpu', torch.float32)
  conv = G.Conv2D(g, 'conv', 8, 6, 3, 1, 'SAME')
  G.DepthwiseConv2D(g, 'dw', 8, 3, 1)
  G.Dense(g, 'fc', 8, 4)
  return g, conv


def test_apply_gathers_rejections_name_the_variable(gather_cpu):
  ok = np.array([0, 2, 5], dtype=np.int32)
  for gathers, values, name in (
      ({'model/dw/depthwise_weights': ok}, None, 'model/dw/depthwise_weights'),
      ({'model/fc/kernel': ok}, None, 'model/fc/kernel'),
      ({'model/conv/kernel': np.array([0, 5, 2], dtype=np.int32)}, None, 'model/conv/kernel'),
      ({'model/conv/kernel': np.array([0, 2, 2], dtype=np.int32)}, None, 'model/conv/kernel'),
      ({'model/conv/kernel': np.array([0, 2, 8], dtype=np.int32)}, None, 'model/conv/kernel'),
      ({'model/conv/kernel': np.array([-1, 2, 5], dtype=np.int32)}, None, 'model/conv/kernel'),
      ({'model/conv/kernel': ok}, {'model/conv/kernel': np.zeros((3, 3, 4, 6), np.float32)}, 'model/conv/kernel'),
      ({'model/nope/kernel': ok}, None, 'model/nope/kernel')):
    g, _ = _small_graph()
    with pytest.raises(ValueError, match=re.escape(name)):
      g.apply_gathers(gathers, values)
  g, conv = _small_graph()
  g.apply_gathers({'model/conv/kernel': ok}, {'model/conv/kernel': np.zeros((3, 3, 3, 6), np.float32)})
  assert conv.kernel.ref_shape == (3, 3, 3, 6) and conv.kernel.cin_full == 8
  g.finalize(requires_grad=False)
  assert conv.kernel.gather.tolist() == [0, 2, 5] and tuple(conv.kernel.tensor.shape) == (6, 3, 3, 3)
  with pytest.raises(RuntimeError):
    g.apply_gathers({'model/conv/kernel': ok})     # after finalize


def test_gathered_layer_refuses_gradients_and_taps_see_the_full_input(gather_cpu):
  FLAGS, fake, tmp = gather_cpu
  g, conv = _small_graph()
  g.apply_gathers({'model/conv/kernel': np.array([1, 4], dtype=np.int32)})
  g.finalize(requires_grad=True)                  # a trainable kernel
  x = torch.randn(2, 8, 5, 5).contiguous(memory_format=torch.channels_last)
  with torch.enable_grad(), g.as_default():
    with pytest.raises(RuntimeError, match='model/conv/kernel'):
      conv(x)
  with torch.no_grad(), g.as_default():
    y = conv(x)
    w = conv.kernel.tensor.detach()
    assert torch.allclose(y, F.conv2d(x[:, [1, 4]], w, padding=1), atol=1e-6)
    g.taps = {}
    conv(x)
    assert g.taps[conv][0].shape[1] == 8          # the un-gathered input is recorded
    g.taps = None
    with pytest.raises(ValueError, match='model/conv/kernel'):
      conv(x[:, :4])


@pytest.mark.parametrize('seed', range(6))
def test_emulation_agrees_with_the_export_tools_conv_gather(seed):
  """FakeHipGather.conv_gather_fwd against export_chn_pruned_model.conv_gather (the tool's definition of how the artefact runs), with
  stride 2, bias, residual and the folded scale / shift + Relu6 epilogue."""
  from pocketflow_amd.tools.conversion.export_chn_pruned_model import conv_gather
  rng = np.random.RandomState(seed)
  B, C, N, k = 2, int(rng.randint(3, 20)), int(rng.randint(1, 12)), int(rng.choice([1, 3, 5]))
  stride, pad, H, W = int(rng.choice([1, 2])), int(rng.choice([0, k // 2])), int(rng.randint(6, 12)), int(rng.randint(6, 12))
  Ck = int(rng.randint(1, C + 1))
  gather = np.sort(rng.permutation(C)[:Ck]).astype(np.int32)
  kernel = rng.randn(k, k, Ck, N).astype(np.float32)
  x = torch.from_numpy(rng.randn(B, C, H, W).astype(np.float32))
  ref = conv_gather(x, kernel, gather, stride, pad)
  Ho, Wo = ref.shape[2], ref.shape[3]
  bias = torch.from_numpy(rng.randn(N).astype(np.float32))
  res = torch.from_numpy(rng.randn(B, N, Ho, Wo).astype(np.float32))
  ss = torch.from_numpy(np.stack([rng.rand(N) + 0.5, rng.randn(N)]).astype(np.float32))
  wk = torch.from_numpy(np.ascontiguousarray(kernel.transpose(3, 0, 1, 2)))
  fake = FakeHipGather()
  v = lambda t: t.view(1, N, 1, 1)
  for kw, want in (({}, ref), ({'bias': bias}, ref + v(bias)), ({'residual': res}, ref + res),
                   ({'scale_shift': ss, 'act': 'Relu6'}, torch.clamp(ref * v(ss[0]) + v(ss[1]), 0, 6)),
                   ({'scale_shift': ss, 'act': None}, ref * v(ss[0]) + v(ss[1]))):
    y = torch.full((B, N, Ho, Wo), float('nan')).contiguous(memory_format=torch.channels_last)   # the layout the layers allocate
    fake.conv_gather_fwd(x, wk, torch.from_numpy(gather), y, B, H, W, C, N, k, k, stride, pad, pad, Ho, Wo, **kw)
    assert float((y - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max())), sorted(kw)


def test_gather_kernels_compile_without_spills(tmp_path):
  """pf_conv_gather.hip for gfx950: no kernel may spill vector registers or need more than 256 of them (the check
  test_repo_rules.test_contraction_kernels_compile_without_spills makes for the other contraction kernels)."""
  import subprocess
  hipcc = '/opt/rocm/bin/hipcc'
  if not os.path.exists(hipcc):
    pytest.skip('no hipcc')
  out = str(tmp_path / 'pf_conv_gather.s')
  r = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off',
                      '-fhip-fp32-correctly-rounded-divide-sqrt', '-S', '--cuda-device-only',
                      os.path.join(ROOT, 'pocketflow_amd', 'csrc', 'pf_conv_gather.hip'), '-o', out], capture_output=True, text=True, timeout=600)
  assert r.returncode == 0, r.stderr[-2000:]
  seen = []
  for m in re.finditer(r'\.name:\s+(\S+)(.*?)\.wavefront_size', open(out).read(), re.S):
    name, blk = m.group(1), m.group(2)
    if 'k_conv_gather' not in name:
      continue
    vg = int(re.search(r'\.vgpr_count:\s+(\d+)', blk).group(1))
    sp = int(re.search(r'\.vgpr_spill_count:\s+(\d+)', blk).group(1))
    scratch = int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', blk).group(1))
    assert sp == 0 and vg <= 256 and scratch == 0, (name, vg, sp, scratch)
    seen.append(name)
  assert len(seen) == 3, seen                     # float32, bf16 x 64 columns, bf16 x 128 columns


def test_calc_inference_time_on_the_emulation(gather_cpu, capsys):
  from pocketflow_amd.tools.benchmark import calc_inference_time as T
  FLAGS, fake, tmp = gather_cpu
  mh, path = _export(FLAGS, 'resnet_at_cifar10', tmp)
  common = ['--net', 'resnet_at_cifar10', '--resnet_size', '20', '--batch_size', '4', '--nb_repts_warmup', '2', '--nb_repts', '2',
            '--compute_dtype', 'float32', '--json']
  lines = []
  for extra in (['--model_file', path, '--reinflate', 'none'], ['--model_file', path, '--reinflate', 'all'],
                ['--model_file', os.path.dirname(path)]):
    assert T.main(common + extra) == 0
    out = capsys.readouterr().out
    lines.append(json.loads([ln for ln in out.splitlines() if ln.startswith('{')][-1]))
  for ln in lines:
    for key in ('ms_per_batch', 'ms_per_image', 'batch_size', 'nb_gathered_layers', 'kernel_params_kept_share', 'model_file',
                'nb_repts', 'nb_repts_warmup'):
      assert key in ln, key
    assert ln['ms_per_batch'] > 0 and abs(ln['ms_per_image'] * 4 - ln['ms_per_batch']) < 1e-9 and ln['batch_size'] == 4
  assert lines[0]['nb_gathered_layers'] > 0 and 0.3 < lines[0]['kernel_params_kept_share'] < 0.7
  assert lines[1]['nb_gathered_layers'] == 0 and lines[2]['nb_gathered_layers'] == 0 and lines[2]['kernel_params_kept_share'] == 1.0
  assert fake.calls['conv_gather_fwd'] == 4 * lines[0]['nb_gathered_layers']
