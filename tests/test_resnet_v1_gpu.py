"""ResNet v1 bottleneck blocks on the GPU: one block with the fused join (graph.BatchNormAddAct on pf_bn_join.hip) against the same
block forced onto the composition of the v1 basic block (BatchNormAct, torch add, Activation), and ResNet-50 v1 under the full-prec
and the uniform-quantisation learner."""
import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

pytestmark = pytest.mark.gpu


def _block_run(monkeypatch, dtype, fused):
  """Forward + backward of one projection block (cin 64, filters 16, stride 2) at batch 4, 16 x 16, from seeded variables.
  Returns {name: float64 tensor}: the output, the input gradient and every parameter gradient."""
  from pocketflow_amd import graph as G
  from pocketflow_amd.utils.external import resnet_model as R
  if not fused:
    monkeypatch.setattr(G, 'bn_join_tensor_ok', lambda x: False)
  g = G.Graph('model', 'cuda', dtype)
  with g.as_default():
    blk = R._BottleneckBlockV1(g, 64, 16, True, 2)
  g.finalize(seed=3, requires_grad=True)
  gen = torch.Generator(device='cpu').manual_seed(21)
  with torch.no_grad():
    for v in g.store.vars:
      if v.kind == 'bn_gamma':
        v.tensor.copy_((0.5 + torch.rand(v.tensor.shape, generator=gen)).to(v.tensor.device))
      elif v.kind == 'bn_beta':
        v.tensor.copy_((0.3 * torch.randn(v.tensor.shape, generator=gen)).to(v.tensor.device))
  x = torch.randn(4, 64, 16, 16, generator=gen).to(dtype).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
  w = torch.randn(4, 64, 8, 8, generator=gen).cuda()
  g.store.zero_grad()
  g.training = True
  g.begin_step()
  calls = dict(fwd=0, gate=0)
  from pocketflow_amd import hip
  for key, name in (('fwd', 'bn_add_act_fwd'), ('gate', 'bn_add_act_bwd_gate')):
    def counted(*a, _f=getattr(hip, name), _k=key, **kw):
      calls[_k] += 1
      return _f(*a, **kw)
    monkeypatch.setattr(hip, name, counted)
  with g.as_default():
    y = blk(G.fork(x, g))
  (y.float() * w).sum().backward()
  torch.cuda.synchronize()
  assert (calls['fwd'], calls['gate']) == ((2, 1) if fused else (0, 0))      # the join, and the fork's sum of two gradients
  assert hasattr(y, '_pf_skip') == fused
  st = g.store
  out = {'output': y.detach().double().cpu(), 'dx': x.grad.double().cpu()}
  for v in st.trainable_vars:
    flat = st.w_grad if v.group == 'W' else st.o_grad
    out[v.name] = flat[v.offset:v.offset + v.numel].detach().double().cpu().clone()
  monkeypatch.undo()
  return out


def _cos(a, b):
  a, b = a.reshape(-1), b.reshape(-1)
  return float(a @ b / (a.norm() * b.norm() + 1e-300))


def test_block_float32_equals_the_composition(monkeypatch):
  """float32: the forward of the join is the same three operations, bit for bit; the backward differs in the order of the BN sums.
  Bar: 1e-4 of the largest value, the float32 bar of tests/test_zz_search_gpu.py for the BN kernels against autograd."""
  a = _block_run(monkeypatch, torch.float32, False)
  b = _block_run(monkeypatch, torch.float32, True)
  assert sorted(a) == sorted(b) and len(a) == 2 + 4 + 2 * 4
  assert torch.equal(a['output'], b['output'])
  for k in a:
    scale = float(a[k].abs().max())
    assert scale > 0.0, k
    err = float((a[k] - b[k]).abs().max())
    assert err <= 1e-4 * max(1.0, scale), (k, err, scale)


def test_block_bf16_within_the_bf16_storage_bar(monkeypatch):
  """bf16, in the convention of parity_common.bf16_gradient_check: the float32 composition is the reference, the bf16 composition
  against it is the noise floor of bf16 STORAGE, quantity by quantity (cosine); the fused bf16 block must reach the floor - 0.05 and
  0.80 wherever the floor is meaningful (>= 0.90), and the concatenated gradient the floor - 0.03 with its norm within 5 %."""
  ref = _block_run(monkeypatch, torch.float32, False)
  floor = _block_run(monkeypatch, torch.bfloat16, False)
  got = _block_run(monkeypatch, torch.bfloat16, True)
  reliable = 0
  for k in ref:
    fl, pr = _cos(floor[k], ref[k]), _cos(got[k], ref[k])
    print('v1 block bf16 %-55s floor %.4f fused %.4f' % (k, fl, pr))
    if fl >= 0.90:
      reliable += 1
      assert pr >= fl - 0.05 and pr >= 0.80, (k, pr, fl)
  assert reliable >= len(ref) // 2
  cat = lambda d: torch.cat([d[k].reshape(-1) for k in sorted(ref) if k != 'output'])
  whole_floor, whole = _cos(cat(floor), cat(ref)), _cos(cat(got), cat(ref))
  ratio = float(cat(got).norm() / cat(ref).norm())
  print('v1 block bf16 whole gradient: floor %.4f fused %.4f norm ratio %.4f' % (whole_floor, whole, ratio))
  assert whole >= whole_floor - 0.03 and abs(ratio - 1.0) <= 0.05


class _AtenProbe(TorchDispatchMode):
  """Records every aten element-wise add / relu (and relu's backward) whose result is a 4-D GPU tensor with the batch size in front:
  an activation.  It sees the forward pass and the autograd engine's own gradient accumulation alike."""
  NAMES = ('add', 'add_', 'relu', 'relu_', 'threshold_backward', 'clamp_min', 'clamp_min_')

  def __init__(self, batch):
    super().__init__()
    self.batch, self.hits = batch, []

  def __torch_dispatch__(self, func, types, args=(), kwargs=None):
    out = func(*args, **(kwargs or {}))
    name = getattr(getattr(func, 'overloadpacket', None), '__name__', str(func))
    if name in self.NAMES and isinstance(out, torch.Tensor) and out.is_cuda and out.dim() == 4 and out.shape[0] == self.batch:
      self.hits.append((name, tuple(out.shape)))
    return out


def test_the_probe_sees_forward_and_engine_side_launches():
  x = torch.randn(8, 16, 4, 4, device='cuda', requires_grad=True)
  with _AtenProbe(8) as probe:
    y = torch.relu(x * 2.0) + x * 3.0               # forward: relu, add; backward: threshold_backward, the engine's accumulation
    y.sum().backward()
  names = [n for n, _ in probe.hits]
  assert 'relu' in names and 'threshold_backward' in names and names.count('add') + names.count('add_') >= 2, names


@pytest.mark.parametrize('kind', ['full-prec', 'uniform'])
def test_resnet50_v1_trains_under_the_learners(tmp_path, monkeypatch, kind):
  """ResNet-50 v1 at 64 x 64, batch 8, bf16: one forward + backward without the update (gradients read), then two training steps.
  Losses finite; parameters finite and moved; no parameter gradient all zero; and in the probed step no aten add / relu launch on
  an activation: the 16 joins, the two consumers of every block output and the fork in front of the first block all run on
  pf_bn_join.hip (launch counter on the binding, as tests/test_head_fused_gpu.py counts its launches)."""
  from parity_common import product_gradients
  from pocketflow_amd.flags import FLAGS
  import pocketflow_amd.learners.learner_utils  # noqa: F401  (defines flags)
  import pocketflow_amd.learners.abstract_learner  # noqa: F401
  import pocketflow_amd.datasets.abstract_dataset  # noqa: F401  (synthetic_pool)
  from pocketflow_amd import hip
  from pocketflow_amd.nets.resnet_at_ilsvrc12 import ModelHelper
  from pocketflow_amd.learners.full_precision.learner import FullPrecLearner
  from pocketflow_amd.learners.uniform_quantization.learner import UniformQuantLearner
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  batch = 8
  for k, v in dict(save_path=str(tmp_path / 'models' / 'model.ckpt'), save_path_eval=str(tmp_path / 'models_eval' / 'model.ckpt'),
                   synthetic_pool=2, batch_size=batch, batch_size_eval=batch, uql_weight_bits=8, uql_activation_bits=8,
                   enbl_dst=(kind == 'uniform'), dst_eval_teacher=False, save_path_dst=str(tmp_path / 'models_dst' / 'model.ckpt'),
                   uql_save_quant_model_path=str(tmp_path / 'uql' / 'm.ckpt'), nb_eval_batches_override=1, resnet_size=50,
                   resnet_version=1, nb_classes=1001, image_size=64, uql_use_buckets=False, compute_dtype='bfloat16').items():
    setattr(FLAGS, k, v)
  import scipy.stats                              # clipped normals instead of scipy's truncated-normal sampler (seconds per network)
  monkeypatch.setattr(scipy.stats.truncnorm, 'rvs', lambda a, b, size=None, random_state=None:
                      np.clip(random_state.standard_normal(size), a, b))
  mh = ModelHelper()
  assert mh.model_name == 'resnet_v1_50'
  create_synthetic_checkpoint(mh)
  learner = (UniformQuantLearner if kind == 'uniform' else FullPrecLearner)(None, mh)
  graph = learner.graph
  assert len(graph.join_layers) == 16 and len(graph.activation_ops) == 49
  if kind == 'uniform':
    assert all(j.op.bits == 8 for j in graph.join_layers)
  calls = dict(bn_add_act_fwd=0, bn_add_act_bwd_gate=0)
  for name in calls:
    def counted(*a, _f=getattr(hip, name), _n=name, **kw):
      calls[_n] += 1
      return _f(*a, **kw)
    monkeypatch.setattr(hip, name, counted)
  with _AtenProbe(batch) as probe:
    out, grads = product_gradients(learner)
  torch.cuda.synchronize()
  assert probe.hits == [], probe.hits[:8]
  # student: 16 joins + the fork's sum; with distillation 16 more, in inference mode, per forward of the teacher (which also runs
  # ahead of the student, learners/teacher_ahead.py)
  teacher = calls['bn_add_act_fwd'] - 17
  assert calls['bn_add_act_bwd_gate'] == 16 and (teacher == 0 if kind == 'full-prec' else teacher in (16, 32)), calls
  assert len(grads) == len(graph.store.trainable_vars)
  for name, gr in grads.items():
    assert np.isfinite(gr).all() and float(np.abs(gr).max()) > 0.0, name
  st = graph.store
  before = (st.w_master.detach().clone(), st.o_master.detach().clone())
  for _ in range(2):
    o = learner.train_step()
    loss = o['loss'] if isinstance(o, dict) else o[1]        # the full-prec learner returns (lr, loss, metrics)
    assert bool(torch.isfinite(loss.detach().float()).all()), o
  torch.cuda.synchronize()
  for b, a in zip(before, (st.w_master.detach(), st.o_master.detach())):
    assert bool(torch.isfinite(a).all()) and float((a - b).abs().max()) > 0.0
  for v in st.trainable_vars:
    flat, old = (st.w_master, before[0]) if v.group == 'W' else (st.o_master, before[1])
    assert not torch.equal(flat[v.offset:v.offset + v.numel], old[v.offset:v.offset + v.numel]), v.name
