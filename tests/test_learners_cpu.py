"""The learners' HOST logic executed on the CPU against the CPU oracle learner, exactly.

The HIP entry points are replaced by float32 emulations (tests/fake_hip.py); everything else is the product
code: graph rewrite (which ops get which bit widths), launch plans over the flat buffers, KRSC <-> HWIO index
arithmetic, bucket modes, codebook variables in the variable store, loss wiring (CE + coupled L2 + distillation),
optimiser masks and slots, learning-rate schedules, the mask-refresh schedule.  Both sides use float32; the
convolutions differ in summation order (torch CPU kernels vs the oracle's), so the bars are the same kind as in
tests/test_parity_gpu.py (loss within 1e-4 .. 2e-3, weights within the Adam bound)."""
import numpy as np
import pytest
import torch

from fake_hip import FakeHipFull


@pytest.fixture
def cpu_learners(monkeypatch, tmp_path):
  import pocketflow_amd.graph as G
  import pocketflow_amd.plan as P
  import pocketflow_amd.losses as L
  import pocketflow_amd.optim as Opt
  import pocketflow_amd.learners.abstract_learner as AL
  import pocketflow_amd.learners.weight_sparsification.learner as WS
  import pocketflow_amd.learners.nonuniform_quantization.utils as NU
  import pocketflow_amd.learners.distillation_helper  # noqa: F401
  import pocketflow_amd.learners.learner_utils  # noqa: F401
  import pocketflow_amd.nets.lenet_at_cifar10  # noqa: F401  (flag definitions)
  import pocketflow_amd.nets.resnet_at_cifar10  # noqa: F401
  import pocketflow_amd.learners.uniform_quantization.learner  # noqa: F401
  import pocketflow_amd.learners.nonuniform_quantization.learner  # noqa: F401
  from pocketflow_amd.flags import FLAGS
  fake = FakeHipFull()
  import pocketflow_amd.learners.layerwise as LW
  for mod in (G, P, L, Opt, WS, NU, LW):
    monkeypatch.setattr(mod, 'hip', fake)
  monkeypatch.setattr(AL, 'require_gpu', lambda: torch.device('cpu'))
  monkeypatch.setattr(G, 'DEPTHWISE_ANY_DEVICE', True)      # MobileNet: the depthwise plumbing on the emulated entry points
  FLAGS.save_path = str(tmp_path / 'models' / 'model.ckpt')
  FLAGS.save_path_eval = str(tmp_path / 'models_eval' / 'model.ckpt')
  FLAGS.enbl_dst = False
  FLAGS.nb_eval_batches_override = 2
  FLAGS.save_path_dst = str(tmp_path / 'models_dst' / 'model.ckpt')
  FLAGS.synthetic_pool = 2
  FLAGS.compute_dtype = 'float32'
  return FLAGS, fake, tmp_path


def _pool(it):
  return [(i.numpy(), l.numpy()) for i, l in it.batches]


def _cfg(FLAGS, model, dataset, shape, **kw):
  c = dict(model=model, dataset=dataset, resnet_size=FLAGS.resnet_size if 'resnet_size' in FLAGS else 0,
           nb_classes=FLAGS.nb_classes, loss_w_dcy=FLAGS.loss_w_dcy, enbl_dst=FLAGS.enbl_dst,
           loss_w_dst=FLAGS.loss_w_dst, tempr_dst=FLAGS.tempr_dst, momentum=FLAGS.momentum, image_shape=shape)
  c.update(kw)
  return c


def _max_rel(a, b):
  worst = 0.0
  for k, ref in b.items():
    worst = max(worst, float(np.max(np.abs(a[k] - ref) / np.maximum(1.0, np.abs(ref)))) if ref.size else 0.0)
  return worst


@pytest.mark.parametrize('use_buckets,bucket_type,bits', [(False, 'channel', 8), (True, 'channel', 4), (True, 'split', 3)])
def test_uq_lenet_on_cpu(cpu_learners, use_buckets, bucket_type, bits):
  FLAGS, fake, tmp = cpu_learners
  from oracle.learner_oracle import OracleLearner
  from pocketflow_amd.nets.lenet_at_cifar10 import ModelHelper
  from pocketflow_amd.learners.uniform_quantization.learner import UniformQuantLearner
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  FLAGS.batch_size, FLAGS.batch_size_eval, FLAGS.nb_classes = 16, 16, 10
  FLAGS.uql_weight_bits, FLAGS.uql_activation_bits = bits, 8
  FLAGS.uql_use_buckets, FLAGS.uql_bucket_type, FLAGS.uql_bucket_size = use_buckets, bucket_type, 64
  FLAGS.uql_save_quant_model_path = str(tmp / 'uql' / 'm.ckpt')
  FLAGS.nb_eval_batches_override = 2
  mh = ModelHelper()
  create_synthetic_checkpoint(mh)
  lrn = UniformQuantLearner(None, mh)
  ora = OracleLearner(lrn.graph.store.export_numpy(),
                      _cfg(FLAGS, 'lenet', 'cifar_10', (32, 32, 3), learner='uniform', uql_weight_bits=bits,
                           uql_activation_bits=8, uql_use_buckets=use_buckets, uql_bucket_type=bucket_type,
                           uql_bucket_size=64), lrn.lrn_rate)
  pool = _pool(lrn.iter_train)
  for step in range(3):
    out = lrn.train_step()
    ref = ora.train_step(*pool[step % 2])
    assert abs(float(out['loss'].detach()) - ref['loss']) <= 1e-4 * max(1.0, abs(ref['loss'])), step
  assert _max_rel(lrn.graph.store.export_numpy(), ora.export()) <= 2 * 3 * lrn.lrn_rate(0) + 1e-6
  lrn.graph.training = False
  rs = lrn.run_eval()
  ev = [ora.eval_batch(*b) for b in _pool(lrn.iter_eval)[:2]]
  assert abs(rs['loss'] - np.mean([e['loss'] for e in ev])) <= 2e-4
  assert abs(rs['acc_top1'] - np.mean([e['metrics']['accuracy'] for e in ev])) <= 1.0 / 32 + 1e-6   # one near-tie sample of 32


@pytest.mark.parametrize('a_bits', [32, 8])
def test_uq_resnet20_gradients_match_oracle_on_cpu(cpu_learners, a_bits):
  """Gradient-level parity (VERDICT r2 "next" 2a) of the layer executor's autograd plumbing with the HIP entry points
  emulated in float32: d(loss)/d(variable) after ONE backward pass, variable by variable, against the oracle learner --
  the check the Adam-bounded weight comparison cannot give.  The GPU suite runs the same helper on the real kernels."""
  FLAGS, fake, tmp = cpu_learners
  from oracle.learner_oracle import OracleLearner
  from parity_common import product_gradients, compare_gradients, gradient_report
  from pocketflow_amd.nets.resnet_at_cifar10 import ModelHelper
  from pocketflow_amd.learners.uniform_quantization.learner import UniformQuantLearner
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  FLAGS.batch_size, FLAGS.batch_size_eval, FLAGS.nb_classes, FLAGS.resnet_size = 8, 8, 10, 20
  FLAGS.uql_weight_bits, FLAGS.uql_activation_bits, FLAGS.uql_use_buckets, FLAGS.uql_bucket_type = 8, a_bits, True, 'channel'
  FLAGS.enbl_dst, FLAGS.dst_eval_teacher = True, False
  FLAGS.uql_save_quant_model_path = str(tmp / 'uql' / 'm.ckpt')
  mh = ModelHelper()
  create_synthetic_checkpoint(mh)
  lrn = UniformQuantLearner(None, mh)
  ora = OracleLearner(lrn.graph.store.export_numpy(),
                      _cfg(FLAGS, 'resnet', 'cifar_10', (32, 32, 3), learner='uniform', uql_weight_bits=8,
                           uql_activation_bits=a_bits, uql_use_buckets=True, uql_bucket_type='channel'), lrn.lrn_rate)
  pool = _pool(lrn.iter_train)
  before = lrn.graph.store.export_numpy()
  out, hg = product_gradients(lrn)
  after = lrn.graph.store.export_numpy()
  assert all(np.array_equal(before[k], after[k]) for k in before if 'moving_' not in k), 'the capture must not update'
  ref, og = ora.compute_grads(*pool[0])
  assert abs(float(out['loss'].detach()) - ref['loss']) <= 2e-4 * max(1.0, abs(ref['loss']))
  per, wc, wr = compare_gradients(hg, ora, og)
  worst_l2, worst_cos = gradient_report(per, wc, wr, 'ResNet-20 UQ w8/a%d + dst (CPU emulation)' % a_bits)
  assert len(per) == len(og)
  # 32-bit activations: continuous path, float32 summation order only.  8 bits: a rounding-boundary flip changes a
  # gradient element by a whole STE gate (DESIGN section 2 "Discontinuities")
  # (measured with float32 on BOTH sides at 8 bits: whole-gradient cosine 0.97, worst variable 0.93 -- a random-init BN
  # network amplifies every flipped rounding decision; the 8-bit bar is therefore statistical here and on the GPU)
  assert worst_l2[1][0] <= (1e-4 if a_bits == 32 else 0.6), worst_l2
  assert abs(wr - 1.0) <= (1e-3 if a_bits == 32 else 2e-2) and wc >= (1 - 1e-6 if a_bits == 32 else 0.95)
  # the captured gradient is the one the optimiser would have applied: a wrong-sign backward cannot pass
  sign = compare_gradients({k: -v for k, v in hg.items()}, ora, og)[1]
  assert sign < 0


def test_bf16_parity_body_on_cpu(cpu_learners):
  """The body of the GPU test `test_uq_resnet50_bf16_fused_path_matches_oracle_within_bf16_noise` with the HIP entry points
  emulated in float32: conditioned checkpoint -> student moved off its teacher -> float32 oracle / bf16-storage oracle /
  product gradients -> loss trajectory.  (In float32 the product sits far inside the bf16 noise floor it is held to.)"""
  FLAGS, fake, tmp = cpu_learners
  from parity_common import run_bf16_fused_parity
  run_bf16_fused_parity(FLAGS, tmp, steps=1, expect_bf16=False)


def test_bf16_parity_body_through_recorded_steps_on_cpu(cpu_learners, monkeypatch):
  """The same body with the trajectory running through the recorded step (in-line stand-in for the hipGraph): three launch-by-launch
  steps, then replays, compared with the oracle step by step; weights, BN statistics and the teacher-labelled evaluation afterwards."""
  FLAGS, fake, tmp = cpu_learners
  monkeypatch.setenv('PF_STEP_GRAPH', 'inline')
  monkeypatch.setenv('PF_STEP_GRAPH_STRICT', '1')
  from parity_common import run_bf16_fused_parity
  run_bf16_fused_parity(FLAGS, tmp, steps=5, expect_bf16=False, step_graph=True)


def test_uq_resnet20_distillation_on_cpu(cpu_learners):
  FLAGS, fake, tmp = cpu_learners
  from oracle.learner_oracle import OracleLearner
  from pocketflow_amd.nets.resnet_at_cifar10 import ModelHelper
  from pocketflow_amd.learners.uniform_quantization.learner import UniformQuantLearner
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  FLAGS.batch_size, FLAGS.batch_size_eval, FLAGS.nb_classes, FLAGS.resnet_size = 8, 8, 10, 20
  FLAGS.uql_weight_bits, FLAGS.uql_activation_bits, FLAGS.uql_use_buckets, FLAGS.uql_bucket_type = 8, 8, True, 'channel'
  FLAGS.enbl_dst, FLAGS.dst_eval_teacher = True, False
  FLAGS.uql_save_quant_model_path = str(tmp / 'uql' / 'm.ckpt')
  mh = ModelHelper()
  create_synthetic_checkpoint(mh)
  lrn = UniformQuantLearner(None, mh)
  ora = OracleLearner(lrn.graph.store.export_numpy(),
                      _cfg(FLAGS, 'resnet', 'cifar_10', (32, 32, 3), learner='uniform', uql_weight_bits=8,
                           uql_activation_bits=8, uql_use_buckets=True, uql_bucket_type='channel'), lrn.lrn_rate)
  pool = _pool(lrn.iter_train)
  for step in range(2):
    out = lrn.train_step()
    ref = ora.train_step(*pool[step % 2])
    # 8-bit activation quantisers on both sides, same float32 point function: only BN / conv summation order differs
    assert abs(float(out['loss'].detach()) - ref['loss']) <= 2e-3 * max(1.0, abs(ref['loss'])), (step, float(out['loss']), ref['loss'])
    assert abs(float(out['dst_loss'].detach()) - ref['dst_loss']) <= 2e-3 * max(1.0, abs(ref['dst_loss']))
  assert _max_rel(lrn.graph.store.export_numpy(), ora.export()) <= 2 * 2 * lrn.lrn_rate(0) + 1e-5


def _live_bytes_growth(step, n=3):
  """Growth of the bytes held by live tensors over `n` steps with Python's cyclic collector disabled."""
  import gc
  import torch

  def live():
    return sum(o.numel() * o.element_size() for o in gc.get_objects() if isinstance(o, torch.Tensor))
  step()
  gc.collect()
  gc.disable()
  try:
    step()
    base = live()
    for _ in range(n):
      step()
    return live() - base
  finally:
    gc.enable()


@pytest.mark.parametrize('kind', ['nuq-resnet20', 'ws-resnet20', 'fp-mobilenet'])
def test_other_learners_free_their_tensors_by_refcount(cpu_learners, kind):
  """The same property for the other step implementations: NUQ (codebook gradient, normalisation), weight sparsification
  (masks, Momentum), and the MobileNet executor (depthwise convolutions, dropout, ReLU6)."""
  FLAGS, fake, tmp = cpu_learners
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  FLAGS.batch_size, FLAGS.batch_size_eval = 4, 4
  if kind == 'nuq-resnet20':
    from pocketflow_amd.nets.resnet_at_cifar10 import ModelHelper
    from pocketflow_amd.learners.nonuniform_quantization.learner import NonUniformQuantLearner
    FLAGS.nb_classes, FLAGS.resnet_size = 10, 20
    FLAGS.nuql_weight_bits, FLAGS.nuql_use_buckets, FLAGS.nuql_opt_mode = 4, True, 'both'
    FLAGS.nuql_save_quant_model_path = str(tmp / 'nuql' / 'm.ckpt')
    mh = ModelHelper()
    create_synthetic_checkpoint(mh)
    lrn = NonUniformQuantLearner(None, mh)
    lrn.init_clusters()
  elif kind == 'ws-resnet20':
    from pocketflow_amd.nets.resnet_at_cifar10 import ModelHelper
    from pocketflow_amd.learners.weight_sparsification.learner import WeightSparseLearner
    FLAGS.nb_classes, FLAGS.resnet_size = 10, 20
    FLAGS.ws_prune_ratio, FLAGS.ws_prune_ratio_prtl, FLAGS.ws_save_path = 0.5, 'uniform', str(tmp / 'ws' / 'm.ckpt')
    lrn = WeightSparseLearner(None, ModelHelper())
  else:
    from pocketflow_amd.nets.mobilenet_at_ilsvrc12 import ModelHelper
    from pocketflow_amd.learners.full_precision.learner import FullPrecLearner
    FLAGS.nb_classes, FLAGS.image_size, FLAGS.mobilenet_depth_mult = 7, 32, 0.25
    lrn = FullPrecLearner(None, ModelHelper())
  grown = _live_bytes_growth(lrn.train_step)
  assert grown <= 0, '%s: tensors of finished steps survive without the cyclic collector: +%d bytes over 3 steps' % (kind, grown)


@pytest.mark.parametrize('fused', [True])          # (the unfused executor: test_other_learners_... and tests/test_fused_plumbing_cpu.py)
def test_learner_steps_free_their_tensors_by_refcount(cpu_learners, monkeypatch, fused):
  """Whole learner steps (teacher forward, quantisers, forward, losses, backward, optimiser) with Python's cyclic collector
  DISABLED: the bytes held by live tensors must not grow from step to step (see test_a_step_leaves_no_reference_cycles in
  tests/test_fused_plumbing_cpu.py for what a cycle costs on the GPU).  ResNet-50 bottlenecks, fused and unfused plumbing."""
  import gc
  import torch
  import pocketflow_amd.graph as G
  FLAGS, fake, tmp = cpu_learners
  from pocketflow_amd.nets.resnet_at_ilsvrc12 import ModelHelper
  from pocketflow_amd.learners.uniform_quantization.learner import UniformQuantLearner
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  if fused:
    monkeypatch.setattr(G, 'fusable_tensor', lambda t: True)
  FLAGS.batch_size, FLAGS.batch_size_eval, FLAGS.nb_classes, FLAGS.resnet_size, FLAGS.image_size = 2, 2, 11, 50, 32
  FLAGS.uql_weight_bits, FLAGS.uql_activation_bits = 8, 8
  FLAGS.enbl_dst, FLAGS.dst_eval_teacher = True, False
  FLAGS.uql_save_quant_model_path = str(tmp / 'uql' / 'm.ckpt')
  mh = ModelHelper()
  create_synthetic_checkpoint(mh)
  lrn = UniformQuantLearner(None, mh)

  def live_tensor_bytes():
    return sum(o.numel() * o.element_size() for o in gc.get_objects() if isinstance(o, torch.Tensor))
  lrn.train_step()
  gc.collect()
  gc.disable()
  try:
    lrn.train_step()
    base = live_tensor_bytes()
    for _ in range(3):
      lrn.train_step()
    grown = live_tensor_bytes() - base
  finally:
    gc.enable()
  assert grown <= 0, 'tensors of finished steps survive without the cyclic collector: +%d bytes over 3 steps' % grown


@pytest.mark.parametrize('use_buckets,bucket_type,opt_mode', [(False, 'split', 'weights'), (True, 'split', 'both'),
                                                              (True, 'channel', 'cluster')])
def test_nuq_resnet20_on_cpu(cpu_learners, use_buckets, bucket_type, opt_mode):
  FLAGS, fake, tmp = cpu_learners
  from oracle.learner_oracle import OracleLearner
  from pocketflow_amd.nets.resnet_at_cifar10 import ModelHelper
  from pocketflow_amd.learners.nonuniform_quantization.learner import NonUniformQuantLearner
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  FLAGS.batch_size, FLAGS.batch_size_eval, FLAGS.nb_classes, FLAGS.resnet_size = 8, 8, 10, 20
  FLAGS.nuql_weight_bits, FLAGS.nuql_activation_bits = 3, 32
  FLAGS.nuql_use_buckets, FLAGS.nuql_bucket_type, FLAGS.nuql_bucket_size, FLAGS.nuql_opt_mode = use_buckets, bucket_type, 128, opt_mode
  FLAGS.nuql_save_quant_model_path = str(tmp / 'nuql' / 'm.ckpt')
  mh = ModelHelper()
  create_synthetic_checkpoint(mh)
  lrn = NonUniformQuantLearner(None, mh)
  lrn.init_clusters()
  init = lrn.graph.store.export_numpy()
  ora = OracleLearner({k: v for k, v in init.items() if 'clusters' not in k},
                      _cfg(FLAGS, 'resnet', 'cifar_10', (32, 32, 3), learner='non-uniform', nuql_weight_bits=3,
                           nuql_use_buckets=use_buckets, nuql_bucket_type=bucket_type, nuql_bucket_size=128,
                           nuql_opt_mode=opt_mode, nuql_activation_bits=32), lrn.lrn_rate)
  nq = lrn.nonuni_quant
  by_var = {op.var.name: nq.cluster_vars[id(op.var)].name for op in nq.matmul_ops}
  for i, name in enumerate(ora.matmul_var_names):
    if i in ora.student.quant.codebooks:
      ref = ora.student.quant.codebooks[i].detach().numpy()
      assert np.array_equal(init[by_var[name]].reshape(ref.shape), ref), 'cluster_init of %s' % name
  pool = _pool(lrn.iter_train)
  for step in range(2):
    out = lrn.train_step()
    ref = ora.train_step(*pool[step % 2])
    assert abs(float(out['loss'].detach()) - ref['loss']) <= 1e-4 * max(1.0, abs(ref['loss'])), (step, float(out['loss']), ref['loss'])
  vals = lrn.graph.store.export_numpy()
  tol = 2 * 2 * lrn.lrn_rate(0) + 1e-5
  assert _max_rel(vals, {k: v for k, v in ora.export().items() if 'moving_' not in k}) <= tol
  for i, name in enumerate(ora.matmul_var_names):
    if i in ora.student.quant.codebooks:
      ref = ora.student.quant.codebooks[i].detach().numpy()
      assert np.max(np.abs(vals[by_var[name]].reshape(ref.shape) - ref)) <= tol, name


def test_ws_resnet20_on_cpu(cpu_learners):
  FLAGS, fake, tmp = cpu_learners
  from oracle import pf_oracle as O
  from oracle.learner_oracle import OracleLearner
  from pocketflow_amd.nets.resnet_at_cifar10 import ModelHelper
  from pocketflow_amd.learners.weight_sparsification.learner import WeightSparseLearner
  FLAGS.batch_size, FLAGS.batch_size_eval, FLAGS.nb_classes, FLAGS.resnet_size = 8, 8, 10, 20
  FLAGS.ws_prune_ratio, FLAGS.ws_prune_ratio_prtl, FLAGS.ws_mask_update_step = 0.5, 'uniform', 2
  FLAGS.ws_save_path = str(tmp / 'ws' / 'm.ckpt')
  FLAGS.nb_smpls_train, FLAGS.nb_epochs_rat = 8 * 12, 1.0 / 250
  lrn = WeightSparseLearner(None, ModelHelper())
  N = lrn.nb_iters_train
  assert N == 12
  ora = OracleLearner(lrn.graph.store.export_numpy(),
                      _cfg(FLAGS, 'resnet', 'cifar_10', (32, 32, 3), learner='weight-sparse', ws_prune_ratio=0.5,
                           ws_prune_ratio_prtl='uniform'), lrn.lrn_rate)
  refresh = set(O.ws_refresh_steps(N, 2))
  pool = _pool(lrn.iter_train)
  flips = 0
  for it in range(8):
    lr, loss, _ = lrn.train_step()
    ref = ora.train_step(*pool[it % 2])
    assert abs(float(loss.detach()) - ref['loss']) <= 2e-3 * max(1.0, abs(ref['loss'])), (it, float(loss), ref['loss'])
    if it in refresh:
      lrn.prune_step()
      ora.prune_step(N)
      for v in lrn.maskable_vars:
        m = v.to_ref(lrn.masks[v.offset:v.offset + v.numel].numpy())
        flips += int(np.sum(m != ora.masks[v.name]))
      # teacher forcing after a refresh (a mask is a step function of |w|; see tests/test_parity_gpu.py)
      lrn.graph.store.load_numpy(ora.export())
      for v in lrn.maskable_vars:
        sl = slice(v.offset, v.offset + v.numel)
        lrn.masks[sl] = torch.from_numpy(v.to_storage(ora.masks[v.name]).reshape(-1))
        lrn.var_bkup[sl] = torch.from_numpy(v.to_storage(ora.bkups[v.name]).reshape(-1))
  assert flips <= 8, flips
  for v in lrn.maskable_vars:
    m = lrn.masks[v.offset:v.offset + v.numel]
    assert abs(float(1 - m.mean()) - 0.5) <= 1.0 / m.numel() + 1e-6


def test_channel_pruned_mobilenet_on_cpu(cpu_learners, monkeypatch):
  """ChannelPrunedLearner end to end on the CPU (same shrunk configuration as tests/test_learner_gpu.py): taps,
  LASSO channel selection, least-squares reconstruction, mask construction and the masked fine-tune."""
  FLAGS, fake, tmp = cpu_learners
  import pocketflow_amd.learners.channel_pruning.learner as CP
  from pocketflow_amd.nets.mobilenet_at_ilsvrc12 import ModelHelper
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  monkeypatch.setattr(CP, 'hip', fake)
  monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
  FLAGS.batch_size, FLAGS.batch_size_eval, FLAGS.image_size, FLAGS.nb_classes = 8, 8, 32, 17
  FLAGS.mobilenet_depth_mult = 0.25
  FLAGS.cp_prune_option, FLAGS.cp_uniform_preserve_ratio, FLAGS.cp_nb_batches, FLAGS.cp_nb_points_per_layer = 'uniform', 0.5, 8, 10
  FLAGS.cp_channel_pruned_path = str(tmp / 'models' / 'pruned_model.ckpt')
  FLAGS.cp_best_path = str(tmp / 'models' / 'best_model.ckpt')
  FLAGS.cp_original_path = str(tmp / 'models' / 'original_model.ckpt')
  FLAGS.nb_iters_override, FLAGS.summ_step, FLAGS.synthetic_pool = 3, 2, 8
  mh = ModelHelper()
  create_synthetic_checkpoint(mh)
  lrn = CP.ChannelPrunedLearner(None, mh)
  rslt = lrn.train()
  assert np.isfinite(rslt['loss'])
  assert 0.2 < lrn.pruner.preserve_ratio < 0.7
  n_masked = 0
  for op in lrn.graph.matmul_ops:
    if op.name not in lrn.fake_pruning_dict or op.var.kind != 'conv':
      continue
    keep_in, keep_out = [np.asarray(k, bool) for k in lrn.fake_pruning_dict[op.name]]
    w = op.var.to_ref(op.var.master.detach().numpy())
    assert np.all(w[:, :, ~keep_in, :] == 0) and np.all(w[:, :, :, ~keep_out] == 0), op.name
    n_masked += int((~keep_in).sum() + (~keep_out).sum())
  assert n_masked > 0


def test_uq_rl_bit_search_on_cpu(cpu_learners, caplog):
  """`--uql_enbl_rl_agent`: DDPG roll-outs over per-layer bit widths, each rewarded by a short quantisation-aware
  fine-tune + evaluation (reference uq bit_optimizer.py:137-195), then the regular fine-tune with the best list."""
  import logging
  FLAGS, fake, tmp = cpu_learners
  from pocketflow_amd.nets.resnet_at_cifar10 import ModelHelper
  from pocketflow_amd.learners.uniform_quantization.learner import UniformQuantLearner
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  FLAGS.batch_size, FLAGS.batch_size_eval, FLAGS.nb_classes, FLAGS.resnet_size = 8, 8, 10, 8
  FLAGS.uql_weight_bits, FLAGS.uql_activation_bits, FLAGS.uql_use_buckets = 4, 32, False
  FLAGS.uql_enbl_rl_agent, FLAGS.uql_nb_rlouts, FLAGS.uql_tune_global_steps, FLAGS.uql_equivalent_bits = True, 8, 2, 5
  FLAGS.uql_tune_save_path = str(tmp / 'rl_tune' / 'model.ckpt')
  FLAGS.uql_save_quant_model_path = str(tmp / 'uql' / 'm.ckpt')
  FLAGS.ddpg_seed, FLAGS.nb_iters_override = 7, 2
  try:
    mh = ModelHelper()
    create_synthetic_checkpoint(mh)
    pretrained = None
    with caplog.at_level(logging.INFO, logger='pocketflow_amd'):
      lrn = UniformQuantLearner(None, mh)
    n = lrn.statistics['nb_matmuls']
    w_bits, a_bits = lrn.optimal_w_bit_list, lrn.optimal_a_bit_list
    assert len(w_bits) == n and a_bits == [32] * lrn.statistics['nb_activations']
    assert all(isinstance(b, int) and FLAGS.uql_w_bit_min <= b <= FLAGS.uql_w_bit_max for b in w_bits)
    used = sum(b * k for b, k in zip(w_bits, lrn.statistics['num_weights']))
    assert used <= sum(lrn.statistics['num_weights']) * 5                       # the bit budget holds
    assert lrn.ft_step == 0                                                     # ops['reset_ft_step'] after every tune
    rolls = [r for r in caplog.records if r.getMessage().startswith('#_rlout')]
    assert len(rolls) == 8
    assert sum('a-loss' in r.getMessage() for r in caplog.records) == 8
    # the agent's buffer (n * nb_rlouts // 4 rows) filled up after two roll-outs, so it did train
    assert any('c-loss = 0.00e+00' not in r.getMessage() for r in caplog.records if 'a-loss' in r.getMessage())
    assert len(set(r.getMessage() for r in rolls)) > 1                          # exploration: bit lists differ
    rslt = lrn.train()
    assert np.isfinite(rslt['loss'])
  finally:
    FLAGS.uql_enbl_rl_agent, FLAGS.ddpg_seed, FLAGS.nb_iters_override = False, -1, 0


@pytest.mark.parametrize('opt_mode,use_buckets', [('both', True), ('weights', False)])
def test_nuq_rl_bit_search_on_cpu(cpu_learners, caplog, opt_mode, use_buckets):
  """`--nuql_enbl_rl_agent`: codebooks are re-sized and re-initialised per roll-out (reference nuq bit_optimizer.py
  :227-238), fine-tuned with SGD when they are optimised, and the best list is used for the final fine-tune."""
  import logging
  FLAGS, fake, tmp = cpu_learners
  from pocketflow_amd.nets.resnet_at_cifar10 import ModelHelper
  from pocketflow_amd.learners.nonuniform_quantization.learner import NonUniformQuantLearner
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  FLAGS.batch_size, FLAGS.batch_size_eval, FLAGS.nb_classes, FLAGS.resnet_size = 8, 8, 10, 8
  FLAGS.nuql_weight_bits, FLAGS.nuql_activation_bits = 3, 32
  FLAGS.nuql_use_buckets, FLAGS.nuql_bucket_type, FLAGS.nuql_bucket_size, FLAGS.nuql_opt_mode = use_buckets, 'split', 128, opt_mode
  FLAGS.nuql_enbl_rl_agent, FLAGS.nuql_nb_rlouts, FLAGS.nuql_tune_global_steps, FLAGS.nuql_equivalent_bits = True, 6, 2, 3
  FLAGS.nuql_w_bit_max = 5
  FLAGS.nuql_tune_save_path = str(tmp / 'rl_tune' / 'model.ckpt')
  FLAGS.nuql_save_quant_model_path = str(tmp / 'nuql' / 'm.ckpt')
  FLAGS.ddpg_seed, FLAGS.nb_iters_override = 11, 2
  try:
    mh = ModelHelper()
    create_synthetic_checkpoint(mh)
    with caplog.at_level(logging.INFO, logger='pocketflow_amd'):
      lrn = NonUniformQuantLearner(None, mh)
    n = lrn.statistics['nb_matmuls']
    w_bits = lrn.optimal_w_bit_list
    assert len(w_bits) == n and all(2 <= b <= 5 for b in w_bits)
    assert sum(b * k for b, k in zip(w_bits, lrn.statistics['num_weights'])) <= 3 * sum(lrn.statistics['num_weights'])
    assert (lrn.optimizer_fintune is not None) == (opt_mode == 'both')
    nq = lrn.nonuni_quant
    # codebooks: allocated for 2**5 rows, the live 2**bits rows ascending per bucket, zeros behind
    vals = lrn.graph.store.export_numpy()
    lrn.nonuni_quant.feed_bits(w_bits, lrn.optimal_a_bit_list)
    lrn.init_clusters()
    vals = lrn.graph.store.export_numpy()
    for op, b in zip(nq.matmul_ops, w_bits):
      c = vals[nq.cluster_vars[id(op.var)].name]
      assert c.shape[0] == 32
      assert np.all(c[2 ** b:] == 0) and np.all(np.diff(c[:2 ** b], axis=0) >= 0) and np.any(c[:2 ** b] != 0)
    rslt = lrn.train()
    assert np.isfinite(rslt['loss'])
    vals = lrn.graph.store.export_numpy()
    for op, b in zip(nq.matmul_ops, w_bits):
      assert np.all(vals[nq.cluster_vars[id(op.var)].name][2 ** b:] == 0)        # dead rows never move
    assert len([r for r in caplog.records if r.getMessage().startswith('#_rlout')]) == 6
  finally:
    FLAGS.nuql_enbl_rl_agent, FLAGS.ddpg_seed, FLAGS.nb_iters_override, FLAGS.nuql_w_bit_max = False, -1, 0, 8


def test_inference_mode_bn_with_gradients(cpu_learners):
  """graph._BnActQuant in inference mode with gradients (frozen statistics, trainable gamma / beta) against plain torch autograd."""
  FLAGS, fake, tmp = cpu_learners
  import pocketflow_amd.graph as G
  g = G.Graph('model', 'cpu', torch.float32)
  bn = G.BatchNormAct(g, 'bn', 24, 'Relu', 0.997, 1e-5)
  g.finalize(requires_grad=True)
  rng = np.random.RandomState(0)
  with torch.no_grad():
    bn.gamma.tensor.copy_(torch.from_numpy((1 + 0.2 * rng.randn(24)).astype(np.float32)))
    bn.beta.tensor.copy_(torch.from_numpy((0.2 * rng.randn(24)).astype(np.float32)))
    bn.moving_mean.tensor.copy_(torch.from_numpy((0.3 * rng.randn(24)).astype(np.float32)))
    bn.moving_var.tensor.copy_(torch.from_numpy((0.5 + rng.rand(24)).astype(np.float32)))
  x = torch.from_numpy(rng.randn(4, 24, 5, 5).astype(np.float32)).contiguous(memory_format=torch.channels_last).requires_grad_(True)
  up = torch.from_numpy(rng.randn(4, 24, 5, 5).astype(np.float32))
  g.training = False
  with g.as_default():
    y = bn(x)
  (y * up).sum().backward()
  mm, mv = bn.moving_mean.tensor.clone(), bn.moving_var.tensor.clone()
  xr = x.detach().clone().requires_grad_(True)
  gam, bet = bn.gamma.tensor.detach().clone().requires_grad_(True), bn.beta.tensor.detach().clone().requires_grad_(True)
  yr = torch.relu((xr - mm.view(1, -1, 1, 1)) * torch.rsqrt(mv + 1e-5).view(1, -1, 1, 1) * gam.view(1, -1, 1, 1) + bet.view(1, -1, 1, 1))
  (yr * up).sum().backward()
  np.testing.assert_allclose(y.detach().numpy(), yr.detach().numpy(), rtol=1e-5, atol=1e-5)
  np.testing.assert_allclose(x.grad.numpy(), xr.grad.numpy(), rtol=1e-5, atol=1e-5)
  np.testing.assert_allclose(bn.gamma.tensor.grad.numpy(), gam.grad.numpy(), rtol=1e-4, atol=1e-4)
  np.testing.assert_allclose(bn.beta.tensor.grad.numpy(), bet.grad.numpy(), rtol=1e-4, atol=1e-4)
  assert torch.equal(bn.moving_mean.tensor, mm) and torch.equal(bn.moving_var.tensor, mv)      # statistics stay frozen


def test_ws_optimal_pruning_ratio_search_on_cpu(cpu_learners, monkeypatch, caplog):
  """`ws_prune_ratio_prtl=optimal` (the reference's default): DDPG roll-outs, each = masks from the full network +
  layer-wise regression + masked fine-tune on inference-mode networks (reference pr_optimizer.py:411-564)."""
  import logging
  FLAGS, fake, tmp = cpu_learners
  import pocketflow_amd.learners.weight_sparsification.pr_optimizer as PR
  from pocketflow_amd.nets.resnet_at_cifar10 import ModelHelper
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  from pocketflow_amd.learners.weight_sparsification.learner import WeightSparseLearner
  monkeypatch.setattr(PR, 'hip', fake)
  FLAGS.batch_size, FLAGS.batch_size_eval, FLAGS.nb_classes, FLAGS.resnet_size = 8, 8, 10, 8
  FLAGS.ws_prune_ratio, FLAGS.ws_prune_ratio_prtl, FLAGS.ws_reward_type = 0.6, 'optimal', 'single-obj'
  FLAGS.ws_nb_rlouts, FLAGS.ws_nb_rlouts_min, FLAGS.ws_nb_iters_rg, FLAGS.ws_nb_iters_ft, FLAGS.ws_nb_iters_feval = 4, 1, 2, 3, 2
  FLAGS.ws_save_path = str(tmp / 'ws' / 'm.ckpt')
  FLAGS.ddpg_seed, FLAGS.exec_mode = 5, 'train'
  try:
    mh = ModelHelper()
    create_synthetic_checkpoint(mh)
    with caplog.at_level(logging.INFO, logger='pocketflow_amd'):
      opt = PR.PROptimizer(mh, None)
      pairs = opt.run()
    names = [v.name for v in opt.vars_full['maskable']]
    assert [n for n, _ in pairs] == names and len(pairs) == 11           # ResNet-8: stem + 3 x (projection + 2 convs) + dense
    ratios = np.array([r for _, r in pairs])
    n = np.array([v.numel for v in opt.vars_full['maskable']], dtype=np.float64)
    assert ratios[0] == 0.0 and ratios[-1] == 0.0                      # CIFAR-10: head & tail stay dense
    assert np.all(ratios >= 0) and np.all(ratios <= 1 - 0.4 / 3 + 1e-6)
    assert np.sum(n * ratios) / np.sum(n) >= 0.6 - 1e-4                # single-objective: overall target is met
    assert len(opt.reward_history) == 4 and max(opt.reward_history) == opt.reward_history[int(np.argmax(opt.reward_history))]
    # the pruned network honours the masks after regression + fine-tune, and only maskable kernels are sparse
    st = opt.graph_prnd.store
    for v in opt.vars_prnd['maskable']:
      sl = slice(v.offset, v.offset + v.numel)
      assert float((st.w_master[sl] * (1 - opt.masks[sl])).abs().max()) == 0.0
    msgs = [r.getMessage() for r in caplog.records]
    assert sum(m.startswith('loss: ') for m in msgs) == 4 and sum('time consumption' in m for m in msgs) == 4
    # the learner consumes the searched ratios
    FLAGS.ws_nb_rlouts = 1
    lrn = WeightSparseLearner(None, mh)
    assert [n for n, _ in lrn.var_names_n_prune_ratios] == names
  finally:
    FLAGS.ws_prune_ratio_prtl, FLAGS.ddpg_seed = 'uniform', -1


def test_ws_optimal_rollout_pieces_on_cpu(cpu_learners, monkeypatch):
  """Masks = |w_full| > percentile(|w_full|, r * 100) (reference pr_optimizer.py:254-281); one layer-wise regression
  step = Adam on l2_loss(conv_i(pruned) - conv_i(full)) w.r.t. kernel i only, masked (:283-316)."""
  FLAGS, fake, tmp = cpu_learners
  from oracle import pf_oracle as O
  import pocketflow_amd.learners.weight_sparsification.pr_optimizer as PR
  from pocketflow_amd.nets.lenet_at_cifar10 import ModelHelper
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  monkeypatch.setattr(PR, 'hip', fake)
  FLAGS.batch_size, FLAGS.batch_size_eval, FLAGS.nb_classes = 8, 8, 10
  FLAGS.ws_prune_ratio, FLAGS.ws_prune_ratio_prtl, FLAGS.ws_nb_rlouts, FLAGS.ws_nb_rlouts_min = 0.5, 'optimal', 1, 1
  FLAGS.synthetic_pool = 1                                # every regression step sees the same batch
  lr_rg_saved, FLAGS.ws_lrn_rate_rg = FLAGS.ws_lrn_rate_rg, 1e-3
  try:
    mh = ModelHelper()
    create_synthetic_checkpoint(mh)
    opt = PR.PROptimizer(mh, None)
    opt.graph_full.store.load_numpy(__import__('pocketflow_amd.utils.checkpoint', fromlist=['x']).load(
        __import__('pocketflow_amd.utils.checkpoint', fromlist=['x']).latest_checkpoint(str(tmp / 'models'))), strict=False)
    full = opt.graph_full.store.export_numpy()
    ratios = [0.0, 0.5, 0.3, 0.7][:len(opt.vars_prnd['maskable'])]
    assert len(opt.vars_prnd['maskable']) == 4                       # LeNet: conv1, conv2, fc3, fc4 kernels
    opt._PROptimizer__init_pruned_network(ratios)
    prnd = opt.graph_prnd.store.export_numpy()
    for v_f, v_p, r in zip(opt.vars_full['maskable'], opt.vars_prnd['maskable'], ratios):
      w = full[v_f.name]
      thr = O.percentile_nearest(np.abs(w), np.float32(np.float32(r) * np.float32(100.0)))
      want_mask = (np.abs(w) > thr).astype(np.float32)
      got_mask = v_p.to_ref(opt.masks[v_p.offset:v_p.offset + v_p.numel].numpy())
      assert np.array_equal(got_mask, want_mask), v_p.name
      assert np.array_equal(prnd[v_p.name], w * want_mask)
    for name, val in prnd.items():                                   # everything else is a copy of the full network
      if name not in [v.name for v in opt.vars_prnd['maskable']]:
        assert np.array_equal(val, full[name.replace('pruned_model', 'model', 1)]), name

    # one regression step on conv2 (idx 1) against a direct computation
    idx, lr = 1, FLAGS.ws_lrn_rate_rg
    var = opt.vars_prnd['maskable'][idx]
    lf, lp = opt.core_full[idx], opt.core_prnd[idx]
    images, _ = opt.iter_trn.get_next()
    opt.iter_trn.reset()
    y_full = opt._PROptimizer__forward_tapped(opt.graph_full, images, lf)[lf][1]
    x_prnd = opt._PROptimizer__forward_tapped(opt.graph_prnd, images, lp)[lp][0]
    w0 = lp.kernel.tensor.detach().clone().requires_grad_(True)
    y = torch.nn.functional.conv2d(x_prnd, w0, lp.bias.tensor.detach(), stride=lp.stride, padding=2 if lp.padding == 'SAME' else 0)
    loss0 = ((y - y_full) ** 2).sum() / 2
    (g,) = torch.autograd.grad(loss0, w0)
    mask = opt.masks[var.offset:var.offset + var.numel].view(var.storage_shape)
    g_st = g.permute(0, 2, 3, 1).contiguous() * mask                       # logical OIHW -> storage KRSC
    p0 = var.master.detach().clone()
    want, _, _ = O.adam_step(p0.numpy().reshape(-1), g_st.numpy().reshape(-1), np.zeros(var.numel, np.float32),
                             np.zeros(var.numel, np.float32), 1, lr)
    before = opt.graph_prnd.store.export_numpy()
    st = opt.graph_prnd.store
    base = opt.opt_rg
    opt.rg_mask.zero_()
    opt.rg_mask[var.offset:var.offset + var.numel] = opt.masks[var.offset:var.offset + var.numel]
    base.w_mask, base.o_mask = opt.rg_mask, torch.zeros_like(st.o_master)
    losses = [float(opt._PROptimizer__regression_step(idx).detach()) for _ in range(4)]
    assert abs(losses[0] - float(loss0.detach())) <= 1e-4 * max(1.0, float(loss0.detach()))
    assert losses[-1] < losses[0]                                          # same batch every step: the loss falls
    after = opt.graph_prnd.store.export_numpy()
    for name in after:
      if name != var.name:
        assert np.array_equal(after[name], before[name]), name              # only the regressed kernel moves
    assert np.all(after[var.name][var.to_ref(mask.numpy()) == 0] == 0)       # pruned weights stay at zero
    # first Adam step: compare through a fresh optimiser state
    opt._PROptimizer__init_pruned_network(ratios)
    opt.iter_trn.reset()
    opt._PROptimizer__regression_step(idx)
    got = var.master.detach().numpy().reshape(-1)
    assert np.max(np.abs(got - want)) <= 2e-3 * lr + 1e-7
  finally:
    FLAGS.ws_prune_ratio_prtl, FLAGS.synthetic_pool, FLAGS.ws_lrn_rate_rg = 'uniform', 2, lr_rg_saved


def test_channel_pruned_auto_mode_on_cpu(cpu_learners, monkeypatch, caplog):
  """`cp_prune_option=auto` (the reference's default, cp learner.py:601-695): DDPG roll-outs over per-layer preserve
  ratios, the best strategy replayed through the list path, then the masked fine-tune."""
  import logging
  FLAGS, fake, tmp = cpu_learners
  import pocketflow_amd.learners.channel_pruning.learner as CP
  from pocketflow_amd.nets.mobilenet_at_ilsvrc12 import ModelHelper
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  monkeypatch.setattr(CP, 'hip', fake)
  monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
  FLAGS.batch_size, FLAGS.batch_size_eval, FLAGS.image_size, FLAGS.nb_classes = 8, 8, 32, 17
  FLAGS.mobilenet_depth_mult = 0.25
  FLAGS.cp_prune_option, FLAGS.cp_preserve_ratio, FLAGS.cp_nb_batches, FLAGS.cp_nb_points_per_layer = 'auto', 0.5, 4, 10
  FLAGS.cp_nb_rlouts, FLAGS.cp_nb_rlouts_min, FLAGS.cp_reward_policy = 3, 1, 'accuracy'
  FLAGS.cp_channel_pruned_path = str(tmp / 'models' / 'pruned_model.ckpt')
  FLAGS.cp_best_path = str(tmp / 'models' / 'best_model.ckpt')
  FLAGS.cp_original_path = str(tmp / 'models' / 'original_model.ckpt')
  FLAGS.nb_iters_override, FLAGS.summ_step, FLAGS.synthetic_pool, FLAGS.ddpg_seed = 2, 2, 4, 3
  try:
    mh = ModelHelper()
    create_synthetic_checkpoint(mh)
    lrn = CP.ChannelPrunedLearner(None, mh)
    with caplog.at_level(logging.INFO, logger='pocketflow_amd'):
      rslt = lrn.train()
    assert np.isfinite(rslt['loss'])
    assert len(lrn.reward_history) == 3 and lrn.bestinfo is not None
    strategy, acc, flops = lrn.bestinfo
    n_convs = len(lrn.pruner.thisconvs)
    assert len(strategy) == n_convs and strategy[0] == 1.0 and strategy[-1] == 1
    assert all(0 < r <= 1 for r in strategy)
    assert acc == max(lrn.reward_history)                                  # reward policy 'accuracy'
    # 'accuracy' policy: the constraint keeps the FLOP target reachable -> the replayed model meets it
    assert lrn.pruner.preserve_ratio <= 0.5 + 0.08, lrn.pruner.preserve_ratio
    assert abs(lrn.pruner.compute_model_flops(fake=True) - flops) <= 0.15 * flops     # replay (fresh samples) ~ best roll-out
    for op in lrn.graph.matmul_ops:
      if op.name in lrn.fake_pruning_dict and op.var.kind == 'conv':
        keep_in, keep_out = [np.asarray(k, bool) for k in lrn.fake_pruning_dict[op.name]]
        w = op.var.to_ref(op.var.master.detach().numpy())
        assert np.all(w[:, :, ~keep_in, :] == 0) and np.all(w[:, :, :, ~keep_out] == 0), op.name
  finally:
    FLAGS.cp_prune_option, FLAGS.ddpg_seed, FLAGS.nb_iters_override = 'uniform', -1, 0


@pytest.mark.parametrize('sampling,feature_bn', [('aligned', 'inference'), ('reference', 'train')])
def test_channel_pruned_resnet_uniform_on_cpu(cpu_learners, monkeypatch, sampling, feature_bn):
  """Residual network: convolutions fed by a residual sum keep their producer untouched (not W1-prunable) and the last
  convolution of a block is re-fitted against Y + residual_branch_diff (reference channel_pruner.py:579-586, 611-614).
  Second variant: the reference's own sampling (points per tensor name, projection shortcuts corrected too, batch-statistics
  BN) through the WHOLE prune + fine-tune run."""
  FLAGS, fake, tmp = cpu_learners
  import pocketflow_amd.learners.channel_pruning.learner as CP
  from pocketflow_amd.nets.resnet_at_cifar10 import ModelHelper
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  monkeypatch.setattr(CP, 'hip', fake)
  monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
  FLAGS.batch_size, FLAGS.batch_size_eval, FLAGS.nb_classes, FLAGS.resnet_size = 8, 8, 10, 8
  FLAGS.cp_prune_option, FLAGS.cp_uniform_preserve_ratio, FLAGS.cp_nb_batches, FLAGS.cp_nb_points_per_layer = 'uniform', 0.5, 4, 10
  FLAGS.cp_channel_pruned_path = str(tmp / 'models' / 'pruned_model.ckpt')
  FLAGS.cp_best_path = str(tmp / 'models' / 'best_model.ckpt')
  FLAGS.cp_original_path = str(tmp / 'models' / 'original_model.ckpt')
  FLAGS.nb_iters_override, FLAGS.summ_step, FLAGS.synthetic_pool = 2, 2, 4
  old_modes = (FLAGS.cp_sampling, FLAGS.cp_feature_bn)
  FLAGS.cp_sampling, FLAGS.cp_feature_bn = sampling, feature_bn
  try:
    mh = ModelHelper()
    create_synthetic_checkpoint(mh)
    lrn = CP.ChannelPrunedLearner(None, mh)
    rslt = lrn.train()
    assert np.isfinite(rslt['loss'])
    pr = lrn.pruner
    names = [c.op.name for c in pr.thisconvs]
    assert len(names) == 10                                      # stem + 3 x (projection, conv1, conv2)
    assert len(pr.last_in_resblock) == 3 and len(pr.feats_add) == 3
    assert len(pr.add_owner) == 6                                # conv2 AND the projection of every block feed its sum
    prunable = [pr.is_W1_prunable(c) for c in pr.thisconvs]
    # stem; block 1: projection + conv1 read BN(stem) (producer = stem), conv2 reads conv1; blocks 2, 3: fed by a sum
    assert prunable == [False, True, True, True, False, False, True, False, False, True]
    d = lrn.fake_pruning_dict
    for c, p in zip(pr.thisconvs[1:-1], prunable[1:-1]):
      assert 0 < sum(d[c.op.name][0]) < len(d[c.op.name][0])      # every inner layer lost input channels
    assert all(d[names[0]][0]) and all(d[names[-1]][0])           # first & final layer are never pruned
    assert 0.2 < pr.preserve_ratio < 0.8
  finally:
    FLAGS.nb_iters_override = 0
    FLAGS.cp_sampling, FLAGS.cp_feature_bn = old_modes


def test_proximal_shrink_against_numpy():
  """W <- W' * max(1 - tau / ||W'_c||, 0), tau = nearest-rank percentile of the channel norms
  (reference channel_pruning_gpu/learner.py:369-376)."""
  from oracle import pf_oracle as O
  from pocketflow_amd.learners.channel_pruning_gpu.learner import proximal_shrink
  rng = np.random.RandomState(0)
  w_hwio = (rng.randn(3, 3, 12, 7) * rng.rand(1, 1, 12, 1)).astype(np.float32)
  w_hwio[:, :, 5, :] = 0                                                # an already dead channel
  for perctl in (0.0, 10.0, 37.5, 50.0, 100.0):
    norm = np.sqrt(np.sum(np.square(w_hwio), axis=(0, 1, 3), keepdims=True))
    thr = O.percentile_nearest(norm, np.float32(perctl))
    with np.errstate(divide='ignore', invalid='ignore'):
      shrk = np.maximum(1.0 - thr / norm, 0.0)
    shrk = np.where(np.isnan(shrk), 0.0, shrk)
    want = w_hwio * shrk
    w_krsc = torch.from_numpy(np.ascontiguousarray(w_hwio.transpose(3, 0, 1, 2)).reshape(7, 9, 12))
    got, n = proximal_shrink(w_krsc, perctl)
    got_hwio = got.numpy().reshape(7, 3, 3, 12).transpose(1, 2, 3, 0)
    np.testing.assert_allclose(got_hwio, want, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(n.numpy(), norm.reshape(-1), rtol=1e-6)
    dead = int(np.sum(np.all(got_hwio == 0, axis=(0, 1, 3))))
    assert dead >= int(np.floor(12 * perctl / 100.0)) or perctl == 0.0


def test_cpg_proximal_step_oracle_and_plumbing():
  """oracle/pf_oracle.py cpg_proximal_step (restating channel_pruning_gpu/learner.py:379-383) against the torch expression the
  learner used until round 4 (`proximal_shrink`), and the learner's `proximal_step` plumbing (norms -> nearest-rank threshold ->
  shrink) over the emulated entry points."""
  from oracle import pf_oracle as O
  from fake_hip import FakeHipFull
  import pocketflow_amd.learners.channel_pruning_gpu.learner as CPG
  rng = np.random.RandomState(3)
  w_hwio = (rng.randn(3, 3, 24, 10) * rng.rand(1, 1, 24, 1)).astype(np.float32)
  g_hwio = rng.randn(3, 3, 24, 10).astype(np.float32)
  w_hwio[:, :, 7, :] = 0
  g_hwio[:, :, 7, :] = 0                                               # a dead channel stays dead
  fake = FakeHipFull()
  old = CPG.hip
  CPG.hip = fake
  try:
    for lr, perctl in ((1e-3, 0.0), (1e-2, 25.0), (5e-2, 50.0), (1e-3, 90.0)):
      want, norm, thr = O.cpg_proximal_step(w_hwio, g_hwio, lr, perctl)
      w_krsc = torch.from_numpy(np.ascontiguousarray(w_hwio.transpose(3, 0, 1, 2)).reshape(10, 9, 24))
      g_krsc = torch.from_numpy(np.ascontiguousarray(g_hwio.transpose(3, 0, 1, 2)).reshape(10, 9, 24))
      got, n = CPG.proximal_shrink(w_krsc - np.float32(lr) * g_krsc, perctl)
      np.testing.assert_allclose(got.numpy().reshape(10, 3, 3, 24).transpose(1, 2, 3, 0), want, rtol=5e-5, atol=1e-6)
      np.testing.assert_allclose(n.numpy(), norm, rtol=2e-6)
      w_flat, g_flat = w_krsc.clone().reshape(-1), g_krsc.reshape(-1)
      ws = (torch.empty(24), torch.empty(24), torch.empty(1), torch.empty(16, dtype=torch.int32))
      CPG.proximal_step(w_flat, g_flat, lr, perctl, 90, 24, ws)
      np.testing.assert_allclose(w_flat.numpy().reshape(10, 3, 3, 24).transpose(1, 2, 3, 0), want, rtol=5e-5, atol=1e-6)
      assert abs(float(ws[2][0]) - float(thr)) <= 2e-6 * max(1.0, float(thr))
      dead = int(np.sum(np.all(want == 0, axis=(0, 1, 3))))
      assert dead >= int(np.floor(24 * perctl / 100.0))
  finally:
    CPG.hip = old


def test_channel_pruned_gpu_learner_on_cpu(cpu_learners, monkeypatch, caplog):
  """'chn-pruned-gpu' (reference learners/channel_pruning_gpu/learner.py): proximal-gradient channel selection layer by
  layer against the full network, masked per-layer re-fit, masked whole-network fine-tune."""
  import logging
  FLAGS, fake, tmp = cpu_learners
  import pocketflow_amd.learners.channel_pruning_gpu.learner as CPG
  import pocketflow_amd.learners.weight_sparsification.learner as WS
  from pocketflow_amd.nets.resnet_at_cifar10 import ModelHelper
  from pocketflow_amd.learners.learner_utils import create_learner, create_synthetic_checkpoint
  monkeypatch.setattr(CPG, 'hip', fake)
  monkeypatch.setattr(WS, 'hip', fake)
  FLAGS.batch_size, FLAGS.batch_size_eval, FLAGS.nb_classes, FLAGS.resnet_size = 8, 8, 10, 8
  FLAGS.learner, FLAGS.cpg_prune_ratio, FLAGS.cpg_nb_iters_layer, FLAGS.cpg_lrn_rate_pgd_init = 'chn-pruned-gpu', 0.5, 6, 1e-6
  FLAGS.cpg_save_path = str(tmp / 'cpg' / 'model.ckpt')
  FLAGS.cpg_save_path_eval = str(tmp / 'cpg_eval' / 'model.ckpt')
  FLAGS.nb_iters_override, FLAGS.summ_step = 3, 2
  mh = ModelHelper()
  create_synthetic_checkpoint(mh)
  lrn = create_learner(None, mh)
  assert isinstance(lrn, CPG.ChannelPrunedGpuLearner) and lrn.nb_layers == 10
  full_before = lrn.graph_full.store.export_numpy()
  with caplog.at_level(logging.INFO, logger='pocketflow_amd'):
    rslt = lrn.train()
  assert np.isfinite(rslt['loss']) and 0.0 < rslt['pr_msk'] < 0.6
  vals = lrn.graph.store.export_numpy()
  for idx, var in enumerate(lrn.vars_prnd['maskable']):
    w = vals[var.name]
    dead = np.all(w == 0, axis=(0, 1, 3))
    m = var.to_ref(lrn.masks[var.offset:var.offset + var.numel].numpy())
    if idx in (0, lrn.nb_layers - 1):
      assert not dead.any() and np.all(m == 1)                          # head & tail are skipped
      continue
    cin = w.shape[2]
    assert dead.sum() >= cin // 2 and dead.sum() < cin, (var.name, dead.sum())      # >= 50 % of the input channels are gone
    assert np.array_equal(np.all(m == 0, axis=(0, 1, 3)), dead) and set(np.unique(m)) <= {0.0, 1.0}
    assert abs(lrn.actual_prune_ratios[idx] - dead.mean()) < 1e-9
  # the full network is untouched (weights and BN statistics)
  for k, v in lrn.graph_full.store.export_numpy().items():
    assert np.array_equal(v, full_before[k]), k
  assert sum('(actual)' in r.getMessage() for r in caplog.records) == 8


@pytest.mark.parametrize('net', ['resnet', 'lenet'])
def test_full_prec_learner_on_cpu(cpu_learners, monkeypatch, net):
  """FullPrecLearner (the teacher's trainer and the container of the frozen teacher): Momentum steps with the nets'
  own learning-rate schedule against the oracle learner."""
  FLAGS, fake, tmp = cpu_learners
  from oracle.learner_oracle import OracleLearner
  from pocketflow_amd.learners.full_precision.learner import FullPrecLearner
  monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
  FLAGS.batch_size, FLAGS.batch_size_eval, FLAGS.nb_classes = 8, 8, 10
  if net == 'resnet':
    from pocketflow_amd.nets.resnet_at_cifar10 import ModelHelper
    FLAGS.resnet_size = 20
  else:
    from pocketflow_amd.nets.lenet_at_cifar10 import ModelHelper
  lrn = FullPrecLearner(None, ModelHelper())
  ora = OracleLearner(lrn.graph.store.export_numpy(), _cfg(FLAGS, net, 'cifar_10', (32, 32, 3), learner='full-prec'), lrn.lrn_rate)
  pool = _pool(lrn.iter_train)
  for step in range(3):
    lr, loss, _ = lrn.train_step()
    ref = ora.train_step(*pool[step % 2])
    assert abs(float(loss.detach()) - ref['loss']) <= 1e-4 * max(1.0, abs(ref['loss'])), (step, float(loss), ref['loss'])
  assert _max_rel(lrn.graph.store.export_numpy(), {k: v for k, v in ora.export().items() if 'moving_' not in k}) <= 1e-4


def test_layerwise_tune_op_on_cpu(cpu_learners):
  """`uql_enbl_rl_layerwise_tune`: tune op n minimises mean((op(x, Q(w)) - op(x, w))^2) w.r.t. kernel n with its own
  Adam(1e-3) (reference uq utils.py:136-161).  Because the quantiser's range is wrapped in stop_gradient (:224-225) and
  Round is overridden by Identity (:185), dQ(w)/dw is exactly the identity: the gradient through the quantised op
  cancels the gradient through the full-precision op and the op never moves the kernel -- the reference's own
  "TODO: working not very well".  The product reproduces exactly that: the mismatch is reported, nothing changes."""
  FLAGS, fake, tmp = cpu_learners
  from oracle import pf_oracle as O
  from pocketflow_amd.nets.lenet_at_cifar10 import ModelHelper
  from pocketflow_amd.learners.uniform_quantization.learner import UniformQuantLearner
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  from pocketflow_amd.learners.layerwise import forward_tapped, layers_of_vars
  FLAGS.batch_size, FLAGS.batch_size_eval, FLAGS.nb_classes = 8, 8, 10
  FLAGS.uql_weight_bits, FLAGS.uql_activation_bits, FLAGS.uql_use_buckets = 2, 32, False
  FLAGS.synthetic_pool = 1
  mh = ModelHelper()
  create_synthetic_checkpoint(mh)
  lrn = UniformQuantLearner(None, mh)
  w_bits, a_bits = [2, 3], [32, 32, 32]
  names = [op.var.name for op in lrn.uni_quant.matmul_ops]
  assert len(names) == 2                                       # conv2 and fc3 (first & last layers stay full precision)
  before = lrn.graph.store.export_numpy()
  # diff of the dense layer against a direct computation (x = its input in the quantised training graph)
  images, _ = lrn.iter_train.get_next()
  lrn.iter_train.reset()
  lrn.uni_quant.feed_bits(w_bits, a_bits)
  layers = layers_of_vars(lrn.graph, lrn.forward_eval, images, [op.var for op in lrn.uni_quant.matmul_ops])
  lrn.graph.begin_step()
  lrn.uni_quant.quantize_weights()
  fc = layers[1]
  x = forward_tapped(lrn.graph, lrn.forward_train, images, fc, grad=True)[fc][0].detach().numpy()
  w = fc.kernel.to_ref(fc.kernel.master.detach().numpy())                       # [in, out]
  qw, _ = O.uniform_quantize(w, 3, 'weight')
  d = x @ qw - x @ w
  for n in (0, 1):
    diffs = [lrn.ops['layerwise_tune'](n, w_bits, a_bits) for _ in range(4)]
    assert all(np.isfinite(diffs)) and diffs[0] > 0 and len(set(diffs)) == 1, diffs
    if n == 1:
      assert abs(diffs[0] - float(np.mean(d * d))) <= 1e-5 * max(1.0, float(np.mean(d * d)))
  after = lrn.graph.store.export_numpy()
  for k in after:
    if 'moving_' not in k:
      assert np.array_equal(after[k], before[k]), k
  # and the bit search runs with the layer-wise phase switched on
  FLAGS.uql_enbl_rl_agent, FLAGS.uql_enbl_rl_layerwise_tune, FLAGS.uql_enbl_rl_global_tune = True, True, False
  FLAGS.uql_nb_rlouts, FLAGS.uql_tune_layerwise_steps, FLAGS.uql_equivalent_bits, FLAGS.ddpg_seed = 4, 2, 5, 1
  FLAGS.uql_tune_save_path = str(tmp / 'rl_tune' / 'model.ckpt')
  FLAGS.nb_eval_batches_override = 1
  lrn3 = UniformQuantLearner(None, mh)
  assert len(lrn3.optimal_w_bit_list) == 2 and all(2 <= b <= 8 for b in lrn3.optimal_w_bit_list)


@pytest.mark.parametrize('optimizer', ['adam', 'momentum'])
def test_cp_masked_finetune_matches_oracle_on_cpu(cpu_learners, monkeypatch, optimizer):
  """The channel-pruned learner's masked fine-tune against the oracle's 'channel' mode (oracle/learner_oracle.py
  _setup_cp; reference cp learner.py:381-471), HIP entry points emulated: same body as the GPU test."""
  import pocketflow_amd.learners.channel_pruning.learner as CP
  import pocketflow_amd.nets.mobilenet_at_ilsvrc12  # noqa: F401
  from parity_common import run_cp_masked_finetune
  FLAGS, fake, tmp = cpu_learners
  monkeypatch.setattr(CP, 'hip', fake)
  run_cp_masked_finetune(FLAGS, tmp, optimizer)


@pytest.mark.parametrize('model', ['resnet', 'mobilenet'])
def test_cp_feature_sampling_matches_oracle_on_cpu(cpu_learners, monkeypatch, model):
  """SURVEY 8a row a17 with the HIP entry points emulated: same body as the GPU test (tests/test_learner_gpu.py)."""
  import pocketflow_amd.learners.channel_pruning.learner as CP
  import pocketflow_amd.nets.mobilenet_at_ilsvrc12  # noqa: F401
  from parity_common import run_cp_feature_sampling_parity
  FLAGS, fake, tmp = cpu_learners
  monkeypatch.setattr(CP, 'hip', fake)
  r = run_cp_feature_sampling_parity(FLAGS, tmp, model)
  assert r['convs'] == (10 if model == 'resnet' else 15) and r['adds'] == (6 if model == 'resnet' else 0), r


@pytest.mark.parametrize('model,use_buckets,bucket_type,bits', [('lenet', True, 'split', 3), ('resnet', True, 'channel', 4), ('lenet', False, 'channel', 8)])
def test_int_export_of_a_uq_learner_on_cpu(cpu_learners, model, use_buckets, bucket_type, bits):
  """Integer export with the HIP entry points emulated: same body as the GPU test."""
  from parity_common import run_int_export_roundtrip
  FLAGS, fake, tmp = cpu_learners
  summ = run_int_export_roundtrip(FLAGS, tmp, model, use_buckets, bucket_type, bits)
  assert summ['quantised_tensors'] == (2 if model == 'lenet' else 21)       # ResNet-20: 23 matmul kernels, first and last stay float32


def test_teacher_ahead_gives_the_same_steps_on_cpu(cpu_learners, monkeypatch):
  """learners/teacher_ahead.py (PF_TEACHER_AHEAD, default on for HIP devices): the teacher's forward pass over batch k+1 issued at the end of step k.
  With the in-order stream stand-in the control flow runs on the CPU emulation: same batches in the same order, the same teacher
  logits, bit-identical losses and weights as the in-line teacher; one batch is always in flight after a step."""
  FLAGS, fake, tmp = cpu_learners
  from pocketflow_amd.nets.resnet_at_cifar10 import ModelHelper
  from pocketflow_amd.learners.uniform_quantization.learner import UniformQuantLearner
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  FLAGS.batch_size, FLAGS.batch_size_eval, FLAGS.nb_classes, FLAGS.resnet_size = 8, 8, 10, 20
  FLAGS.uql_weight_bits, FLAGS.uql_activation_bits, FLAGS.uql_use_buckets, FLAGS.uql_bucket_type = 8, 8, False, 'channel'
  FLAGS.enbl_dst, FLAGS.dst_eval_teacher = True, False
  FLAGS.uql_save_quant_model_path = str(tmp / 'uql' / 'm.ckpt')
  FLAGS.synthetic_pool = 3

  def run(mode):
    if mode is None:
      monkeypatch.delenv('PF_TEACHER_AHEAD', raising=False)
    else:
      monkeypatch.setenv('PF_TEACHER_AHEAD', mode)
    mh = ModelHelper()
    create_synthetic_checkpoint(mh)
    lrn = UniformQuantLearner(None, mh)
    losses = [(float(o['loss'].detach()), float(o['dst_loss'].detach())) for o in (lrn.train_step() for _ in range(4))]
    return lrn, losses

  base, l0 = run(None)
  assert getattr(base, '_teacher_ahead', 1) is None
  monkeypatch.setenv('PF_TEACHER_AHEAD', '1')
  from pocketflow_amd.learners import teacher_ahead
  assert teacher_ahead.make(base) is None                                    # a CPU device never gets the two-stream helper
  ahead, l1 = run('inline')
  h = ahead._teacher_ahead
  assert h is not None and h.n_issued == 4 and h.n_taken == 3 and h.pending is not None
  assert l0 == l1
  a, b = base.graph.store.export_numpy(), ahead.graph.store.export_numpy()
  assert all(np.array_equal(a[k], b[k]) for k in a)
  assert ahead.iter_train.idx == base.iter_train.idx + 1                      # exactly one batch prefetched
  # another consumer of the training iterator (layer-wise tuning) gets the prefetched batch first: same data order as without the helper
  nxt = teacher_ahead.next_images(ahead)
  assert h.pending is None and torch.equal(torch.as_tensor(nxt), torch.as_tensor(base.iter_train.batches[base.iter_train.idx % 3][0]))
  assert torch.equal(torch.as_tensor(teacher_ahead.next_images(ahead)), torch.as_tensor(base.iter_train.batches[(base.iter_train.idx + 1) % 3][0]))
  ahead.train_step()
  ahead._unget = [('images', 'labels')]                  # what a suspended step graph hands back
  teacher_ahead.drop(ahead)                             # iterator reset: neither the prefetched batch nor the handed-back ones survive
  assert h.pending is None and ahead._unget == []


def _run_steps(make, n, graph_mode, monkeypatch, suspend_at=(), FLAGS=None):
  """n train steps of a fresh learner, eager or through step_graph's in-line stand-in; returns (learner, per-step losses)."""
  from pocketflow_amd import step_graph
  if graph_mode:
    monkeypatch.setenv('PF_STEP_GRAPH', 'inline')
    monkeypatch.setenv('PF_STEP_GRAPH_STRICT', '1')
  else:
    monkeypatch.delenv('PF_STEP_GRAPH', raising=False)
  FLAGS.enbl_step_graph = bool(graph_mode)
  lrn = make()
  losses = []
  for i in range(n):
    if graph_mode and i in suspend_at:
      sg = step_graph.of(lrn)
      sg.suspend() if not sg.suspended else sg.resume()
    o = lrn.train_step()
    loss = o['loss'] if isinstance(o, dict) else o[1]
    losses.append(float(loss.detach()))
  return lrn, losses


@pytest.mark.parametrize('ahead', ['inline', '0'])
def test_step_graph_control_flow_uq_distillation_on_cpu(cpu_learners, monkeypatch, ahead):
  """pocketflow_amd/step_graph.py with the in-line stand-in for the hipGraph (the body is executed at every "replay"): static
  batch buffers, the teacher branch over the NEXT batch, the learning rate and Adam's bias correction fed through device memory
  (pf_adam_flat_dev), the hand-over of the prefetched batch between eager and recorded steps in both directions.  The steps must
  be the eager steps: same batches in the same order, bit-identical losses and weights, with and without the eager teacher-ahead
  helper and with the graph suspended for two steps in the middle."""
  FLAGS, fake, tmp = cpu_learners
  from pocketflow_amd.nets.resnet_at_cifar10 import ModelHelper
  from pocketflow_amd.learners.uniform_quantization.learner import UniformQuantLearner
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  from pocketflow_amd import step_graph
  FLAGS.batch_size, FLAGS.batch_size_eval, FLAGS.nb_classes, FLAGS.resnet_size = 8, 8, 10, 20
  FLAGS.uql_weight_bits, FLAGS.uql_activation_bits, FLAGS.uql_use_buckets, FLAGS.uql_bucket_type = 8, 8, False, 'channel'
  FLAGS.enbl_dst, FLAGS.dst_eval_teacher = True, False
  FLAGS.uql_save_quant_model_path = str(tmp / 'uql' / 'm.ckpt')
  FLAGS.synthetic_pool = 5
  monkeypatch.setenv('PF_TEACHER_AHEAD', ahead)

  def make():
    mh = ModelHelper()
    create_synthetic_checkpoint(mh)
    return UniformQuantLearner(None, mh)
  base, l0 = _run_steps(make, 11, False, monkeypatch, FLAGS=FLAGS)
  lrn, l1 = _run_steps(make, 11, True, monkeypatch, suspend_at=(6, 8), FLAGS=FLAGS)
  sg = step_graph.of(lrn)
  assert sg.state == 'ready' and sg.n_replays == 11 - 3 - 2 and sg.error is None
  assert lrn.optimizer.hp is not None and lrn.ft_step == base.ft_step == 11
  assert l0 == l1, (l0, l1)
  a, b = base.graph.store.export_numpy(), lrn.graph.store.export_numpy()
  assert all(np.array_equal(a[k], b[k]) for k in a)
  assert lrn.optimizer.beta1_power == base.optimizer.beta1_power and lrn.optimizer.beta2_power == base.optimizer.beta2_power
  # a change of bit widths voids the recording; the learner warms up and records again
  lrn._UniformQuantLearner__feed([4] * len(lrn.optimal_w_bit_list), lrn.optimal_a_bit_list)
  assert step_graph.of(lrn).state == 'warm'
  # another consumer of the training iterator (layer-wise tuning follows a bit-width feed) sees the batch the next step would have
  # seen -- the one the graph held in its static buffers -- and the step after it the following one: the eager run's order
  from pocketflow_amd.learners import teacher_ahead
  for _ in range(2):
    assert torch.equal(torch.as_tensor(teacher_ahead.next_images(lrn)), torch.as_tensor(teacher_ahead.next_images(base)))
  assert teacher_ahead.of(lrn) is None or teacher_ahead.of(lrn).pending is None
  for _ in range(5):
    lrn.train_step()
  assert step_graph.of(lrn).state == 'ready' and step_graph.of(lrn).n_replays == 6 + 2


@pytest.mark.parametrize('ahead', ['inline', '0'])
def test_step_graph_foreign_consumers_and_iterator_reset_keep_the_eager_data_order(cpu_learners, monkeypatch, ahead):
  """while a step graph is READY (not suspended) it holds the next two batches in its static buffers.  (1) Another
  consumer of the training iterator (`teacher_ahead.next_images`: layer-wise tuning) must get THOSE batches first, and the next plain
  step must resume the replays by itself; (2) `teacher_ahead.drop` + an iterator reset (the channel pruner's sampling pass) must
  forget them -- they belong to the iterator's previous pass -- instead of handing them back after the reset; (3) with
  PF_TEACHER_AHEAD=0 the helper that a suspended graph makes for the hand-over must not stay.  Reference: the eager run doing the same."""
  FLAGS, fake, tmp = cpu_learners
  from pocketflow_amd.nets.resnet_at_cifar10 import ModelHelper
  from pocketflow_amd.learners.uniform_quantization.learner import UniformQuantLearner
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  from pocketflow_amd.learners import teacher_ahead
  from pocketflow_amd import step_graph
  FLAGS.batch_size, FLAGS.batch_size_eval, FLAGS.nb_classes, FLAGS.resnet_size = 8, 8, 10, 20
  FLAGS.uql_weight_bits, FLAGS.uql_activation_bits, FLAGS.uql_use_buckets, FLAGS.uql_bucket_type = 8, 8, False, 'channel'
  FLAGS.enbl_dst, FLAGS.dst_eval_teacher = True, False
  FLAGS.uql_save_quant_model_path = str(tmp / 'uql' / 'm.ckpt')
  FLAGS.synthetic_pool = 7
  monkeypatch.setenv('PF_TEACHER_AHEAD', ahead)

  def make():
    mh = ModelHelper()
    create_synthetic_checkpoint(mh)
    return UniformQuantLearner(None, mh)

  def loss_of(o):
    return float(o['loss'].detach())

  def run(graph_mode):
    lrn, losses = _run_steps(make, 6, graph_mode, monkeypatch, FLAGS=FLAGS)
    if graph_mode:
      assert step_graph.of(lrn).state == 'ready' and not step_graph.of(lrn).suspended
    seen = [torch.as_tensor(teacher_ahead.next_images(lrn)).clone() for _ in range(2)]     # a foreign consumer, graph READY
    losses += [loss_of(lrn.train_step()) for _ in range(2)]
    if graph_mode:
      sg = step_graph.of(lrn)
      assert sg.state == 'ready' and not sg.suspended and sg.n_replays == 3 + 2          # resumed by itself
      if ahead == '0':
        assert getattr(lrn, '_teacher_ahead', None) is None                               # the hand-over helper did not stay
    teacher_ahead.drop(lrn)                                                               # as ChannelPrunedLearner.create_pruner does
    lrn.iter_train.reset()
    losses += [loss_of(lrn.train_step()) for _ in range(3)]
    return lrn, losses, seen
  base, l0, s0 = run(False)
  lrn, l1, s1 = run(True)
  assert all(torch.equal(a, b) for a, b in zip(s0, s1))
  assert l0 == l1, (l0, l1)
  a, b = base.graph.store.export_numpy(), lrn.graph.store.export_numpy()
  assert all(np.array_equal(a[k], b[k]) for k in a)
  assert step_graph.of(lrn).n_replays == 3 + 2 + 3 and getattr(lrn, '_unget', None) in (None, [])


@pytest.mark.parametrize('ahead', ['inline', '0'])
def test_step_graph_failed_recording_leaves_the_eager_run_untouched(cpu_learners, monkeypatch, ahead):
  """A recording that fails half-way (a library call that cannot be captured, hipStreamEndCapture refusing the graph): nothing of
  it executed on the device, so the eager path that takes over has to continue from the step counter and Adam powers of the last
  executed step, with the batches that were drawn for the static buffers first in line -- same losses and weights as a run that
  never tried."""
  FLAGS, fake, tmp = cpu_learners
  from pocketflow_amd.nets.resnet_at_cifar10 import ModelHelper
  from pocketflow_amd.learners.uniform_quantization.learner import UniformQuantLearner
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  from pocketflow_amd import step_graph
  FLAGS.batch_size, FLAGS.batch_size_eval, FLAGS.nb_classes, FLAGS.resnet_size = 8, 8, 10, 20
  FLAGS.uql_weight_bits, FLAGS.uql_activation_bits, FLAGS.uql_use_buckets, FLAGS.uql_bucket_type = 8, 8, False, 'channel'
  FLAGS.enbl_dst, FLAGS.dst_eval_teacher = True, False
  FLAGS.uql_save_quant_model_path = str(tmp / 'uql' / 'm.ckpt')
  FLAGS.synthetic_pool = 5
  monkeypatch.setenv('PF_TEACHER_AHEAD', ahead)

  def make():
    mh = ModelHelper()
    create_synthetic_checkpoint(mh)
    return UniformQuantLearner(None, mh)
  base, l0 = _run_steps(make, 7, False, monkeypatch, FLAGS=FLAGS)

  class Refusing(step_graph.InlineBackend):
    def capture(self, body):
      lrn = self.lrn
      # what the host side of a captured step does before the capture is refused (no launch of it ever executes)
      lrn.ft_step += 1
      lrn.optimizer.beta1_power = np.float32(lrn.optimizer.beta1_power * np.float32(0.9))
      lrn.optimizer.beta2_power = np.float32(lrn.optimizer.beta2_power * np.float32(0.999))
      raise RuntimeError('operation not permitted when stream is capturing')
  monkeypatch.setenv('PF_STEP_GRAPH', 'inline')
  monkeypatch.delenv('PF_STEP_GRAPH_STRICT', raising=False)
  FLAGS.enbl_step_graph = True
  lrn = make()
  sg = step_graph.of(lrn)
  sg.backend = Refusing()
  sg.backend.lrn = lrn
  l1 = [float(lrn.train_step()['loss'].detach()) for _ in range(7)]
  assert sg.state == 'failed' and isinstance(sg.error, RuntimeError) and sg.n_replays == 0
  assert lrn.ft_step == base.ft_step == 7 and not lrn.optimizer.hyper_external and not lrn.graph.capturing
  assert lrn.optimizer.beta1_power == base.optimizer.beta1_power and lrn.optimizer.beta2_power == base.optimizer.beta2_power
  assert l0 == l1, (l0, l1)
  a, b = base.graph.store.export_numpy(), lrn.graph.store.export_numpy()
  assert all(np.array_equal(a[k], b[k]) for k in a)


def test_step_graph_control_flow_ws_on_cpu(cpu_learners, monkeypatch):
  """... a learner without a teacher (no look-ahead batch), Momentum with the learning rate in device memory
  (pf_momentum_flat_dev), a mask refresh between recorded steps (the masks are updated in place: the recording stays valid)."""
  FLAGS, fake, tmp = cpu_learners
  from pocketflow_amd.nets.resnet_at_cifar10 import ModelHelper
  from pocketflow_amd.learners.weight_sparsification.learner import WeightSparseLearner
  from pocketflow_amd import step_graph
  FLAGS.batch_size, FLAGS.batch_size_eval, FLAGS.nb_classes, FLAGS.resnet_size = 8, 8, 10, 20
  FLAGS.ws_prune_ratio, FLAGS.ws_prune_ratio_prtl, FLAGS.ws_mask_update_step = 0.5, 'uniform', 2
  FLAGS.ws_save_path = str(tmp / 'ws' / 'm.ckpt')
  FLAGS.nb_smpls_train, FLAGS.nb_epochs_rat, FLAGS.synthetic_pool = 8 * 12, 1.0 / 250, 5

  def run(graph_mode):
    if graph_mode:
      monkeypatch.setenv('PF_STEP_GRAPH', 'inline')
      monkeypatch.setenv('PF_STEP_GRAPH_STRICT', '1')
    FLAGS.enbl_step_graph = graph_mode
    lrn = WeightSparseLearner(None, ModelHelper())
    losses = []
    for it in range(9):
      if graph_mode and it == 7:
        step_graph.of(lrn).suspend()
      losses.append(float(lrn.train_step()[1].detach()))
      if it in (4, 6):
        lrn.prune_step()
    return lrn, losses
  base, l0 = run(False)
  lrn, l1 = run(True)
  assert step_graph.of(lrn).state == 'ready' and step_graph.of(lrn).n_replays == 4
  assert l0 == l1, (l0, l1)
  a, b = base.graph.store.export_numpy(), lrn.graph.store.export_numpy()
  assert all(np.array_equal(a[k], b[k]) for k in a)
  assert torch.equal(base.masks, lrn.masks)


def test_step_graph_control_flow_mobilenet_dropout_on_cpu(cpu_learners, monkeypatch):
  """... a network that draws something on the host every step: MobileNet's (seed, step)-keyed dropout mask goes through
  graph.step_feeders; the recorded step and the eager step see the same mask sequence."""
  FLAGS, fake, tmp = cpu_learners
  from pocketflow_amd.nets.mobilenet_at_ilsvrc12 import ModelHelper
  from pocketflow_amd.learners.full_precision.learner import FullPrecLearner
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  import pocketflow_amd.utils.external.mobilenet_v1 as MV
  FLAGS.batch_size, FLAGS.batch_size_eval, FLAGS.image_size, FLAGS.nb_classes = 4, 4, 32, 11
  FLAGS.mobilenet_depth_mult, FLAGS.synthetic_pool = 0.25, 3
  net = None

  def masks(n_steps, capturing_at):
    mh = ModelHelper()
    create_synthetic_checkpoint(mh)
    lrn = FullPrecLearner(None, mh)
    g = lrn.graph
    with g.as_default():
      lrn.forward_train(lrn.to_device(*lrn.iter_train.get_next())[0])
    m = g.nets['mobilenet']
    m.keep = 0.5                                           # (0.999 would make every mask all-ones)
    # the CPU branch of dropout_mask draws per call; emulate the device branch's static buffer by hand
    m._mask_buf = torch.empty((4, m.features))
    g.step_feeders.append(m.feed_mask)
    out = []
    m.dropout_step = 0
    for i in range(n_steps):
      if i in capturing_at:                                # a recording: the buffer is read, nothing is fed, the counter stands
        g.capturing = True
        before = m.dropout_step
        assert m._mask_buf is not None and m.dropout_step == before
        g.capturing = False
        continue
      for f in g.step_feeders:
        f()
      out.append(m._mask_buf.clone())
    return out
  a = masks(5, ())
  b = masks(6, (2,))
  assert len(a) == len(b) == 5 and all(torch.equal(x, y) for x, y in zip(a, b))
  assert not torch.equal(a[0], a[1])
  ref = torch.from_numpy(MV.MobilenetV1._host_mask(type('S', (), {'dropout_seed': 2024, 'features': a[0].shape[1], 'keep': 0.5})(), 4, 3))
  assert torch.equal(a[3], ref)


def test_bf16_parity_bodies_of_the_other_configurations_on_cpu(cpu_learners, monkeypatch):
  """The bodies of the GPU tests `test_ws_resnet20_bf16_...`, `test_cp_mobilenet_bf16_...` and `test_nuq_resnet50_4bit_bf16_...`
  (tests/parity_common.py) with the HIP entry points emulated in float32: the plumbing of the checks themselves (bf16-storage
  oracle, per-variable floors, trajectories, bit-identical masks / codeword assignments) runs here before it costs GPU minutes."""
  FLAGS, fake, tmp = cpu_learners
  import pocketflow_amd.learners.channel_pruning.learner as CP
  from parity_common import run_ws_bf16_parity, run_nuq_bf16_parity, run_cp_masked_finetune
  monkeypatch.setattr(CP, 'hip', fake)
  run_ws_bf16_parity(FLAGS, tmp / 'ws', expect_bf16=False, batch=16)
  FLAGS.reset()
  FLAGS.save_path = str(tmp / 'cp' / 'models' / 'model.ckpt')
  FLAGS.synthetic_pool, FLAGS.compute_dtype = 2, 'float32'
  run_cp_masked_finetune(FLAGS, tmp / 'cp', 'adam', steps=2, bf16='emulated-float32')
  FLAGS.reset()
  FLAGS.save_path = str(tmp / 'nuq' / 'models' / 'model.ckpt')
  FLAGS.synthetic_pool, FLAGS.compute_dtype = 2, 'float32'
  run_nuq_bf16_parity(FLAGS, tmp / 'nuq', expect_bf16=False, batch=4, steps=1)
