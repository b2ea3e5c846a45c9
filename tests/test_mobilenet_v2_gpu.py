"""MobileNet-v2 at depth multiplier 0.5 end to end on the GPU, built like tests/test_mobilenet_075_gpu.py: 64 x 64, batch 8, 17 classes,
a synthetic checkpoint, the uniform-quantisation learner at w8 / a8 (and the full-precision learner), one forward + backward of the
learner's own training step without the parameter update.

The lazy depthwise route (graph.DepthwiseConv2D route `lazy`: the producer BN + ReLU6 + fake-quant in the prologue of
pf_depthwise_fwd_act / pf_depthwise_wrw_act) forced ON for every layer against forced OFF: logits, loss and every gradient bit for bit
-- the forward is identical by the kernels' definition (tests/test_depthwise_act_gpu.py), backward-data is the same kernel, and the
filter gradient is pinned there too.  Launches are counted on the binding, as tests/test_head_fused_gpu.py counts."""
import os

import numpy as np
import pytest
import torch

import mobilenet_v2_ref as R

pytestmark = pytest.mark.gpu

BATCH, CLASSES, SIZE, MULT = 8, 17, 64, 0.5
_RUNS = {}
_ROOTS = {}
_COUNTED = ('depthwise_fwd', 'depthwise_fwd_act', 'depthwise_bwd_data', 'depthwise_wrw', 'depthwise_wrw_act', 'bn_act_quant_apply',
            'bn_add_act_fwd', 'bn_add_act_bwd_gate')


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


def _helper(tmp_path_factory, dtype):
  from pocketflow_amd.flags import FLAGS
  import pocketflow_amd.learners.learner_utils  # noqa: F401  (defines flags)
  import pocketflow_amd.learners.abstract_learner  # noqa: F401
  import pocketflow_amd.datasets.abstract_dataset  # noqa: F401  (synthetic_pool)
  import pocketflow_amd.learners.uniform_quantization.learner  # noqa: F401
  import pocketflow_amd.nets.mobilenet_at_ilsvrc12 as net
  fresh = 'root' not in _ROOTS
  if fresh:
    _ROOTS['root'] = str(tmp_path_factory.mktemp('mobilenet_v2_050'))
  root = _ROOTS['root']
  for k, v in dict(save_path=os.path.join(root, 'models', 'model.ckpt'), save_path_eval=os.path.join(root, 'models_eval', 'model.ckpt'),
                   uql_save_quant_model_path=os.path.join(root, 'uql', 'model.ckpt'), synthetic_pool=2, nb_eval_batches_override=2,
                   batch_size=BATCH, batch_size_eval=BATCH, uql_weight_bits=8, uql_activation_bits=8, uql_use_buckets=False,
                   enbl_dst=False, enbl_step_graph=False, compute_dtype=dtype, mobilenet_version=2, mobilenet_depth_mult=MULT,
                   nb_classes=CLASSES, image_size=SIZE).items():
    setattr(FLAGS, k, v)
  mh = net.ModelHelper()
  if fresh:
    from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
    create_synthetic_checkpoint(mh)
  return mh


def _step(tmp_path_factory, kind='uniform', dtype='float32', lazy=True, own=True, tag=0):
  """One forward + backward of the learner's training step from the synthetic checkpoint (no update).  `lazy`: graph.DW_LAZY forced
  on / off; `own`: graph.OWN_DEPTHWISE.  Kept per module (`tag` tells repeats of one configuration apart)."""
  key = (kind, dtype, lazy, own, tag)
  if key in _RUNS:
    return _RUNS[key]
  from parity_common import product_gradients
  from pocketflow_amd import graph as G
  from pocketflow_amd import hip
  mh = _helper(tmp_path_factory, dtype)
  calls = dict.fromkeys(_COUNTED, 0)
  library = []
  mp = pytest.MonkeyPatch()
  try:
    mp.setattr(G, 'OWN_DEPTHWISE', own)
    mp.setattr(G, 'DW_LAZY', lazy)
    if kind == 'uniform':
      from pocketflow_amd.learners.uniform_quantization.learner import UniformQuantLearner
      learner = UniformQuantLearner(None, mh)
    else:
      from pocketflow_amd.learners.full_precision.learner import FullPrecLearner
      learner = FullPrecLearner(None, mh)
    g = learner.graph
    net = g.nets.get('mobilenet')
    weights = None

    def counted(name, fn):
      def f(*a, **kw):
        calls[name] += 1
        return fn(*a, **kw)
      return f
    for n in _COUNTED:
      mp.setattr(hip, n, counted(n, getattr(hip, n)))
    lib = G.DepthwiseConv2D._call_library
    mp.setattr(G.DepthwiseConv2D, '_call_library', lambda self, r, want_stats: (library.append(self.kernel.name), lib(self, r, want_stats))[1])
    seen = []
    forward = learner.forward_train

    def forward_train(x):
      seen.append((x.detach().float().cpu().numpy(), None))
      y = forward(x)
      seen[-1] = (seen[-1][0], y)
      return y
    learner.forward_train = forward_train
    out, grads = product_gradients(learner)
    torch.cuda.synchronize()
    loss = out['loss'] if isinstance(out, dict) else out[1]
    assert len(seen) == 1 and tuple(seen[0][1].shape) == (BATCH, CLASSES)
    assert bool(torch.isfinite(loss.detach().float()).all())
    g, net = learner.graph, learner.graph.nets['mobilenet']
    weights = g.store.export_numpy()               # the masters: the step above made no update
    _RUNS[key] = dict(logits=seen[0][1].detach().double().cpu().numpy(), loss=float(loss.detach().double()), grads=grads, calls=dict(calls),
                      library=list(library), images=seen[0][0], weights=weights, mask=net._host_mask(BATCH, 0),
                      n_dw=len(g.depthwise_layers), n_join=len(g.join_layers),
                      n_lazy_producers=sum(b.expand_bn is not None for b in net.blocks) + 1)
  finally:
    mp.undo()
  del learner
  torch.cuda.empty_cache()
  return _RUNS[key]


def _same_bits(a, b):
  assert a['loss'] == b['loss'], (a['loss'], b['loss'])
  assert np.array_equal(a['logits'], b['logits'])
  assert sorted(a['grads']) == sorted(b['grads'])
  for name in a['grads']:
    assert np.array_equal(a['grads'][name], b['grads'][name]), name


def test_lazy_on_equals_lazy_off_bit_for_bit_and_takes_the_fused_entries(tmp_path_factory):
  on, off = _step(tmp_path_factory, lazy=True), _step(tmp_path_factory, lazy=False)
  assert on['n_dw'] == 17 == on['n_lazy_producers'] and on['n_join'] == 10
  _same_bits(on, off)
  for name, g in on['grads'].items():
    assert np.isfinite(g).all() and float(np.abs(g).max()) > 0.0, name
  # ON: every depthwise layer has a lazy producer (the stem's BN, sixteen expansions) and took the fused pair; no plain launch, no
  # apply pass for those seventeen BNs, the library never entered
  assert on['library'] == [] == off['library']
  assert on['calls']['depthwise_fwd_act'] == 17 == on['calls']['depthwise_wrw_act']
  assert on['calls']['depthwise_fwd'] == 0 == on['calls']['depthwise_wrw']
  assert off['calls']['depthwise_fwd'] == 17 == off['calls']['depthwise_wrw'] and off['calls']['depthwise_fwd_act'] == 0 == off['calls']['depthwise_wrw_act']
  assert on['calls']['depthwise_bwd_data'] == 17 == off['calls']['depthwise_bwd_data']
  assert off['calls']['bn_act_quant_apply'] - on['calls']['bn_act_quant_apply'] == 17
  # the ten joins: one forward pass each plus the five sums of a forked block input; the gate pass only where a block output has two readers
  assert on['calls']['bn_add_act_fwd'] == 15 and on['calls']['bn_add_act_bwd_gate'] == 5


def test_own_kernels_against_the_library_route_both_against_float64(tmp_path_factory):
  """d_own <= 2 d_library, both the distance of the step's logits to the float64 restatement (tests/mobilenet_v2_ref.py) on the same
  master weights, batch and dropout mask: the project's bar for two float routes of one network.  (The restatement does not quantise:
  both distances carry the w8 / a8 quantisation noise.)"""
  own, lib = _step(tmp_path_factory, lazy=True), _step(tmp_path_factory, lazy=False, own=False)
  assert len(lib['library']) == 17 and not any(lib['calls'][k] for k in _COUNTED if k.startswith('depthwise')), lib['calls']
  assert np.array_equal(own['images'], lib['images']) and np.array_equal(own['mask'], lib['mask'])
  ref = R.forward(own['weights'], own['images'], MULT, True, mask=own['mask']).numpy()
  d = {k: float(np.abs(r['logits'] - ref).max() / np.abs(ref).max()) for k, r in (('own', own), ('library', lib))}
  print('mobilenet_v2 0.5 float32 w8/a8, logits against the float64 restatement: own kernels (lazy route) %.3e, library route %.3e'
        % (d['own'], d['library']))
  assert d['own'] <= 2.0 * d['library'], d


def test_bf16_step_is_finite_and_repeats_bit_for_bit(tmp_path_factory):
  a, b = _step(tmp_path_factory, dtype='bfloat16', lazy=True, tag=0), _step(tmp_path_factory, dtype='bfloat16', lazy=True, tag=1)
  assert np.isfinite(a['logits']).all() and np.isfinite(a['loss'])
  for name, g in a['grads'].items():
    assert np.isfinite(g).all(), name
  _same_bits(a, b)
  assert a['calls']['depthwise_fwd_act'] == 17 == a['calls']['depthwise_wrw_act'] and a['library'] == []


def test_bf16_lazy_on_equals_lazy_off(tmp_path_factory):
  _same_bits(_step(tmp_path_factory, dtype='bfloat16', lazy=True, tag=0), _step(tmp_path_factory, dtype='bfloat16', lazy=False))


@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
def test_full_precision_learner_lazy_on_equals_lazy_off(tmp_path_factory, dtype):
  on, off = _step(tmp_path_factory, kind='full', dtype=dtype, lazy=True), _step(tmp_path_factory, kind='full', dtype=dtype, lazy=False)
  assert np.isfinite(on['logits']).all() and np.isfinite(on['loss'])
  _same_bits(on, off)
  assert on['calls']['depthwise_fwd_act'] == 17 == on['calls']['depthwise_wrw_act'] and on['calls']['depthwise_fwd'] == 0
  assert off['calls']['depthwise_fwd_act'] == 0 and off['calls']['depthwise_fwd'] == 17


def test_inference_pass_lazy_on_equals_lazy_off(tmp_path_factory):
  """A full-precision evaluation forward (no gradients, moving statistics): the lazy route in inference, bit for bit."""
  from pocketflow_amd import graph as G
  from pocketflow_amd import hip
  from pocketflow_amd.learners.full_precision.learner import FullPrecLearner
  mh = _helper(tmp_path_factory, 'bfloat16')
  mp = pytest.MonkeyPatch()
  outs, calls = {}, {}
  try:
    learner = FullPrecLearner(None, mh)
    g = learner.graph
    x = torch.randn(BATCH, 3, SIZE, SIZE, device='cuda', generator=torch.Generator(device='cuda').manual_seed(3)).to(torch.bfloat16)
    x = x.contiguous(memory_format=torch.channels_last)
    n = [0]
    fused = hip.depthwise_fwd_act
    mp.setattr(hip, 'depthwise_fwd_act', lambda *a, **kw: (n.__setitem__(0, n[0] + 1), fused(*a, **kw))[1])
    for lazy in (True, False):
      mp.setattr(G, 'DW_LAZY', lazy)
      n[0] = 0
      with torch.no_grad(), g.as_default():
        outs[lazy] = learner.forward_eval(x).float().cpu()
      calls[lazy] = n[0]
    torch.cuda.synchronize()
  finally:
    mp.undo()
  assert calls[True] == 17 and calls[False] == 0
  assert torch.isfinite(outs[True]).all() and torch.equal(outs[True], outs[False])
