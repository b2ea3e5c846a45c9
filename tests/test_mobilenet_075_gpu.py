"""MobileNet-v1 at depth multiplier 0.75 (24, 48, 96, 192, 384, 768 channels: C / 8 = 3 ... 96, none of which divides the 256-lane
workgroup) end to end, at 64 x 64, batch 8, 17 classes, float32.

Training: one step of the uniform-quantisation learner keeps all 13 depthwise layers on pf_depthwise.hip (13 launches of each of the
three entries, counted on the binding as tests/test_head_fused_gpu.py counts; DepthwiseConv2D._call_library never entered), and its
gradients and logits are as close to those of the library route (G.OWN_DEPTHWISE off: F.conv2d(groups=C), what this width ran on
before) as the two routes are at depth 0.5, where both have existed all along: with d = the largest per-variable max |a - b| / max |b|,
d(0.75) <= 2 d(0.5) -- the factor 2 for two different random networks, as in the d_on <= 2 d_off bars of the int8 tests.
Int8 inference: the recipe (bf16) and the bar of tests/test_int8_mobilenet_gpu.py on a synthetic 0.75 artefact."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BATCH = 8
_RUNS = {}
_ROOTS = {}


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


def _helper(tmp_path_factory, depth):
  """Flags for MobileNet-v1 `depth` and (once per depth) a synthetic checkpoint.  Returns the model helper."""
  from pocketflow_amd.flags import FLAGS
  import pocketflow_amd.learners.learner_utils  # noqa: F401  (defines flags)
  import pocketflow_amd.learners.abstract_learner  # noqa: F401
  import pocketflow_amd.datasets.abstract_dataset  # noqa: F401  (synthetic_pool)
  import pocketflow_amd.learners.uniform_quantization.learner  # noqa: F401
  import pocketflow_amd.nets.mobilenet_at_ilsvrc12 as net
  fresh = depth not in _ROOTS
  if fresh:
    _ROOTS[depth] = str(tmp_path_factory.mktemp('mobilenet_%03d' % round(depth * 100)))
  root = _ROOTS[depth]
  for k, v in dict(save_path=os.path.join(root, 'models', 'model.ckpt'), save_path_eval=os.path.join(root, 'models_eval', 'model.ckpt'),
                   uql_save_quant_model_path=os.path.join(root, 'uql', 'model.ckpt'), synthetic_pool=2, nb_eval_batches_override=2,
                   batch_size=BATCH, batch_size_eval=BATCH, uql_weight_bits=8, uql_activation_bits=8, uql_use_buckets=False,
                   enbl_dst=False, enbl_step_graph=False, compute_dtype='float32', mobilenet_version=1, mobilenet_depth_mult=depth,
                   nb_classes=17, image_size=64).items():
    setattr(FLAGS, k, v)
  mh = net.ModelHelper()
  if fresh:
    from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
    create_synthetic_checkpoint(mh)
  return mh


def _step(tmp_path_factory, depth, own):
  """One forward + backward of the learner's training step from the synthetic checkpoint (no update), on the in-tree depthwise
  kernels (`own`) or on the library route.  Returns dict(logits, grads, calls, library): float64 logits, {variable: gradient}, the
  launches of the three depthwise entries, the names of the layers that entered DepthwiseConv2D._call_library.  Kept per module."""
  key = (depth, own)
  if key in _RUNS:
    return _RUNS[key]
  from parity_common import product_gradients
  from pocketflow_amd import graph as G
  from pocketflow_amd import hip
  from pocketflow_amd.learners.uniform_quantization.learner import UniformQuantLearner
  mh = _helper(tmp_path_factory, depth)
  names = ('depthwise_fwd', 'depthwise_bwd_data', 'depthwise_wrw')
  calls = dict.fromkeys(names, 0)
  library = []
  mp = pytest.MonkeyPatch()
  try:
    mp.setattr(G, 'OWN_DEPTHWISE', own)
    learner = UniformQuantLearner(None, mh)
    assert len(learner.graph.depthwise_layers) == 13

    def counted(name, fn):
      def f(*a, **kw):
        calls[name] += 1
        return fn(*a, **kw)
      return f
    for n in names:
      mp.setattr(hip, n, counted(n, getattr(hip, n)))
    lib = G.DepthwiseConv2D._call_library
    mp.setattr(G.DepthwiseConv2D, '_call_library', lambda self, r, want_stats: (library.append(self.kernel.name), lib(self, r, want_stats))[1])
    seen = []
    forward = learner.forward_train
    learner.forward_train = lambda x: (seen.append(forward(x)), seen[-1])[1]
    out, grads = product_gradients(learner)
    torch.cuda.synchronize()
    assert len(seen) == 1 and tuple(seen[0].shape) == (BATCH, 17)
    assert bool(torch.isfinite(out['loss'].detach().float()).all())
    _RUNS[key] = dict(logits=seen[0].detach().double().cpu().numpy(), grads=grads, calls=dict(calls), library=list(library),
                      channels=sorted({dw.channels for dw in learner.graph.depthwise_layers}))
  finally:
    mp.undo()
  del learner
  torch.cuda.empty_cache()
  return _RUNS[key]


def _rel(a, b):
  return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()) / float(np.abs(np.asarray(b, np.float64)).max())


def test_a_training_step_at_075_keeps_every_depthwise_layer_on_the_in_tree_kernels(tmp_path_factory):
  run = _step(tmp_path_factory, 0.75, True)
  assert run['channels'] == [24, 48, 96, 192, 384, 768]
  assert run['library'] == []
  assert run['calls'] == dict(depthwise_fwd=13, depthwise_bwd_data=13, depthwise_wrw=13)
  for name, g in run['grads'].items():
    assert np.isfinite(g).all() and float(np.abs(g).max()) > 0.0, name


def test_own_route_against_library_route_at_075_as_close_as_at_050(tmp_path_factory):
  d = {}
  for depth in (0.75, 0.5):
    own, lib = _step(tmp_path_factory, depth, True), _step(tmp_path_factory, depth, False)
    # the switch did what it says: 13 layers on the library and no launch of the in-tree entries, and the reverse
    assert len(lib['library']) == 13 and not any(lib['calls'].values()), (depth, lib['calls'])
    assert own['library'] == [] and own['calls']['depthwise_fwd'] == 13
    assert sorted(own['grads']) == sorted(lib['grads'])
    per = {n: _rel(own['grads'][n], lib['grads'][n]) for n in own['grads']}
    worst = max(per, key=per.get)
    d[depth] = (per[worst], _rel(own['logits'], lib['logits']))
    print('mobilenet_v1 %.2f float32, own depthwise kernels against the library route: gradients %.3e (worst: %s), logits %.3e'
          % (depth, per[worst], worst, d[depth][1]))
  assert d[0.75][0] <= 2.0 * d[0.5][0], d
  assert d[0.75][1] <= 2.0 * d[0.5][1], d


def test_int8_inference_at_075_runs_repeats_and_stays_within_the_bar(tmp_path_factory):
  """tests/test_int8_mobilenet_gpu.py::test_mobilenet_logits_with_depthwise_on_int8 at depth 0.75: every depthwise layer that
  pf_dw_i8_fwd takes is packed and runs on codes, logits repeat bit for bit, and d_on <= 2 d_off against the float64 forward of that
  file -- in bf16, the compute type of that recipe and the one its bar was set for (the float path's own distance to float64 is the
  yardstick)."""
  from test_int8_mobilenet_gpu import _dist, forward64
  from pocketflow_amd import int8 as I8
  from pocketflow_amd.flags import FLAGS
  from pocketflow_amd.inference import load_int8
  from pocketflow_amd.learners.uniform_quantization.learner import UniformQuantLearner
  from pocketflow_amd.tools.conversion import export_quant_int8_model as E
  from pocketflow_amd.utils import checkpoint
  mh = _helper(tmp_path_factory, 0.75)
  FLAGS.compute_dtype = 'bfloat16'
  learner = UniformQuantLearner(None, mh)
  learner.restore_vars(checkpoint.latest_checkpoint(os.path.dirname(FLAGS.save_path)))
  path = os.path.join(_ROOTS[0.75], 'uql', 'model_int8.npz')
  assert E.export_from_learner(learner, path)['quantised_tensors'] >= 1
  del learner
  torch.cuda.empty_cache()
  images, _ = mh.dataset_train.make_batch(np.random.RandomState(5), BATCH)
  images = np.asarray(images, dtype=np.float32)
  g_off, fwd_off = load_int8(mh, path, 'cuda', torch.bfloat16, 8, int8='off')
  g_on, fwd_on = load_int8(mh, path, 'cuda', torch.bfloat16, 8, int8='on', depthwise='on')
  dw_names = {dw.kernel.name for dw in g_on.depthwise_layers}
  assert len(dw_names) == 13 and sorted({dw.channels for dw in g_on.depthwise_layers}) == [24, 48, 96, 192, 384, 768]
  # pf_dw_i8_fwd takes C % 16 == 0: the first depthwise layer (24 channels) stays on the float kernel, the other 12 are packed
  packed = {dw.kernel.name for dw in g_on.depthwise_layers if dw.int8 is not None}
  assert packed == {dw.kernel.name for dw in g_on.depthwise_layers if I8.depthwise_supported(dw.channels, dw.k, dw.stride)}
  assert len(packed) == 12 and g_off.nb_int8 == 0
  ref = forward64(g_off, mh, images, 8)
  off, on = fwd_off(images), fwd_on(images)
  torch.cuda.synchronize()
  assert torch.isfinite(on).all() and torch.isfinite(off).all()
  assert torch.equal(on, fwd_on(images)) and torch.equal(off, fwd_off(images))
  assert packed <= g_on.int8_ran and len(g_on.int8_ran) == g_on.nb_int8 and len(g_off.int8_ran) == 0
  d_off, d_on = _dist(off, ref), _dist(on, ref)
  print('mobilenet_at_ilsvrc12 0.75 bf16: %d int8 layers (12 depthwise); float path vs float64 %.3e; int8 with depthwise vs float64 %.3e'
        % (g_on.nb_int8, d_off, d_on))
  assert d_on <= 2.0 * d_off, (d_on, d_off)
