"""MobileNet-v2 1.0 at B = 256 / 224 x 224, bf16, one process and one build:

  census   which route each of the 52 convolutions + the logits layer took (Conv2D._route / DepthwiseConv2D._route) and which entry
           each BatchNorm ran, for one training step and one inference pass of the uniform-quantisation learner, plus every distinct
           GPU kernel name of that step with its launch count (torch.profiler): a convolution, batch-norm or add launch that is not one
           of the project's kernels shows there;
  time     the whole training step with the lazy depthwise route forced off and on (graph.DW_LAZY), the two alternating, median and
           spread (max - min) over the rounds: a uniform-quantisation run (w8 / a8) and a full-precision run.

  python tools/gpu/mobilenet_v2_step.py > profiles/mobilenet_v2_step.txt
"""
import argparse
import collections
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch


def _flags(args, work):
  from pocketflow_amd.flags import FLAGS
  import pocketflow_amd.learners.learner_utils  # noqa: F401  (defines flags)
  import pocketflow_amd.learners.abstract_learner  # noqa: F401
  import pocketflow_amd.datasets.abstract_dataset  # noqa: F401
  import pocketflow_amd.learners.uniform_quantization.learner  # noqa: F401
  import pocketflow_amd.nets.mobilenet_at_ilsvrc12 as net
  for k, v in dict(save_path=os.path.join(work, 'models', 'model.ckpt'), save_path_eval=os.path.join(work, 'models_eval', 'model.ckpt'),
                   uql_save_quant_model_path=os.path.join(work, 'uql', 'model.ckpt'), synthetic_pool=2, nb_eval_batches_override=1,
                   batch_size=args.batch, batch_size_eval=args.batch, uql_weight_bits=8, uql_activation_bits=8, uql_use_buckets=False,
                   enbl_dst=False, enbl_step_graph=False, compute_dtype='bfloat16', mobilenet_version=2, mobilenet_depth_mult=args.depth,
                   nb_classes=1001, image_size=args.size).items():
    setattr(FLAGS, k, v)
  return net.ModelHelper()


def _learner(kind, mh):
  if kind == 'uniform':
    from pocketflow_amd.learners.uniform_quantization.learner import UniformQuantLearner
    return UniformQuantLearner(None, mh)
  from pocketflow_amd.learners.full_precision.learner import FullPrecLearner
  return FullPrecLearner(None, mh)


def census(args, learner):
  from pocketflow_amd import graph as G
  from pocketflow_amd import hip
  routes, entries = [], collections.Counter()
  conv_route, dw_route = G.Conv2D._route, G.DepthwiseConv2D._route

  def conv(self, x, residual, out_bn):
    r = conv_route(self, x, residual, out_bn)
    t = x.x if isinstance(x, G.LazyAct) else x
    routes.append((self.kernel.name, 'k%d s%d %d->%d @%d' % (self.k, self.stride, self.kernel.ref_shape[2], self.kernel.ref_shape[3], t.shape[2]),
                   r[0] + (' (prologue)' if r[0] == 'conv1x1' and isinstance(r[1], G.LazyAct) else '')))
    return r

  def dw(self, x, out_bn):
    r = dw_route(self, x, out_bn)
    t = x.x if isinstance(x, G.LazyAct) else x
    routes.append((self.kernel.name, 'dw s%d C=%d @%d' % (self.stride, self.channels, t.shape[2]), r[0]))
    return r
  G.Conv2D._route, G.DepthwiseConv2D._route = conv, dw
  names = [n for n in dir(hip) if n.startswith(('bn_', 'depthwise_', 'conv', 'uq_', 'minmax_tensor', 'act_grad'))
           and callable(getattr(hip, n)) and not n.endswith(('_groups', '_splits', '_plan', '_supported', '_slabs', '_ok'))]
  saved = {n: getattr(hip, n) for n in names}

  def counted(n, fn):
    def f(*a, **kw):
      entries[n] += 1
      return fn(*a, **kw)
    return f
  for n in names:
    setattr(hip, n, counted(n, saved[n]))
  try:
    for lazy in (False, True):
      G.DW_LAZY = lazy
      for what in ('training step', 'inference pass'):
        routes.clear()
        entries.clear()
        if what == 'training step':
          learner.train_step()
        else:
          images, _ = learner.iter_eval.get_next() if hasattr(learner, 'iter_eval') else learner.iter_train.get_next()
          x, _ = learner.to_device(images, None)
          with torch.no_grad(), learner.graph.as_default():
            learner.forward_eval(x)
        torch.cuda.synchronize()
        print('## census, %s, PF_DW_LAZY=%d: %d convolution calls' % (what, lazy, len(routes)))
        by = collections.Counter(r[2] for r in routes)
        print('routes: ' + ', '.join('%s x %d' % kv for kv in sorted(by.items())))
        if lazy or what == 'inference pass':
          for name, geom, route in routes:
            print('  %-62s %-28s %s' % (name, geom, route))
        print('entries: ' + ', '.join('%s x %d' % kv for kv in sorted(entries.items())))
  finally:
    G.Conv2D._route, G.DepthwiseConv2D._route = conv_route, dw_route
    for n in names:
      setattr(hip, n, saved[n])
    G.DW_LAZY = None
  try:
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU], record_shapes=True) as prof:
      learner.train_step()
      torch.cuda.synchronize()
    kernels = collections.Counter()
    for ev in prof.events():
      if getattr(ev, 'device_type', None) is not None and 'cuda' in str(ev.device_type).lower():
        kernels[ev.name.split('(')[0][:110]] += 1
    print('## GPU kernels of one training step (default switches): %d launches, %d distinct names' % (sum(kernels.values()), len(kernels)))
    for k, v in sorted(kernels.items(), key=lambda kv: -kv[1]):
      print('  %4d  %s' % (v, k))
    # where the few aten element-wise launches come from: the operand shapes and dtypes of every aten add / mul call of the step
    ops = collections.Counter()
    for ev in prof.events():
      if ev.name in ('aten::add', 'aten::add_', 'aten::mul', 'aten::mul_', 'aten::sum'):
        ops[(ev.name, str(getattr(ev, 'input_shapes', '')), str(getattr(ev, 'input_dtypes', '') if hasattr(ev, 'input_dtypes') else ''))] += 1
    print('## aten add / mul / sum calls of that step (name, operand shapes, dtypes): %d' % sum(ops.values()))
    for (name, shapes, dtypes), v in sorted(ops.items(), key=lambda kv: -kv[1]):
      print('  %4d  %-10s %s %s' % (v, name, shapes, dtypes))
  except Exception as e:  # pylint: disable=broad-except
    print('## kernel names: profiler not available here (%s: %s)' % (type(e).__name__, e))


def step_times(args, kind, mh):
  from pocketflow_amd import graph as G
  learner = _learner(kind, mh)
  for lazy in (False, True):
    G.DW_LAZY = lazy
    for _ in range(3):
      learner.train_step()
  torch.cuda.synchronize()
  t = {False: [], True: []}
  for _ in range(args.rounds):
    for lazy in (False, True):
      G.DW_LAZY = lazy
      torch.cuda.synchronize()
      beg = time.perf_counter()
      for _ in range(args.steps):
        learner.train_step()
      torch.cuda.synchronize()
      t[lazy].append((time.perf_counter() - beg) / args.steps * 1e3)
  G.DW_LAZY = None
  for lazy in (False, True):
    med = statistics.median(t[lazy])
    print('%-8s PF_DW_LAZY=%d  step %8.3f ms (median of %d rounds of %d steps, spread %.3f ms)  %8.0f images/s'
          % (kind, lazy, med, args.rounds, args.steps, max(t[lazy]) - min(t[lazy]), args.batch / med * 1e3))
  del learner
  torch.cuda.empty_cache()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=256)
  ap.add_argument('--size', type=int, default=224)
  ap.add_argument('--depth', type=float, default=1.0)
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--steps', type=int, default=10)
  ap.add_argument('--skip_census', action='store_true')
  ap.add_argument('--skip_times', action='store_true')
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'mobilenet_v2_step.py measures on the GPU'
  with tempfile.TemporaryDirectory() as work:
    mh = _flags(args, work)
    from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
    create_synthetic_checkpoint(mh)
    print('# MobileNet-v2 %.2f, B = %d, %d x %d, bf16; the parent commit cannot run this network: there is no earlier number' %
          (args.depth, args.batch, args.size, args.size))
    if not args.skip_census:
      learner = _learner('uniform', mh)
      learner.train_step()
      census(args, learner)
      del learner
      torch.cuda.empty_cache()
    if args.skip_times:
      return
    print('## whole training step, lazy depthwise route off / on alternating')
    for kind in ('uniform', 'full'):
      step_times(args, kind, mh)


if __name__ == '__main__':
  main()
