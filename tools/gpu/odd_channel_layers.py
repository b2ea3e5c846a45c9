"""Channel counts whose groups of 8 do not divide the 256-lane workgroup (MobileNet-v1 at depth multiplier 0.75: 24 ... 768 channels),
layer by layer and as a whole model, bf16, batch 256 at 224 x 224.

  depthwise  the 13 depthwise layers of MobileNet-v1 0.75, forward (+ BN statistics), backward-data, backward-filter: the in-tree
             kernels (pf_depthwise.hip, general lane map) against the library route the layers took before (F.conv2d(groups=C) and
             aten's convolution_backward on the explicitly padded input, as DepthwiseConv2D._call_library runs it), and beside each
             row the in-tree kernels on the neighbouring layer of width 1.0 (a power of two: every lane busy), as time per byte.
  pow2       the 13 layers of width 1.0 on this build and on another build of the library (--other_lib: the parent commit's),
             through the raw C entries of both, alternating: the shapes that were supported before must keep their timings.
  bn         the BatchNorm / quantiser passes at rows x C = 256 * 112^2 x 24 ... 256 * 7^2 x 768: the 16-byte vector route (aligned
             tensors) against the scalar route, which the same entry takes for a copy placed 4 bytes off 16-byte alignment.
  artefact   writes a synthetic int8 artefact of the 0.75 network (what tools/benchmark/calc_inference_time.py loads).
  model      calc_inference_time on that artefact and a timed training step of the uniform-quantisation learner (w8 / a8, no
             distillation), of the package under --tree (default: this checkout): run on two checkouts in turn for parent against
             branch.

Without --section the tool is the driver: every section runs in a child process of its own under its own time limit, in the order
above, and the first child that fails ends the run.  With --parent_tree DIR (a built checkout of the parent commit) the driver adds
the `pow2` section against that tree's library and alternates the `model` section between the two trees for --model_rounds rounds.

Every time is a device-event time of `iters` back-to-back calls; routes alternate inside every round and the tables give the median
and the spread (max - min) over the rounds.  Bytes are counted from the shapes.  The smallest layers (7 x 7) take ~10 us: there the
host's enqueue rate bounds both routes alike.

Usage: python tools/gpu/odd_channel_layers.py [--out FILE] [--parent_tree DIR] [--rounds 5] [--iters 10]"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
# (input size, channels at depth multiplier 1, stride) of the depthwise layers, utils/external/mobilenet_v1.py _CONV_DEFS
LAYERS = [(112, 32, 1), (112, 64, 2), (56, 128, 1), (56, 128, 2), (28, 256, 1), (28, 256, 2), (14, 512, 1), (14, 512, 1),
          (14, 512, 1), (14, 512, 1), (14, 512, 1), (14, 512, 2), (7, 1024, 1)]
BN_ROWS = [(112, 24), (56, 96), (28, 192), (14, 384), (7, 768)]
SECTION_TIMEOUT = dict(depthwise=300, pow2=240, bn=300, artefact=300, model=300)


def same(size, stride):
  out = -(-size // stride)
  total = max((out - 1) * stride + 3 - size, 0)
  return total // 2, total - total // 2, out


def time_us(fn, iters):
  import torch
  a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for _ in range(iters):
    fn()
  e.record()
  torch.cuda.synchronize()
  return a.elapsed_time(e) / iters * 1e3


def alternate(fns, rounds, iters):
  """{name: (median us, spread us)} of the routes in `fns`, alternating inside every round, after two warm-up calls each."""
  import torch
  for fn in fns.values():
    fn()
    fn()
  torch.cuda.synchronize()
  t = {k: [] for k in fns}
  for _ in range(rounds):
    for k, fn in fns.items():
      t[k].append(time_us(fn, iters))
  return {k: (statistics.median(v), max(v) - min(v)) for k, v in t.items()}


class DwLayer(object):
  """The tensors of one depthwise layer and its three passes on the in-tree kernels (through `lib`: a ctypes handle of a build of the
  library; None = the binding) and on the library route."""

  def __init__(self, B, H, C, stride):
    import torch
    import torch.nn.functional as F
    from pocketflow_amd import hip
    self.hip, self.dims = hip, (B, H, C, stride)
    ph0, ph1, Ho = same(H, stride)
    self.ph, self.Ho = ph0, Ho
    g = torch.Generator(device='cuda').manual_seed(H + C + stride)
    cl = torch.channels_last
    self.x = torch.randn(B, C, H, H, device='cuda', generator=g).bfloat16().contiguous(memory_format=cl)
    self.w = (torch.randn(C, 3, 3, device='cuda', generator=g) * 0.3).bfloat16()
    self.dy = torch.randn(B, C, Ho, Ho, device='cuda', generator=g).bfloat16().contiguous(memory_format=cl)
    self.y = torch.empty(B, C, Ho, Ho, device='cuda', dtype=torch.bfloat16).contiguous(memory_format=cl)
    self.dx = torch.empty_like(self.x)
    self.dw = torch.empty(C, 3, 3, device='cuda', dtype=torch.bfloat16)
    self.G = hip.depthwise_groups(B, Ho, Ho, C)
    self.partial = torch.empty(self.G, 4, C, device='cuda')
    self.slabs = torch.empty((self.G + 32) * C * 9, device='cuda')
    # DepthwiseConv2D._call_library: TF 'SAME' pads that differ front / behind become a padded copy (made per call, as the layer does)
    self.sym = ph0 == ph1
    self.pad4 = (ph0, ph1, ph0, ph1)
    self.w4 = self.w.reshape(C, 1, 3, 3)
    self.F = F
    self.nbytes = (B * H * H * C + B * Ho * Ho * C) * 2

  def own(self, lib=None):
    B, H, C, s = self.dims
    hip, ph, Ho = self.hip, self.ph, self.Ho
    if lib is None:
      return dict(fwd=lambda: hip.depthwise_fwd(self.x, self.w, self.y, B, H, H, C, 3, s, ph, ph, Ho, Ho, partial=self.partial),
                  bwd=lambda: hip.depthwise_bwd_data(self.dy, self.w, self.dx, B, H, H, C, 3, s, ph, ph, Ho, Ho),
                  wrw=lambda: hip.depthwise_wrw(self.dy, self.x, self.dw, self.slabs, B, H, H, C, 3, s, ph, ph, Ho, Ho))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    geom = [ctypes.c_int(v) for v in (B, H, H, C, 3, s, ph, ph, Ho, Ho)]
    bf16 = ctypes.c_int(hip.PF_BF16)

    def check(err):
      if err != 0:
        raise RuntimeError('depthwise entry failed: hipError %d' % err)
    return dict(fwd=lambda: check(lib.pf_depthwise_fwd(p(self.x), p(self.w), p(self.y), bf16, p(self.partial), *geom, hip._stream())),
                bwd=lambda: check(lib.pf_depthwise_bwd_data(p(self.dy), p(self.w), p(self.dx), bf16, *geom, hip._stream())),
                wrw=lambda: check(lib.pf_depthwise_wrw(p(self.dy), p(self.x), p(self.dw), bf16, bf16, p(self.slabs), *geom, hip._stream())))

  def library(self):
    import torch
    B, H, C, s = self.dims
    F, w4 = self.F, self.w4
    pad = [self.ph, self.ph] if self.sym else [0, 0]
    xin = (lambda: self.x) if self.sym else (lambda: F.pad(self.x, self.pad4))      # forward: the copy is part of the call
    xp = xin()                                                                      # backward: autograd kept the padded input
    bw = lambda mask: torch.ops.aten.convolution_backward(self.dy, xp, w4, None, [s, s], pad, [1, 1], False, [0, 0], C, mask)
    return dict(fwd=lambda: F.conv2d(xin(), w4, None, stride=s, padding=tuple(pad), groups=C),
                bwd=lambda: bw([True, False, False]), wrw=lambda: bw([False, True, False]))


def section_depthwise(args, say):
  import torch
  from pocketflow_amd import hip
  say('depthwise 3x3, MobileNet-v1 %.2f, batch %d, bf16: in-tree kernels against the library route; %d rounds of %d calls, alternating'
      % (args.depth, args.batch, args.rounds, args.iters))
  say('device: %s' % torch.cuda.get_device_name(0))
  say('%-16s %-5s | %9s %7s %6s | %9s %7s | %7s | %-14s %9s %6s %8s' % (
      'H, C, stride', 'pass', 'own us', 'spread', 'TB/s', 'lib us', 'spread', 'own/lib', 'neighbour 1.0', 'own us', 'TB/s', 'ps/B rat'))
  tot = dict(own=0.0, lib=0.0)
  for H, C1, stride in LAYERS:
    C = max(8, int(C1 * args.depth))
    assert hip.depthwise_supported(C, 3, stride), C
    lay, ngb = DwLayer(args.batch, H, C, stride), DwLayer(args.batch, H, C1, stride)
    own, lib, nown = lay.own(), lay.library(), ngb.own()
    for k in ('fwd', 'bwd', 'wrw'):
      r = alternate({'own': own[k], 'lib': lib[k], 'ngb': nown[k]}, args.rounds, args.iters)
      per_byte = (r['own'][0] / lay.nbytes) / (r['ngb'][0] / ngb.nbytes)
      say('%-16s %-5s | %9.1f %7.1f %6.2f | %9.1f %7.1f | %7.3f | %-14s %9.1f %6.2f %8.3f' % (
          '%d, %d, %d' % (H, C, stride), k, r['own'][0], r['own'][1], lay.nbytes / r['own'][0] / 1e6, r['lib'][0], r['lib'][1],
          r['own'][0] / r['lib'][0], '%d, %d, %d' % (H, C1, stride), r['ngb'][0], ngb.nbytes / r['ngb'][0] / 1e6, per_byte))
      tot['own'] += r['own'][0]
      tot['lib'] += r['lib'][0]
    del lay, ngb, own, lib, nown
    torch.cuda.empty_cache()
  say('sum of the 39 medians: own %.1f us, library %.1f us (ratio %.3f)' % (tot['own'], tot['lib'], tot['own'] / tot['lib']))


def section_pow2(args, say):
  import torch
  from pocketflow_amd import hip
  other = ctypes.CDLL(os.path.abspath(args.other_lib))
  this = hip._lib
  say('depthwise 3x3, MobileNet-v1 1.00 (shapes supported before), batch %d, bf16: this build against %s; %d rounds of %d calls, alternating'
      % (args.batch, args.other_lib, args.rounds, args.iters))
  say('%-16s %-5s | %9s %7s | %9s %7s | %10s %s' % ('H, C, stride', 'pass', 'this us', 'spread', 'other us', 'spread', 'difference', 'within the other build\'s spread'))
  worst = 0.0
  for H, C, stride in LAYERS:
    lay = DwLayer(args.batch, H, C, stride)
    a, b = lay.own(this), lay.own(other)
    for k in ('fwd', 'bwd', 'wrw'):
      r = alternate({'this': a[k], 'other': b[k]}, args.rounds, args.iters)
      diff = r['this'][0] - r['other'][0]
      worst = max(worst, diff / r['other'][0])
      say('%-16s %-5s | %9.1f %7.1f | %9.1f %7.1f | %+10.1f %s' % ('%d, %d, %d' % (H, C, stride), k, r['this'][0], r['this'][1],
                                                                  r['other'][0], r['other'][1], diff, 'yes' if diff <= r['other'][1] else 'NO'))
    del lay, a, b
    torch.cuda.empty_cache()
  say('largest (this - other) / other over the 39 rows: %+.2f %%' % (100.0 * worst))


def off4(t):
  """A copy of t placed 4 bytes behind a 16-byte boundary: the entries take their scalar loops for it."""
  import torch
  skip = 4 // t.element_size()
  buf = torch.empty(t.numel() + 16, dtype=t.dtype, device=t.device)
  v = buf[skip:skip + t.numel()].view(t.shape)
  v.copy_(t)
  assert t.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4
  return v


def section_bn(args, say):
  import torch
  from pocketflow_amd import graph, hip
  say('BatchNorm / quantiser passes, bf16, batch %d: vector route (aligned) against scalar route (input 4 bytes off alignment); '
      '%d rounds of %d calls, alternating' % (args.batch, args.rounds, args.iters))
  say('%-18s %-22s | %9s %7s %6s | %10s %8s | %s' % ('rows x C', 'entry', 'vector us', 'spread', 'TB/s', 'scalar us', 'spread', 'scalar / vector'))
  bf = torch.bfloat16
  for hw, C in BN_ROWS:
    assert hip.bn_vector_ok(C)
    rows = args.batch * hw * hw
    g = torch.Generator(device='cuda').manual_seed(rows + C)
    x = torch.randn(rows, C, device='cuda', generator=g).to(bf)
    dq = torch.randn(rows, C, device='cuda', generator=g).to(bf)
    xs = off4(x)
    out, codes = torch.empty(rows, C, device='cuda', dtype=bf), torch.empty(rows, C, device='cuda', dtype=torch.uint8)
    ss = torch.stack([0.5 + torch.rand(C, device='cuda', generator=g), torch.randn(C, device='cuda', generator=g)]).contiguous()
    mi = torch.stack([0.3 * torch.randn(C, device='cuda', generator=g), 0.5 + torch.rand(C, device='cuda', generator=g)]).contiguous()
    dgamma, dbeta = torch.randn(C, device='cuda', generator=g), torch.randn(C, device='cuda', generator=g)
    nb = graph._bn_blocks(rows, C)
    p4, p2 = torch.empty(nb, 4, C, device='cuda'), torch.empty(nb, 2, C, device='cuda')
    slot = torch.empty((1, 2), dtype=torch.int32, device='cuda')
    hip.minmax_slots_init(slot)
    hip.minmax_tensor(torch.tensor([0.0, 6.0], device='cuda'), slot[0], None)
    ab, pair = torch.tensor([6.0, 0.0], device='cuda'), torch.empty(2, device='cuda')
    E = rows * C * 2
    entries = [
        ('bn_stats', 1 * E, lambda xv: hip.bn_stats(xv, rows, C, p4, nb)),
        ('bn_act_quant_apply', 2 * E, lambda xv: hip.bn_act_quant_apply(xv, out, rows, C, ss, 'Relu6', slot[0], 8, True)),
        ('bn_bwd_stats', 2 * E, lambda xv: hip.bn_bwd_stats(dq, xv, rows, C, ss, mi, 'Relu6', p2, nb)),
        ('bn_bwd_apply', 3 * E, lambda xv: hip.bn_bwd_apply(dq, xv, out, rows, C, ss, mi, dgamma, dbeta, 'Relu6')),
        ('bn_act_quant_codes', E + E // 2, lambda xv: hip.bn_act_quant_codes(xv, codes, rows, C, ss, 'Relu6', slot[0], 8, pair)),
        ('bn_act_quant_static', E + E // 2, lambda xv: hip.bn_act_quant_static(xv, codes, rows, C, ss, 'Relu6', ab, 8))]
    # (pf_bn_act_quant_pool is not in the list: its vector form lost this comparison at 12544 x 768, 45.0 against 21.3 us, and was
    # withdrawn for these channel counts; profiles/odd_channel_layers.txt keeps the line)
    for name, nbytes, fn in entries:
      r = alternate({'vector': lambda: fn(x), 'scalar': lambda: fn(xs)}, args.rounds, args.iters)
      say('%-18s %-22s | %9.1f %7.1f %6.2f | %10.1f %8.1f | %8.2f%s' % (
          '%d x %d' % (rows, C), name, r['vector'][0], r['vector'][1], nbytes / r['vector'][0] / 1e6, r['scalar'][0], r['scalar'][1],
          r['scalar'][0] / r['vector'][0], '' if r['vector'][0] < r['scalar'][0] else '   VECTOR ROUTE DOES NOT WIN'))
    del x, dq, xs, out, codes
    torch.cuda.empty_cache()


def _model_flags(args, work):
  from pocketflow_amd.flags import FLAGS
  import pocketflow_amd.learners.learner_utils  # noqa: F401  (defines flags)
  import pocketflow_amd.learners.abstract_learner  # noqa: F401
  import pocketflow_amd.datasets.abstract_dataset  # noqa: F401
  import pocketflow_amd.learners.uniform_quantization.learner  # noqa: F401
  import pocketflow_amd.nets.mobilenet_at_ilsvrc12 as net
  for k, v in dict(save_path=os.path.join(work, 'models', 'model.ckpt'), save_path_eval=os.path.join(work, 'models_eval', 'model.ckpt'),
                   uql_save_quant_model_path=os.path.join(work, 'uql', 'model.ckpt'), synthetic_pool=2, nb_eval_batches_override=1,
                   batch_size=args.batch, batch_size_eval=args.batch, uql_weight_bits=8, uql_activation_bits=8, uql_use_buckets=False,
                   enbl_dst=False, compute_dtype='bfloat16', mobilenet_version=1, mobilenet_depth_mult=args.depth, nb_classes=1001,
                   image_size=224).items():
    setattr(FLAGS, k, v)
  return net.ModelHelper()


def section_artefact(args, say):
  from pocketflow_amd.flags import FLAGS
  mh = _model_flags(args, args.work)
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  from pocketflow_amd.learners.uniform_quantization.learner import UniformQuantLearner
  from pocketflow_amd.tools.conversion import export_quant_int8_model as E
  from pocketflow_amd.utils import checkpoint
  create_synthetic_checkpoint(mh)
  learner = UniformQuantLearner(None, mh)
  learner.restore_vars(checkpoint.latest_checkpoint(os.path.dirname(FLAGS.save_path)))
  summ = E.export_from_learner(learner, os.path.join(args.work, 'model_int8.npz'))
  say('artefact: %s (%d quantised tensors)' % (os.path.join(args.work, 'model_int8.npz'), summ['quantised_tensors']))


def section_model(args, say):
  """One JSON line: ms per batch of calc_inference_time on the artefact, ms per training step, of the package under --tree."""
  import torch
  from pocketflow_amd.tools.benchmark import calc_inference_time as T
  import io
  import contextlib
  buf = io.StringIO()
  with contextlib.redirect_stdout(buf):
    rc = T.main(['--net', 'mobilenet_at_ilsvrc12', '--mobilenet_depth_mult', str(args.depth), '--batch_size', str(args.batch),
                 '--compute_dtype', 'bfloat16', '--nb_classes', '1001', '--image_size', '224', '--nb_repts_warmup', '10', '--nb_repts', '30',
                 '--json', '--model_file', os.path.join(args.work, 'model_int8.npz')])
  assert rc == 0
  inf = json.loads([ln for ln in buf.getvalue().splitlines() if ln.startswith('{')][-1])
  mh = _model_flags(args, args.work)                     # the checkpoint of the `artefact` section
  from pocketflow_amd.learners.uniform_quantization.learner import UniformQuantLearner
  learner = UniformQuantLearner(None, mh)
  for _ in range(3):
    learner.train_step()
  torch.cuda.synchronize()
  steps = 10
  beg = time.perf_counter()
  for _ in range(steps):
    learner.train_step()
  torch.cuda.synchronize()
  ms = (time.perf_counter() - beg) / steps * 1e3
  say(json.dumps(dict(tree=args.tree, inference_ms_per_batch=inf['ms_per_batch'], nb_int8_layers=inf.get('nb_int8_layers'),
                      train_ms_per_step=ms, images_per_s=args.batch / ms * 1e3)))


def child(args, section, extra=(), tree=None):
  """Runs one section in a process of its own under its own time limit; returns its printed lines, raises if it fails."""
  cmd = [sys.executable, os.path.abspath(__file__), '--section', section, '--batch', str(args.batch), '--rounds', str(args.rounds),
         '--iters', str(args.iters), '--depth', str(args.depth), '--work', args.work, '--tree', tree or args.tree] + list(extra)
  r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=SECTION_TIMEOUT[section], cwd=tree or args.tree)
  if r.returncode != 0:
    sys.stderr.write(r.stdout + r.stderr)
    raise RuntimeError('section %s ended with status %d: nothing more is started' % (section, r.returncode))
  return [ln[2:] for ln in r.stdout.splitlines() if ln.startswith('| ')]


def driver(args):
  lines = []

  def run(section, extra=(), tree=None):
    got = child(args, section, extra, tree)
    for ln in got:
      print(ln, flush=True)
    lines.extend(got)
    return got
  run('depthwise')
  lines.append('')
  if args.parent_tree:
    run('pow2', ['--other_lib', os.path.join(args.parent_tree, 'pocketflow_amd', 'csrc', 'libpocketflow_hip.so')])
    lines.append('')
  run('bn')
  lines.append('')
  run('artefact')
  trees = ([('parent', os.path.abspath(args.parent_tree))] if args.parent_tree else []) + [('branch', args.tree)]
  res = {k: [] for k, _ in trees}
  for _ in range(args.model_rounds):
    for k, tree in trees:
      res[k].append(json.loads(run('model', tree=tree)[-1]))
  lines.append('')
  lines.append('whole model, MobileNet-v1 %.2f, batch %d, 224 x 224, bf16, %d alternating rounds (median; all rounds in brackets)'
               % (args.depth, args.batch, args.model_rounds))
  for k, _ in trees:
    for key, what in (('inference_ms_per_batch', 'calc_inference_time, ms per batch'), ('train_ms_per_step', 'training step (UQ w8/a8), ms')):
      v = [r[key] for r in res[k]]
      lines.append('%-7s %-36s %9.2f   [%s]' % (k, what, statistics.median(v), ', '.join('%.2f' % t for t in v)))
  print('\n'.join(lines[-1 - 2 * len(trees):]))
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write('\n'.join(lines) + '\n')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--section', default=None, choices=sorted(SECTION_TIMEOUT))
  ap.add_argument('--out', default=None)
  ap.add_argument('--tree', default=ROOT, help='the checkout whose pocketflow_amd package a section imports')
  ap.add_argument('--parent_tree', default=None, help='driver: a built checkout of the parent commit')
  ap.add_argument('--other_lib', default=None, help='pow2: another build of libpocketflow_hip.so')
  ap.add_argument('--work', default=os.path.join(tempfile.gettempdir(), 'pf_odd_channel_work'), help='checkpoint and artefact of the model sections')
  ap.add_argument('--depth', type=float, default=0.75)
  ap.add_argument('--batch', type=int, default=256)
  ap.add_argument('--iters', type=int, default=10)
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--model_rounds', type=int, default=3)
  args = ap.parse_args()
  args.tree, args.work = os.path.abspath(args.tree), os.path.abspath(args.work)
  if args.section is None:
    return driver(args)
  sys.path.insert(0, args.tree)
  import torch
  assert torch.cuda.is_available(), 'this measurement needs the GPU'
  say = lambda s: print('| ' + s, flush=True)
  globals()['section_' + args.section](args, say)


if __name__ == '__main__':
  main()
