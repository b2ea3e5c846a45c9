#!/usr/bin/env python
"""Reference-executed fixture for the 'chn-pruned-rmt' channel selection.

Runs HERE (needs the reference tree); the GPU box only reads the committed output (reference_cpr.npz / .json).

Four methods of ChannelPrunedRmtLearner (learners/channel_pruning_rmt/learner.py) are lifted with `ast` as they are written
(make_reference_golden.lift, no source copied): `__smpl_inputs_n_outputs`, `__build_meta_lasso`, `__build_meta_lstsq` and
`__solve_sparse_regression`.  The two meta problems are TF graph code whose train ops depend on `tf.control_dependencies`
(the Adam step reads the moments it has just assigned), which the snapshot rule of oracle/tf_graph_stub.py does not model;
they run over the small deferred-execution shim below instead: nodes evaluated in dependency order, control dependencies
first, variables read when the node runs, every op rounded to float32 as TF's float32 kernels do (matmul via NumPy float32).

Per case, the generator seeds np.random, runs the reference's per-layer loop (:580-631: the mini-batch loop around
__smpl_inputs_n_outputs with its break, then np.random.choice) and __solve_sparse_regression, and records the draws, P / Y,
the float32 X^T X / X^T y / initial mask fed to the LASSO, every (gamma, nnz) of the search, the final mask, the least-squares
losses and the written-back kernel.  It also records the reference's cpr_* flag defaults, read from the file's text.

What it does not pin: TensorFlow's own kernels (summation order of matmul) -- the same caveat as every other fixture here.
Deterministic: a re-run rewrites identical files."""
import ast
import contextlib
import json
import math
import os
import sys
from timeit import default_timer as timer

import numpy as np
from scipy.linalg import norm

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
ROOT = os.path.dirname(os.path.dirname(GOLDEN))
sys.path.insert(0, ROOT)
sys.path.insert(0, GOLDEN)

import make_reference_golden as G  # noqa: E402

PATH = 'learners/channel_pruning_rmt/learner.py'
CLS = 'ChannelPrunedRmtLearner'
METHODS = ['__smpl_inputs_n_outputs', '__build_meta_lasso', '__build_meta_lstsq', '__solve_sparse_regression']
F32 = np.float32


# ---- deferred-execution shim for the two meta problems --------------------------------------------------------------------
class _Ctx(object):
  deps = []


def _f32(v):
  return np.asarray(v, dtype=F32)


class Node(object):
  def __init__(self, fn, inputs=()):
    self.fn, self.deps = fn, list(_Ctx.deps)
    self.inputs = [_node(i) for i in inputs]          # constants become nodes once: the memo is keyed by node identity

  def ev(self, run):
    if id(self) in run.memo:
      return run.memo[id(self)]
    for d in self.deps:
      d.ev(run)
    v = self.fn(*[i.ev(run) for i in self.inputs])
    run.memo[id(self)] = v
    return v

  def __add__(self, o): return Node(lambda a, b: _f32(a + b), [self, o])
  def __radd__(self, o): return Node(lambda a, b: _f32(a + b), [o, self])
  def __sub__(self, o): return Node(lambda a, b: _f32(a - b), [self, o])
  def __rsub__(self, o): return Node(lambda a, b: _f32(a - b), [o, self])
  def __mul__(self, o): return Node(lambda a, b: _f32(a * b), [self, o])
  def __rmul__(self, o): return Node(lambda a, b: _f32(a * b), [o, self])
  def __truediv__(self, o): return Node(lambda a, b: _f32(a / b), [self, o])
  def __pow__(self, o): return Node(lambda a, b: _f32(np.power(a, b)), [self, o])
  def __neg__(self): return Node(lambda a: _f32(-a), [self])
  def __gt__(self, o): return Node(lambda a, b: a > b, [self, o])
  def __lt__(self, o): return Node(lambda a, b: a < b, [self, o])
  def __getitem__(self, i): return Node(lambda a: a[i], [self])


class Const(Node):
  def __init__(self, v):
    super(Const, self).__init__(lambda: v)
    self.deps = []


def _node(x):
  if isinstance(x, Node):
    return x
  if isinstance(x, (float, int, np.floating)):
    return Const(F32(x))
  return Const(np.asarray(x))


class Placeholder(Node):
  def __init__(self):
    super(Placeholder, self).__init__(None)
    self.deps = []

  def ev(self, run):
    return _f32(run.feed[self])


class Variable(Node):
  def __init__(self, init):
    super(Variable, self).__init__(None)
    self.deps, self.init, self.value = [], init, None

  def ev(self, run):                      # a read: the value when the reading node runs
    return self.value

  def assign(self, v):
    def f(x):
      self.value = _f32(x)
      return self.value
    return Node(f, [v])

  def assign_add(self, v):
    return self.assign(Node(lambda a: a, [v]) + self)


class Run(object):
  def __init__(self, feed):
    self.feed, self.memo = feed or {}, {}


class Session(object):
  def run(self, fetches, feed_dict=None):
    r = Run(feed_dict)
    if isinstance(fetches, (list, tuple)):
      return [_node(f).ev(r) for f in fetches]
    return _node(fetches).ev(r)


class _Logging(object):
  messages = []

  def info(self, msg):
    self.messages.append(msg)


class _NN(object):
  @staticmethod
  def l2_loss(x):
    return Node(lambda a: _f32(np.sum(_f32(a * a), dtype=F32) / F32(2)), [x])


class ShimTF(object):
  float32 = 'float32'
  logging = _Logging()
  nn = _NN()

  @staticmethod
  @contextlib.contextmanager
  def variable_scope(name):
    yield

  @staticmethod
  @contextlib.contextmanager
  def control_dependencies(ops):
    saved = _Ctx.deps
    _Ctx.deps = saved + list(ops)
    try:
      yield
    finally:
      _Ctx.deps = saved

  @staticmethod
  def placeholder(dtype, shape=None, name=None):
    return Placeholder()

  @staticmethod
  def zeros_initializer():
    return None

  @staticmethod
  def get_variable(name, shape=None, initializer=None, trainable=True, validate_shape=True):
    if initializer is ShimTF.zeros_initializer:
      return Variable(Const(F32(0)))
    return Variable(initializer)

  @staticmethod
  def variables_initializer(var_list):
    def f(*vals):
      for v, x in zip(var_list, vals):
        v.value = _f32(x)
      return None
    return Node(f, [v.init for v in var_list])

  @staticmethod
  def where(c, x, y):
    return Node(lambda a, b, d: _f32(np.where(a, b, d)), [c, x, y])

  @staticmethod
  def zeros_like(x):
    return Node(lambda a: np.zeros_like(a), [x])

  @staticmethod
  def matmul(a, b):
    return Node(lambda p, q: _f32(np.matmul(p, q)), [a, b])

  @staticmethod
  def transpose(a):
    return Node(lambda p: np.ascontiguousarray(p.T), [a])

  @staticmethod
  def shape(a):
    return Node(lambda p: np.array(p.shape, np.int32), [a])

  @staticmethod
  def cast(a, dtype):
    return Node(lambda p: _f32(p), [a])

  @staticmethod
  def sqrt(a):
    return Node(lambda p: _f32(np.sqrt(p)), [a])

  @staticmethod
  def pow(a, b):
    return Node(lambda p, q: _f32(np.power(p, q)), [a, b])

  @staticmethod
  def ones(shape):
    return Const(np.ones(shape, F32))


# ---- cases --------------------------------------------------------------------------------------------------------------
# (name, B, H, W, C, Co, k, stride, padding as the reference sees it, fixed pad applied before, prune ratio)
CASES = [
    ('1x1', 4, 6, 6, 12, 16, 1, 1, 'SAME', 0, 0.5),
    ('3x3_same', 4, 7, 6, 8, 12, 3, 1, 'SAME', 0, 0.5),
    ('3x3_s2_fixed_pad', 4, 8, 8, 8, 16, 3, 2, 'VALID', 1, 0.5),
    ('3x3_s2_same_odd', 4, 9, 9, 8, 12, 3, 2, 'SAME', 0, 0.5),
    ('3x3_s2_same_even', 4, 10, 10, 8, 12, 3, 2, 'SAME', 0, 0.5),
    ('7x7_stem', 4, 16, 16, 3, 16, 7, 2, 'SAME', 0, 0.5),
    ('ratio0', 4, 6, 6, 10, 8, 3, 1, 'SAME', 0, 0.0),
]
NB_SMPLS, CROPS, LOSS_W_DCY = 6, 3, 2e-4


def conv_nhwc(x, w, stride, padding):
  """Exact-enough float64 convolution (TF 'SAME' / 'VALID') that makes the reference's reconstruction asserts hold."""
  B, H, W, C = x.shape
  kh, kw, __, Co = w.shape
  if padding == 'SAME':
    OH, OW = -(-H // stride), -(-W // stride)
    ph = max((OH - 1) * stride + kh - H, 0)
    pw = max((OW - 1) * stride + kw - W, 0)
    xp = np.pad(x.astype(np.float64), ((0, 0), (ph // 2, ph - ph // 2), (pw // 2, pw - pw // 2), (0, 0)))
  else:
    OH, OW = (H - kh) // stride + 1, (W - kw) // stride + 1
    xp = x.astype(np.float64)
  y = np.zeros((B, OH, OW, Co))
  for i in range(kh):
    for j in range(kw):
      y += xp[:, i:i + stride * OH:stride, j:j + stride * OW:stride, :] @ w[i, j].astype(np.float64)
  return y.astype(np.float32)


def reference_flags():
  tree = ast.parse(open(os.path.join(G.REF, PATH)).read())
  out = {}
  for node in ast.walk(tree):
    if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr.startswith('DEFINE_'):
      name = ast.literal_eval(node.args[0])
      if name.startswith('cpr_'):
        out[name] = {'kind': node.func.attr[len('DEFINE_'):], 'default': ast.literal_eval(node.args[1])}
  return out


def main():
  flags = reference_flags()
  FL = type('Flags', (), {k: v['default'] for k, v in flags.items()})()
  FL.cpr_nb_smpls, FL.cpr_nb_crops_per_smpl, FL.loss_w_dcy, FL.batch_size = NB_SMPLS, CROPS, LOSS_W_DCY, 4
  tf = ShimTF()
  ns = G.lift(PATH, ['%s.%s' % (CLS, m) for m in METHODS],
              {'tf': tf, 'FLAGS': FL, 'norm': norm, 'math': math, 'timer': timer})
  cls = ns[CLS]
  self = cls.__new__(cls)
  self.sess_prune = Session()
  self.meta_lasso = getattr(self, '_%s__build_meta_lasso' % CLS)()
  self.meta_lstsq = getattr(self, '_%s__build_meta_lstsq' % CLS)()
  smpl = getattr(self, '_%s__smpl_inputs_n_outputs' % CLS)
  solve = getattr(self, '_%s__solve_sparse_regression' % CLS)

  arrays, meta = {}, {'flags': flags, 'nb_smpls': NB_SMPLS, 'crops': CROPS, 'loss_w_dcy': LOSS_W_DCY, 'cases': []}
  real = {n: getattr(np.random, n) for n in ('randint', 'choice', 'uniform')}
  for ci, (name, B, H, W, C, Co, k, stride, padding, fixed_pad, ratio) in enumerate(CASES):
    rng = np.random.RandomState(100 + ci)
    w = (rng.randn(k, k, C, Co) * 0.2).astype(np.float32)
    nb_mbtcs = int(math.ceil(NB_SMPLS / FL.batch_size))
    xs_full, xs_prnd = [], []
    for __ in range(nb_mbtcs):
      xf = rng.randn(B, H, W, C).astype(np.float32)
      xp = (xf * (rng.rand(1, 1, 1, C) > 0.3) + 0.1 * rng.randn(B, H, W, C)).astype(np.float32)
      if fixed_pad:
        xf = np.pad(xf, ((0, 0), (fixed_pad, fixed_pad), (fixed_pad, fixed_pad), (0, 0)))
        xp = np.pad(xp, ((0, 0), (fixed_pad, fixed_pad), (fixed_pad, fixed_pad), (0, 0)))
      xs_full.append(xf)
      xs_prnd.append(xp)
    draws = []

    def rec(n):
      def f(*a, **kw):
        v = real[n](*a, **kw)
        draws.append((n, a, kw, v))
        return v
      return f
    for n in real:
      setattr(np.random, n, rec(n))
    tf.logging.messages = []
    np.random.seed(1000 + ci)
    try:
      # the per-layer loop of __choose_channels (:580-607) around the lifted sampler
      nb_insts, nb_insts_min = 0, CROPS * NB_SMPLS
      inputs_list, outputs_list = [[] for __ in range(C)], []
      ys_full = []
      for idx_mbtc in range(nb_mbtcs):
        yf = conv_nhwc(xs_full[idx_mbtc], w, stride, padding)
        yp = conv_nhwc(xs_prnd[idx_mbtc], w, stride, padding)
        ys_full.append(yf)
        ins, outs = smpl(w, w, xs_full[idx_mbtc], xs_prnd[idx_mbtc], yf, yp, [1, stride, stride, 1], padding)
        nb_insts += outs.shape[0]
        for c in range(C):
          inputs_list[c] += [ins[c]]
        outputs_list += [outs]
        if nb_insts > nb_insts_min:
          break
      idxs_inst = np.random.choice(nb_insts, size=(nb_insts_min), replace=False)
      inputs_np_list = [np.vstack(x)[idxs_inst] for x in inputs_list]
      outputs_np = np.vstack(outputs_list)[idxs_inst]
      feeds = []
      orig_run = self.sess_prune.run

      def run(fetches, feed_dict=None):
        if feed_dict:
          feeds.append({id(k): np.asarray(v) for k, v in feed_dict.items()})
        return orig_run(fetches, feed_dict)
      self.sess_prune.run = run
      krnl = solve(inputs_np_list, outputs_np, w, ratio)
      del self.sess_prune.run
    finally:
      for n, f in real.items():
        setattr(np.random, n, f)
    ml = self.meta_lasso
    lasso_init = [f for f in feeds if id(ml['xt_x_ph']) in f]
    gammas = [float(f[id(ml['gamma'])]) for f in feeds if id(ml['gamma']) in f]
    nnzs = [int(m.split('= ')[-1]) for m in tf.logging.messages if 'nb_chns_nnz' in m]
    gammas = gammas[::FL.cpr_ista_nb_iters]
    assert len(gammas) == len(nnzs) == len(lasso_init)
    losses = [[float(x) for x in m.split('losses: ')[1].replace(' (reg) / ', ' ').replace(' (dcy)', '').split()]
              for m in tf.logging.messages if m.startswith('losses: ')]
    positions = np.array([v for n, a, kw, v in draws if n == 'randint'], np.int64).reshape(-1, 2)
    choices = [v for n, a, kw, v in draws if n == 'choice']
    uniform = [v for n, a, kw, v in draws if n == 'uniform']
    assert [n for n, __, __, __ in draws] == ['randint'] * positions.size + ['choice', 'choice', 'uniform']
    p = name + '/'
    P = np.stack([x.reshape(-1, k * k) for x in inputs_np_list], -1).astype(np.float32)
    assert np.array_equal(P.astype(np.float64), np.stack(inputs_np_list, -1))
    arrays.update({p + 'w': w, p + 'x_full': np.stack(xs_full[:len(outputs_list)]), p + 'x_prnd': np.stack(xs_prnd[:len(outputs_list)]),
                   p + 'y_full': np.stack(ys_full), p + 'positions': positions, p + 'idxs_inst': idxs_inst,
                   p + 'idxs_rdc': choices[1], p + 'mask_init': uniform[0], p + 'P': P, p + 'Y': outputs_np.astype(np.float32),
                   p + 'xtx': lasso_init[0][id(ml['xt_x_ph'])].astype(np.float32),
                   p + 'xty': lasso_init[0][id(ml['xt_y_ph'])].astype(np.float32).reshape(-1),
                   p + 'mask': ml['mask'].value.reshape(-1), p + 'kernel': np.asarray(krnl, np.float32)})
    meta['cases'].append({'name': name, 'B': B, 'H': H, 'W': W, 'C': C, 'Co': Co, 'k': k, 'stride': stride, 'padding': padding,
                          'fixed_pad': fixed_pad, 'ratio': ratio, 'seed': 1000 + ci, 'nb_mbtcs_used': len(outputs_list),
                          'path': [[g, n] for g, n in zip(gammas, nnzs)], 'losses': losses,
                          'target': int(C * (1.0 - ratio))})
  np.savez_compressed(os.path.join(HERE, 'reference_cpr.npz'), **arrays)
  with open(os.path.join(HERE, 'reference_cpr.json'), 'w') as f:
    json.dump(meta, f, indent=1, sort_keys=True)
    f.write('\n')
  print('wrote %d arrays, %d cases' % (len(arrays), len(meta['cases'])))


if __name__ == '__main__':
  main()
