"""The 'chn-pruned-rmt' learner without a GPU: the NumPy restatement (tests/cpr_oracle.py) against itself where the reference's
semantics pin a value, the host draw order, the flags, the factory, and the learner end to end on emulated entry points."""
import ast
import glob
import logging
import os

import numpy as np
import pytest
import torch

import cpr_oracle as O
from fake_hip import FakeHipFull

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'cpr')


def _fixture():
  import json
  return json.load(open(os.path.join(GOLDEN, 'reference_cpr.json'))), np.load(os.path.join(GOLDEN, 'reference_cpr.npz'))


class FakeHipCpr(FakeHipFull):
  """FakeHipFull + the pf_cpr entry points on CPU tensors (the oracle's arithmetic)."""

  def cpr_gather(self, x, y, pos, kh, kw, stride, pad_t, pad_l, P, Y, row0):
    self._n('cpr_gather')
    xn = x.permute(0, 2, 3, 1).float().numpy()
    yn = y.permute(0, 2, 3, 1).float().numpy()
    Pr, Yr = O.gather(xn, yn, [tuple(p) for p in pos.numpy()], kh, kw, stride, pad_t, pad_l)
    C, Co = xn.shape[3], yn.shape[3]
    P[row0 * kh * kw * C:(row0 + Pr.shape[0]) * kh * kw * C] = torch.from_numpy(Pr.reshape(-1))
    Y[row0 * Co:(row0 + Yr.shape[0]) * Co] = torch.from_numpy(Yr.reshape(-1))

  def cpr_gram_ws(self, C):
    return 1

  def cpr_gram(self, P, Y, idx, kk, C, Co, w_krsc, ws, xtx, xty):
    self._n('cpr_gram')
    w = w_krsc.view(Co, kk, C).numpy()
    k = int(round(kk ** 0.5))
    w_hwio = w.transpose(1, 2, 0).reshape(k, kk // k, C, Co)
    a, b, __ = O.gram(P.view(-1, kk, C).numpy(), Y.view(-1, Co).numpy(), idx.numpy(), w_hwio)
    xtx[:C * C] = torch.from_numpy(a.reshape(-1))
    xty[:C] = torch.from_numpy(b)

  def cpr_ista(self, A, b, m0, m_ws, mask, gamma, lr, iters, nnz):
    self._n('cpr_ista')
    C = b.numel()
    m = O.ista(A.view(C, C).numpy(), b.numpy(), m0.numpy(), gamma, lr, iters)
    mask.copy_(torch.from_numpy(m))
    nnz[0] = int(np.count_nonzero(m))

  def cpr_lstsq_splits(self, N, Kp, Co):
    return 1

  def cpr_lstsq_resid(self, P, kidx, W, Y, R, N, Co):
    K = W.numel() // Co
    X = P.view(-1, K)[:N][:, kidx.long()]
    R[:N * Co] = ((X @ W.view(K, Co)[kidx.long()]) - Y.view(-1, Co)[:N]).reshape(-1)

  def cpr_lstsq_step(self, P, kidx, pos, Y, R, W, m, v, part, N, Co, wd, lr_t, beta1, beta2, c1, c2, eps):
    self._n('cpr_lstsq_step')
    f = np.float32
    K = W.numel() // Co
    self.cpr_lstsq_resid(P, kidx, W, Y, R, N, Co)
    X = P.view(-1, K)[:N][:, kidx.long()]
    G = torch.zeros(K, Co)
    G[kidx.long()] = X.t() @ R[:N * Co].view(N, Co)
    W, m, v = W.view(-1), m.view(-1), v.view(-1)
    g = G.view(-1) / f(N)
    g = g + f(wd) * W
    m.copy_(f(beta1) * m + f(c1) * g)
    v.copy_(f(beta2) * v + f(c2) * (g * g))
    W.copy_(W + (-f(lr_t) * m) / (torch.sqrt(v) + f(eps)))


@pytest.fixture
def cpr_cpu(monkeypatch, tmp_path):
  import pocketflow_amd.graph as G
  import pocketflow_amd.plan as P
  import pocketflow_amd.losses as L
  import pocketflow_amd.optim as Opt
  import pocketflow_amd.learners.abstract_learner as AL
  import pocketflow_amd.learners.weight_sparsification.learner as WS
  import pocketflow_amd.learners.layerwise as LW
  import pocketflow_amd.learners.learner_utils  # noqa: F401
  import pocketflow_amd.learners.distillation_helper  # noqa: F401
  import pocketflow_amd.nets.resnet_at_cifar10  # noqa: F401
  import pocketflow_amd.learners.channel_pruning_rmt.learner as CPR
  from pocketflow_amd.flags import FLAGS
  fake = FakeHipCpr()
  for mod in (G, P, L, Opt, WS, LW, CPR):
    monkeypatch.setattr(mod, 'hip', fake)
  monkeypatch.setattr(AL, 'require_gpu', lambda: torch.device('cpu'))
  monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
  FLAGS.save_path = str(tmp_path / 'models' / 'model.ckpt')
  FLAGS.save_path_eval = str(tmp_path / 'models_eval' / 'model.ckpt')
  FLAGS.enbl_dst, FLAGS.nb_eval_batches_override, FLAGS.synthetic_pool, FLAGS.compute_dtype = False, 2, 2, 'float32'
  FLAGS.learner = 'chn-pruned-rmt'
  FLAGS.cpr_save_path = str(tmp_path / 'cpr' / 'model.ckpt')
  FLAGS.cpr_save_path_eval = str(tmp_path / 'cpr_eval' / 'model.ckpt')
  FLAGS.cpr_save_path_ws = str(tmp_path / 'cpr_ws' / 'model.ckpt')
  FLAGS.cpr_prune_ratio, FLAGS.cpr_skip_frst_layer, FLAGS.cpr_skip_last_layer, FLAGS.cpr_skip_op_names = 0.5, True, False, None
  FLAGS.cpr_nb_smpls, FLAGS.cpr_nb_crops_per_smpl = 16, 2
  FLAGS.cpr_ista_lrn_rate, FLAGS.cpr_ista_nb_iters, FLAGS.cpr_lstsq_lrn_rate, FLAGS.cpr_lstsq_nb_iters = 1e-2, 100, 1e-3, 5
  FLAGS.cpr_warm_start = False
  FLAGS.batch_size, FLAGS.batch_size_eval, FLAGS.nb_classes, FLAGS.resnet_size = 8, 8, 10, 8
  FLAGS.nb_iters_override, FLAGS.summ_step = 3, 2
  return FLAGS, fake, tmp_path


def test_cpr_flags_have_the_reference_names_and_defaults():
  """Names and defaults as the fixture read them from the reference's text."""
  import pocketflow_amd.learners.channel_pruning_rmt.learner  # noqa: F401
  from pocketflow_amd.flags import FLAGS
  meta, __ = _fixture()
  FLAGS.reset()
  ours = FLAGS.flag_values_dict()
  assert len(meta['flags']) == 14
  for name, d in meta['flags'].items():
    assert name in ours and ours[name] == d['default'], (name, ours.get(name), d)


def test_create_learner_knows_chn_pruned_rmt_and_still_refuses_the_others(cpr_cpu):
  FLAGS, fake, tmp = cpr_cpu
  from pocketflow_amd.learners.learner_utils import create_learner
  for name in ('dis-chn-pruned', 'uniform-tf'):
    FLAGS.learner = name
    with pytest.raises(ValueError):
      create_learner(None, None)
  src = open(os.path.join(ROOT, 'pocketflow_amd', 'learners', 'learner_utils.py')).read()
  assert 'ChannelPrunedRmtLearner' in src


def _case_inputs(case, z):
  """The fixture's tapped tensors as this package holds them: a fixed-pad convolution's tap is the UNPADDED tensor."""
  p, fp = case['name'] + '/', case['fixed_pad']
  x = z[p + 'x_prnd']
  if fp:
    x = x[:, :, fp:-fp, fp:-fp, :]
  return x, z[p + 'y_full']


def _pads(case, H, W):
  if case['fixed_pad']:
    return case['fixed_pad'], case['fixed_pad']
  if case['padding'] == 'VALID':
    return 0, 0
  return O.same_pad(H, case['k'], case['stride']), O.same_pad(W, case['k'], case['stride'])


def test_learner_draws_and_oracle_sampling_reproduce_the_fixture():
  """The learner's draw helpers, called in its loop order from the fixture's seed, give the reference's positions, row choices and
  initial mask; the oracle's gather of the unpadded taps gives the reference's P / Y bit for bit."""
  from pocketflow_amd.learners.channel_pruning_rmt.learner import draw_positions, draw_selection
  meta, z = _fixture()
  crops, nb_min = meta['crops'], meta['crops'] * meta['nb_smpls']
  for case in meta['cases']:
    p = case['name'] + '/'
    x, y = _case_inputs(case, z)
    np.random.seed(case['seed'])
    Ps, Ys, positions, nb_insts = [], [], [], 0
    for mb in range(case['nb_mbtcs_used']):
      pos = draw_positions(y.shape[2], y.shape[3], crops)
      positions.append(pos)
      pt, pl = _pads(case, x.shape[2], x.shape[3])
      P, Y = O.gather(x[mb], y[mb], [tuple(q) for q in pos], case['k'], case['k'], case['stride'], pt, pl)
      Ps.append(P)
      Ys.append(Y)
      nb_insts += P.shape[0]
    idxs_inst, idxs_rdc, mask_init = draw_selection(nb_insts, nb_min, case['Co'], case['C'])
    assert np.array_equal(np.concatenate(positions), z[p + 'positions']), case['name']
    assert np.array_equal(idxs_inst, z[p + 'idxs_inst']) and np.array_equal(idxs_rdc, z[p + 'idxs_rdc'])
    assert np.array_equal(mask_init, z[p + 'mask_init'])
    assert np.array_equal(np.concatenate(Ps)[idxs_inst], z[p + 'P']), case['name']
    assert np.array_equal(np.concatenate(Ys)[idxs_inst], z[p + 'Y']), case['name']


def test_oracle_gram_gamma_path_and_lstsq_reproduce_the_fixture():
  """float32 X^T X / X^T y bit for bit; the (gamma, nnz) path and the final mask identical; the least-squares kernel and losses
  within the bar (float32 statements, identical here; the float64 run of the same statements is ~1e-6 away)."""
  meta, z = _fixture()
  for case in meta['cases']:
    p = case['name'] + '/'
    a, b, __ = O.gram(z[p + 'P'], z[p + 'Y'], z[p + 'idxs_rdc'], z[p + 'w'])
    assert np.array_equal(a, z[p + 'xtx']) and np.array_equal(b, z[p + 'xty']), case['name']
    mask, path = O.bisect(lambda g: (lambda m: (m, int(np.count_nonzero(m))))(O.ista(a, b, z[p + 'mask_init'], g, 1e-2, 100)),
                          case['target'])
    assert [list(q) for q in path] == case['path'], case['name']
    assert np.array_equal(mask, z[p + 'mask']) and path[-1][1] == case['target']
    w, before, after = O.lstsq(z[p + 'P'], z[p + 'Y'], z[p + 'w'], mask != 0, 100, 1e-3, meta['loss_w_dcy'])
    assert np.max(np.abs(w - z[p + 'kernel'])) <= 1e-5, case['name']
    for got, want in zip(before + after, case['losses'][0] + case['losses'][1]):
      assert abs(got - want) <= 1e-5 * abs(want), (case['name'], got, want)


def test_cpr_learner_end_to_end_on_cpu(cpr_cpu, caplog):
  FLAGS, fake, tmp = cpr_cpu
  from pocketflow_amd.nets.resnet_at_cifar10 import ModelHelper
  from pocketflow_amd.learners.learner_utils import create_learner, create_synthetic_checkpoint
  from pocketflow_amd.learners.channel_pruning_rmt.learner import ChannelPrunedRmtLearner
  from pocketflow_amd.utils import checkpoint
  mh = ModelHelper()
  create_synthetic_checkpoint(mh)
  full_before = checkpoint.load(checkpoint.latest_checkpoint(os.path.dirname(FLAGS.save_path)))
  np.random.seed(3)
  lrn = create_learner(None, mh)
  assert isinstance(lrn, ChannelPrunedRmtLearner)
  draws = []
  saved = {name: getattr(np.random, name) for name in ('randint', 'choice', 'uniform')}
  for name, fn in saved.items():
    def rec(*a, __f=fn, __n=name, **k):
      draws.append(__n)
      return __f(*a, **k)
    setattr(np.random, name, rec)
  try:
    with caplog.at_level(logging.INFO, logger='pocketflow_amd'):
      rslt = lrn.train()
  finally:
    for name, fn in saved.items():
      setattr(np.random, name, fn)
  # the reference's draw order per layer: (oh, ow) per crop for every sampled mini-batch, choice, choice, uniform
  nb_mbtcs_used = 2 * 16 // 8 // 2 + 1                   # rows grow by crops * batch = 16 per mini-batch until they exceed 2 * 16
  per_layer = ['randint'] * (2 * 2 * min(nb_mbtcs_used, 2)) + ['choice', 'choice', 'uniform']
  assert draws[:len(per_layer) * len(lrn.vars_prnd['maskable'])] == per_layer * len(lrn.vars_prnd['maskable'])
  assert np.isfinite(rslt['loss']) and 0.0 < rslt['pr_krn'] < 0.6
  n = len(lrn.vars_prnd['maskable'])
  assert len(lrn.selection_log) == n and fake.calls['cpr_gather'] >= 2 * n and fake.calls['cpr_gram'] == n
  msgs = [r.getMessage() for r in caplog.records]
  for idx, rec in enumerate(lrn.selection_log):
    cin = lrn.vars_prnd['maskable'][idx].ref_shape[2]
    assert rec['target'] == int(cin * (1.0 - (0.0 if idx == 0 else 0.5)))
    assert rec['nnz'] == rec['target'] or any('search exhausted' in m for m in msgs)
    assert rec['path'][0][0] == 0.1
  # pruned input channels are zero after selection and stay zero through the fine-tune; masks agree
  ws = checkpoint.load(checkpoint.latest_checkpoint(str(tmp / 'cpr_ws')))
  vals = lrn.graph.store.export_numpy()
  for idx, var in enumerate(lrn.vars_prnd['maskable']):
    dead_ws = np.all(ws[var.name] == 0, axis=(0, 1, 3))
    dead = np.all(vals[var.name] == 0, axis=(0, 1, 3))
    assert dead_ws.sum() == var.ref_shape[2] - lrn.selection_log[idx]['nnz']
    assert np.array_equal(dead & dead_ws, dead_ws)
    m = var.to_ref(lrn.masks[var.offset:var.offset + var.numel].numpy())
    assert np.array_equal(np.all(m == 0, axis=(0, 1, 3)), dead_ws)
  # selection moves no BN moving statistic: the warm-start checkpoint holds the pre-trained ones
  stats = [k for k in full_before if 'moving_' in k]
  assert stats
  for k in stats:
    assert np.array_equal(ws['pruned_' + k] if 'pruned_' + k in ws else ws[k.replace('model/', 'pruned_model/', 1)], full_before[k]), k
  # the full network's checkpoint is untouched
  full_after = checkpoint.load(checkpoint.latest_checkpoint(os.path.dirname(FLAGS.save_path)))
  for k, v in full_before.items():
    assert np.array_equal(v, full_after[k]), k
  assert any(m.startswith('iter #2:') and 'pr_krn' in m for m in msgs)
  # warm start skips selection
  FLAGS.cpr_warm_start = True
  calls = dict(fake.calls)
  lrn2 = create_learner(None, mh)
  lrn2.train()
  assert fake.calls.get('cpr_gram') == calls.get('cpr_gram') and lrn2.selection_log == []


def test_no_cpr_file_reads_the_reference_tree():
  """The files of this learner run where the reference tree does not exist: none of them names it in code."""
  added = (glob.glob(os.path.join(ROOT, 'tests', '*cpr*.py')) + glob.glob(os.path.join(ROOT, 'pocketflow_amd', 'learners', 'channel_pruning_rmt', '*.py'))
           + glob.glob(os.path.join(ROOT, 'tools', 'gpu', 'cpr_*.py')))
  assert len(added) >= 5
  needle = os.path.join(os.sep + 'root', 'reference')
  for path in added:
    for node in ast.walk(ast.parse(open(path).read())):
      if isinstance(node, ast.Constant) and isinstance(node.value, str):
        assert needle not in node.value, os.path.relpath(path, ROOT)
