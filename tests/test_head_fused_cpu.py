"""The plumbing of the fused network head (PF_HEAD_FUSE: graph._BnActPool, BatchNormAct.pooled, losses._HeadCE and the hand-over on
the logits tensor) checked on the CPU: tests/fake_hip.py is a double of `hip` WITHOUT the new entry points -- with it the separate
chain must be taken -- and the subclasses below add float32 emulations of them, with which a small bottleneck ResNet and a learner
step are run with the switch off and on.  Both must give the same outputs, gradients and BN state to float32 round-off."""
import numpy as np
import pytest
import torch

from fake_hip import FakeHip, FakeHipFull, _rows, _mask  # noqa: E402  (tests/fake_hip.py)
from oracle import pf_oracle as O


class _HeadBn(object):
  """float32 emulations of pf_bn_act_quant_pool / pf_bn_bwd_stats_pooled / pf_bn_bwd_apply_pooled (include/pocketflow_hip.h)."""

  def bn_act_quant_pool(self, x, pooled, rows, C, hw, ss, act, slot, bits, quantize):
    self._n('bn_pool')
    q = self._q_of(_rows(x, C).float(), ss, act, slot, bits, quantize)
    pooled.copy_(q.view(-1, hw, C).sum(dim=1) / float(hw))

  @staticmethod
  def _expand(g, rows, C, hw):
    return (g.float() / float(hw)).view(-1, 1, C).expand(-1, hw, C).reshape(rows, C)

  def bn_bwd_stats_pooled(self, g, x, rows, C, hw, ss, mi, act, partial, nblk):
    self._n('bn_bwd_stats_pooled')
    xr, dq = _rows(x, C).float(), self._expand(g, rows, C, hw)
    dy = dq * _mask(xr * ss[0] + ss[1], act)
    p = partial[:nblk * 2 * C].view(nblk, 2, C)
    p.zero_()
    p[0, 0], p[0, 1] = dy.sum(0), (dy * (xr - mi[0]) * mi[1]).sum(0)

  def bn_bwd_apply_pooled(self, g, x, dx, rows, C, hw, ss, mi, dgamma, dbeta, act):
    self._n('bn_bwd_apply_pooled')
    xr, dq = _rows(x, C).float(), self._expand(g, rows, C, hw)
    dy = dq * _mask(xr * ss[0] + ss[1], act)
    _rows(dx, C).copy_(ss[0] * (dy - dbeta / rows - (xr - mi[0]) * mi[1] * dgamma / rows))


class HeadFakeHip(_HeadBn, FakeHip):
  pass


class HeadFakeHipFull(_HeadBn, FakeHipFull):
  """... plus pf_ce_distill_head / pf_ce_combine on the oracle's losses."""

  def ce_distill_fwd_bwd(self, *a):
    self._n('ce_plain')
    return FakeHipFull.ce_distill_fwd_bwd(self, *a)

  def ce_distill_head(self, z_s, labels, z_t, tempr, loss_w, losses, dz_hard, dz_soft, row_ws):
    self._n('ce_head')
    zs = z_s.detach().float().numpy()
    ce, dz = O.softmax_cross_entropy(labels.detach().numpy(), zs)
    losses[0], losses[1] = float(ce), 0.0
    dz_hard.copy_(torch.from_numpy(np.asarray(dz, np.float32)).to(dz_hard.dtype))
    if z_t is not None:
      dl, ddz = O.distill_loss(zs, z_t.detach().float().numpy(), tempr, loss_w)
      losses[1] = float(dl)
      dz_soft.copy_(torch.from_numpy(np.asarray(ddz, np.float32)).to(dz_soft.dtype))
    o = z_s.detach().float()
    rank = (o > o.gather(1, labels.argmax(dim=1, keepdim=True))).sum(dim=1)
    losses[2], losses[3] = (rank < 1).float().mean(), (rank < 5).float().mean()

  def ce_combine(self, dz_hard, dz_soft, g0, g1, dz):
    self._n('ce_combine')
    out = torch.zeros_like(dz_hard)
    if g0 is not None:
      out = out + dz_hard * g0.to(dz_hard.dtype)
    if dz_soft is not None and g1 is not None:
      out = out + dz_soft * g1.to(dz_hard.dtype)
    dz.copy_(out)


def _build(act_bits, filters=8):
  from pocketflow_amd import graph as G
  from pocketflow_amd.utils.external import resnet_model as R
  g = G.Graph('model', 'cpu', torch.float32)
  g.fuse_conv1x1 = True
  net = R.Model(50, True, 7, filters, 3, 1, None, None, [2, 2], [1, 2], data_format='channels_last', graph=g)
  g.finalize(seed=3, requires_grad=True)
  for op in g.activation_ops:
    op.bits = act_bits
  return g, net


def _run_net(monkeypatch, fake, fuse, act_bits, mode):
  """One forward (+ backward) of the small bottleneck ResNet; mode: 'train' | 'eval' (no gradients) | 'eval_grad'."""
  from pocketflow_amd import graph as G
  monkeypatch.setattr(G, 'hip', fake)
  monkeypatch.setattr(G, 'fusable_tensor', lambda t: True)
  monkeypatch.setattr(G, 'HEAD_FUSE', fuse)
  monkeypatch.setattr(G, 'HEAD_FUSE_ANY_DEVICE', True)
  g, net = _build(act_bits)
  torch.manual_seed(0)
  x = torch.randn(4, 3, 12, 12).contiguous(memory_format=torch.channels_last)
  wts = torch.randn(4, 7)
  g.begin_step = lambda: None
  fake.minmax_slots_init(g.act_slots)
  st = g.store
  if mode != 'train':                             # generic moving statistics instead of 0 / 1
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
      for v in st.vars:
        if v.kind == 'bn_mean':
          v.tensor.copy_(0.1 * torch.randn(v.tensor.shape, generator=gen))
        elif v.kind == 'bn_var':
          v.tensor.copy_(0.5 + torch.rand(v.tensor.shape, generator=gen))
  if mode == 'eval':
    with torch.no_grad(), g.as_default():
      logits = net(x, False)
  else:
    with g.as_default():
      logits = net(x, mode == 'train')
    (logits * wts).sum().backward()
  return dict(logits=logits.detach().clone(), w_grad=st.w_grad.clone(), o_grad=st.o_grad.clone(), state=st.state.clone(),
              calls=dict(fake.calls))


def _close(a, b, tol=2e-6):
  for k in ('logits', 'w_grad', 'o_grad', 'state'):
    err = float((a[k] - b[k]).abs().max() / (a[k].abs().max() + 1e-12))
    assert err <= tol, (k, err)


@pytest.mark.parametrize('act_bits', [None, 6])
def test_pooled_head_plumbing_is_exact_on_cpu(monkeypatch, act_bits):
  """Training mode: the final BN takes its statistics from conv3's epilogue, is reduced to the pooled tensor without an apply pass,
  and its backward runs in the pooled kernels, dgamma / dbeta straight into the flat gradient views."""
  a = _run_net(monkeypatch, HeadFakeHip(), False, act_bits, 'train')
  b = _run_net(monkeypatch, HeadFakeHip(), True, act_bits, 'train')
  _close(a, b)
  assert a['calls'].get('bn_pool', 0) == 0 and b['calls']['bn_pool'] == 1
  assert b['calls']['bn_apply'] == a['calls']['bn_apply'] - 1 and b['calls']['bn_stats'] == a['calls']['bn_stats']
  assert b['calls']['bn_bwd_stats_pooled'] == 1 == b['calls']['bn_bwd_apply_pooled']
  assert b['calls']['bn_bwd_stats'] == a['calls']['bn_bwd_stats'] - 1 and b['calls']['bn_bwd_apply'] == a['calls']['bn_bwd_apply'] - 1
  assert float(b['o_grad'].abs().max()) > 0.0


@pytest.mark.parametrize('mode,act_bits', [('eval', None), ('eval', 6), ('eval_grad', None)])
def test_pooled_head_in_inference_mode_is_exact_on_cpu(monkeypatch, mode, act_bits):
  """Inference mode without gradients (cached / fresh scale and shift, with and without a quantiser) and with gradients
  (BN_EVAL_GRAD: moving statistics, backward with zero sums)."""
  a = _run_net(monkeypatch, HeadFakeHip(), False, act_bits, mode)
  b = _run_net(monkeypatch, HeadFakeHip(), True, act_bits, mode)
  _close(a, b)
  assert b['calls']['bn_pool'] == 1 and b['calls'].get('bn_apply', 0) == a['calls']['bn_apply'] - 1
  if mode == 'eval_grad':
    assert b['calls']['bn_bwd_stats_pooled'] == 1 and float(b['o_grad'].abs().max()) > 0.0


def test_without_the_entry_points_or_with_taps_the_separate_chain_is_taken(monkeypatch):
  from pocketflow_amd import graph as G
  a = _run_net(monkeypatch, FakeHip(), False, None, 'train')
  b = _run_net(monkeypatch, FakeHip(), True, None, 'train')              # the double without the entry points: today's chain
  assert a['calls'] == b['calls'] and 'bn_pool' not in b['calls']
  for k in ('logits', 'w_grad', 'o_grad', 'state'):
    assert torch.equal(a[k], b[k]), k
  fake = HeadFakeHip()
  monkeypatch.setattr(G, 'hip', fake)
  monkeypatch.setattr(G, 'HEAD_FUSE', True)
  monkeypatch.setattr(G, 'HEAD_FUSE_ANY_DEVICE', True)
  g, net = _build(None)
  x = torch.randn(2, 16, 3, 3).contiguous(memory_format=torch.channels_last)
  assert G.head_fuse_ok(g, x)
  g.taps = {}
  assert not G.head_fuse_ok(g, x) and net.final_bn.pooled(x) is None   # taps: every layer's output must exist
  g.taps = None
  monkeypatch.setattr(G, 'HEAD_FUSE_ANY_DEVICE', False)
  assert not G.head_fuse_ok(g, x)                                       # a CPU tensor
  monkeypatch.setattr(G, 'HEAD_FUSE_ANY_DEVICE', True)
  monkeypatch.setattr(G, 'HEAD_FUSE', False)
  assert not G.head_fuse_ok(g, x)


@pytest.mark.parametrize('teacher', [False, True])
def test_one_loss_launch_plumbing_on_cpu(monkeypatch, teacher):
  """losses.softmax_cross_entropy after prime_distillation: one head launch, distillation_loss and top_k_accuracies pick their
  part up from the logits tensor, backward is one combine launch -- same values and gradients as the separate functions, also
  with upstream scalars other than 1; a teacher tensor other than the primed one is not picked up."""
  from pocketflow_amd import graph as G
  from pocketflow_amd import losses as L
  monkeypatch.setattr(G, 'HEAD_FUSE_ANY_DEVICE', True)
  gen = torch.Generator().manual_seed(1)
  z = torch.randn(6, 9, generator=gen)
  z[1, 2] = z[1, 4] = z[1].max() + 1.0
  z_t = torch.randn(6, 9, generator=gen)
  tgt = torch.tensor([0, 4, 8, 3, 3, 1])
  labels = torch.zeros(6, 9)
  labels[torch.arange(6), tgt] = 1.0
  res = {}
  for fuse in (False, True):
    fake = HeadFakeHipFull()
    monkeypatch.setattr(L, 'hip', fake)
    monkeypatch.setattr(G, 'HEAD_FUSE', fuse)
    zz = z.clone().requires_grad_(True)
    if teacher:
      L.prime_distillation(zz, z_t, 4.0, 3.0)
    ce = L.softmax_cross_entropy(labels, zz)
    a1, a5 = L.top_k_accuracies(labels, zz, (1, 5))
    total = 0.75 * ce
    dst = None
    if teacher:
      dst = L.distillation_loss(zz, z_t, 4.0, 3.0)
      total = total - 1.5 * dst
    total.backward()
    res[fuse] = (ce.detach(), dst.detach() if teacher else torch.zeros(()), a1, a5, zz.grad.clone(), dict(fake.calls))
  for a, b in zip(res[False][:5], res[True][:5]):
    assert float((a - b).abs().max()) <= 1e-6 * max(1.0, float(a.abs().max()))
  assert float(res[True][2]) == float(L.in_top_k(z, tgt, 1).float().mean()) and float(res[True][3]) == float(L.in_top_k(z, tgt, 5).float().mean())
  assert res[True][5] == {'ce_head': 1, 'ce_combine': 1} and res[False][5] == {'ce_plain': 2 if teacher else 1}
  if teacher:
    # asked about another teacher tensor (or other constants): the separate launch, nothing stale is handed out
    fake = HeadFakeHipFull()
    monkeypatch.setattr(L, 'hip', fake)
    zz = z.clone().requires_grad_(True)
    L.prime_distillation(zz, z_t, 4.0, 3.0)
    L.softmax_cross_entropy(labels, zz)
    other = L.distillation_loss(zz, 2.0 * z_t, 4.0, 3.0)
    assert fake.calls == {'ce_head': 1, 'ce_plain': 1} and abs(float(other) - float(res[True][1])) > 1e-3
    assert L.distillation_loss(zz, z_t, 2.0, 3.0) is not None and fake.calls['ce_plain'] == 2


def test_a_learner_step_with_the_fused_head_on_cpu(monkeypatch, tmp_path):
  """UniformQuantLearner + distillation on the CIFAR-10 ResNet-20 (batch 4): two steps with the switch off and on -- what the steps
  return and update agrees to float32 round-off; the fused run makes one loss launch and one combine per step and pools the final
  BN of student and teacher."""
  import pocketflow_amd.graph as G
  import pocketflow_amd.plan as P
  import pocketflow_amd.losses as L
  import pocketflow_amd.optim as Opt
  import pocketflow_amd.learners.abstract_learner as AL
  import pocketflow_amd.learners.learner_utils  # noqa: F401
  from pocketflow_amd.flags import FLAGS
  from pocketflow_amd.nets.resnet_at_cifar10 import ModelHelper
  from pocketflow_amd.learners.uniform_quantization.learner import UniformQuantLearner
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  monkeypatch.setattr(AL, 'require_gpu', lambda: torch.device('cpu'))
  monkeypatch.setattr(G, 'HEAD_FUSE_ANY_DEVICE', True)
  monkeypatch.setenv('PF_TEACHER_AHEAD', '0')
  for k, v in dict(save_path=str(tmp_path / 'models' / 'model.ckpt'), save_path_eval=str(tmp_path / 'models_eval' / 'model.ckpt'),
                   save_path_dst=str(tmp_path / 'models_dst' / 'model.ckpt'), uql_save_quant_model_path=str(tmp_path / 'uql' / 'm.ckpt'),
                   resnet_size=20, nb_classes=10, batch_size=4, batch_size_eval=4, compute_dtype='float32',
                   synthetic_pool=2, uql_weight_bits=8, uql_activation_bits=8, enbl_dst=True, dst_eval_teacher=False).items():
    setattr(FLAGS, k, v)
  # the initial values are not the subject: clipped normals instead of scipy's truncated-normal sampler (seconds per network)
  import scipy.stats
  monkeypatch.setattr(scipy.stats.truncnorm, 'rvs', lambda a, b, size=None, random_state=None:
                      np.clip(random_state.standard_normal(size), a, b))
  mh = ModelHelper()
  create_synthetic_checkpoint(mh)
  runs = {}
  for fuse in (False, True):
    fake = HeadFakeHipFull()
    for mod in (G, P, L, Opt):
      monkeypatch.setattr(mod, 'hip', fake)
    monkeypatch.setattr(G, 'HEAD_FUSE', fuse)
    lrn = UniformQuantLearner(None, mh)
    outs = [lrn.train_step() for _ in range(2)]
    vals = [float(o[k].detach()) for o in outs for k in ('model_loss', 'dst_loss', 'loss')]
    vals += [float(o['metrics']['accuracy'].detach()) for o in outs]
    runs[fuse] = (vals, lrn.graph.store.export_numpy(), dict(fake.calls))
  (va, sa, ca), (vb, sb, cb) = runs[False], runs[True]
  assert np.allclose(va, vb, rtol=1e-5, atol=1e-6), (va, vb)
  for k in sa:
    assert np.allclose(sa[k], sb[k], rtol=1e-4, atol=1e-5), k
  assert cb['ce_head'] == 2 and cb['ce_combine'] == 2 and 'ce_plain' not in cb and ca['ce_plain'] == 4 and 'ce_head' not in ca
  assert cb['bn_pool'] == 4 and cb['bn_bwd_stats_pooled'] == 2 and cb['bn_apply'] == ca['bn_apply'] - 4
