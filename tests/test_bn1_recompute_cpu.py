"""The plumbing of the pair without conv1's input gradient (graph._conv1x1_bwd_data_plan 'bnsums', BnSums.defer, _bn_backward) on
the CPU.  tests/fake_hip.py as it stands has none of the three entries and keeps today's route; a stand-in that gains all three runs
the identity blocks through them: the sums-only launch, a placeholder gradient that owns one element, and the recomputing apply
launch inside the BN node -- with identical gradients, since the stand-in's float32 arithmetic is the same on both routes."""
import pytest
import torch

from fake_hip import FakeHip, _mask, _rows
from test_fused_plumbing_cpu import _build


class _PairHip(FakeHip):
  """FakeHip plus float32 emulations of pf_conv1x1_bwd_apply_plan / _bwd_data_bnsums / _bwd_data_bnapply."""

  def __init__(self, accept=True):
    super(_PairHip, self).__init__()
    self.accept = accept
    self.placeholders = []

  def conv1x1_bwd_apply_plan(self, M, N, K, dtype=torch.bfloat16):
    return 1 if (self.accept and K >= 2 * N) else 0

  def conv1x1_bwd_data_bnsums(self, dY, Wt, bn_x, bn_ss, bn_mi, bn_act, partial, M, N, K):
    self._n('conv1x1_bwd_data_bnsums')
    dq = _rows(dY, N).float() @ Wt.float().t()
    xr = _rows(bn_x, K).float()
    dy = dq * _mask(xr * bn_ss[0] + bn_ss[1], bn_act)
    partial.zero_()
    partial[2, 0], partial[2, 1] = dy.sum(0), (dy * (xr - bn_mi[0]) * bn_mi[1]).sum(0)

  def conv1x1_bwd_data_bnapply(self, dY, Wt, x, ss, mi, act, dgamma, dbeta, addend, dx, M, N, K):
    self._n('conv1x1_bwd_data_bnapply')
    dq = _rows(dY, N).float() @ Wt.float().t()
    xr = _rows(x, K).float()
    dy = dq * _mask(xr * ss[0] + ss[1], act)
    out = ss[0] * (dy - dbeta / M - (xr - mi[0]) * mi[1] * dgamma / M)
    if addend is not None:
      out = out + _rows(addend, K).float()
    _rows(dx, K).copy_(out)


def _run(monkeypatch, fake, recompute=True):
  from pocketflow_amd import graph as G
  monkeypatch.setattr(G, 'hip', fake)
  monkeypatch.setattr(G, 'fusable_tensor', lambda t: True)
  monkeypatch.setattr(G, 'BN1_RECOMPUTE', recompute)
  seen = []
  defer = G.BnSums.defer

  def spy(self, *a, **kw):
    p = defer(self, *a, **kw)
    seen.append((tuple(p.shape), tuple(p.stride()), p.untyped_storage().nbytes() // p.element_size()))
    return p
  monkeypatch.setattr(G.BnSums, 'defer', spy)
  g, net = _build(True, fake, None, 8)
  torch.manual_seed(0)
  x = torch.randn(4, 3, 12, 12).contiguous(memory_format=torch.channels_last)
  wts = torch.randn(4, 7)
  g.begin_step = lambda: None
  fake.minmax_slots_init(g.act_slots)
  with g.as_default():
    logits = net(x, True)
  (logits * wts).sum().backward()
  st = g.store
  n_identity = sum(1 for b in net.blocks if b.proj is None)
  return dict(logits=logits.detach().clone(), w_grad=st.w_grad.clone(), o_grad=st.o_grad.clone(), state=st.state.clone(),
              calls=dict(fake.calls), n_identity=n_identity, placeholders=seen)


def _same(a, b):
  for k in ('logits', 'w_grad', 'o_grad', 'state'):
    assert torch.equal(a[k], b[k]), k


def test_a_library_without_the_entries_keeps_todays_route(monkeypatch):
  """tests/fake_hip.py has none of the three: nothing is deferred, and the switch changes nothing."""
  a = _run(monkeypatch, FakeHip(), True)
  b = _run(monkeypatch, FakeHip(), False)
  assert a['calls'] == b['calls'] and not a['placeholders']
  assert a['calls'].get('bn_bwd_apply_add', 0) == a['n_identity'] == 2
  _same(a, b)


def test_the_switch_and_a_refusing_plan_keep_todays_route(monkeypatch):
  a = _run(monkeypatch, FakeHip(), True)
  for fake, recompute in ((_PairHip(), False), (_PairHip(accept=False), True)):
    b = _run(monkeypatch, fake, recompute)
    assert b['calls'] == a['calls'] and not b['placeholders']
    _same(a, b)


def test_identity_blocks_run_the_pair_and_give_identical_gradients(monkeypatch):
  a = _run(monkeypatch, FakeHip(), True)
  b = _run(monkeypatch, _PairHip(), True)
  n = b['n_identity']
  assert n == 2
  # conv1 of every identity block: sums-only launch instead of the storing one, the apply pass inside the recomputing launch
  assert b['calls'].get('conv1x1_bwd_data_bnsums', 0) == n and b['calls'].get('conv1x1_bwd_data_bnapply', 0) == n
  assert b['calls']['conv1x1_bwd_data_bnstats'] == a['calls']['conv1x1_bwd_data_bnstats'] - n
  assert b['calls'].get('bn_bwd_apply_add', 0) == a['calls']['bn_bwd_apply_add'] - n == 0
  assert b['calls'].get('bn_bwd_apply', 0) == a['calls'].get('bn_bwd_apply', 0)
  assert b['calls']['bn_bwd_stats'] == a['calls']['bn_bwd_stats']
  # what autograd carried in place of the gradient: x's shape on ONE element of memory
  assert len(b['placeholders']) == n
  for shape, stride, elements in b['placeholders']:
    assert len(shape) == 4 and stride == (0, 0, 0, 0) and elements == 1
  _same(a, b)


def test_a_deferred_gradient_that_does_not_come_back_is_an_error():
  from pocketflow_amd import graph as G
  rec = G.BnSums()
  x = torch.zeros(2, 8, 3, 3)
  p = rec.defer(torch.zeros(3, 2, 8), 3, torch.zeros(18, 4), torch.zeros(8, 4), 18, 4, 8, x)
  assert p.shape == x.shape and rec.sums_for(p) is not None
  assert rec.deferred_for(torch.zeros_like(x)) is None and rec.deferred is not None
  assert rec.deferred_for(p)[2:] == (18, 4, 8) and rec.deferred is None
