"""The plumbing of the projection join (graph._FusedConv1x1.backward) on the CPU: with a `hip` object that offers
`conv1x1_bwd_data_join`, the strided shortcut of a projection block parks a COMPACT input gradient (a plain dense GEMM: no zero fill,
no row scatter) which conv1's backward-data reads through the inverse row map, and that launch leaves bn1's BN-backward sums, so that
the BN backward skips its statistics pass.  A `hip` object without the entry (tests/fake_hip.py as it stands) keeps today's route."""
import pytest
import torch

from fake_hip import FakeHip, _mask, _rows
from test_fused_plumbing_cpu import _build


class _Counting(FakeHip):
  """FakeHip that also counts the row-scatter launches (backward-data of a strided projection into a zero-filled tensor)."""

  def conv1x1_fwd(self, X, W, Y, M, N, K, R=None, scale_shift=None, act=None, slot=None, bits=8, partial=None, geom=None,
                  ymap=False, out_scale_shift=None, out_act=None):
    if ymap:
      self._n('conv1x1_ymap')
    return FakeHip.conv1x1_fwd(self, X, W, Y, M, N, K, R=R, scale_shift=scale_shift, act=act, slot=slot, bits=bits, partial=partial,
                               geom=geom, ymap=ymap, out_scale_shift=out_scale_shift, out_act=out_act)


class _JoinHip(_Counting):
  """... plus float32 emulations of pf_conv1x1_join_plan / pf_conv1x1_bwd_data_join (include/pocketflow_hip.h)."""

  def __init__(self, accept=True):
    super(_JoinHip, self).__init__()
    self.accept = accept

  def conv1x1_join_plan(self, M, N, K, with_stats=False):
    return 1 if self.accept else 0

  def conv1x1_bwd_data_join(self, dY, Wt, dQ, R, M, N, K, rgeom=None, bn_x=None, bn_scale_shift=None, bn_mean_invstd=None,
                            bn_act=None, partial=None):
    self._n('conv1x1_join' if bn_x is None else 'conv1x1_join_stats')
    dq = _rows(dY, N).float() @ Wt.float().t()
    if rgeom is None:
      dq = dq + _rows(R, K).float()
    else:
      ho, wo, h, w, s = rgeom
      assert tuple(R.shape[2:]) == (ho, wo) and M % (h * w) == 0
      res = torch.zeros(M // (h * w), h, w, K)
      res[:, ::s, ::s, :] = R.permute(0, 2, 3, 1).float()
      dq = dq + res.reshape(M, K)
    _rows(dQ, K).copy_(dq)
    if bn_x is not None:
      xr = _rows(bn_x, K).float()
      dy = dq * _mask(xr * bn_scale_shift[0] + bn_scale_shift[1], bn_act)
      partial.zero_()
      partial[2, 0], partial[2, 1] = dy.sum(0), (dy * (xr - bn_mean_invstd[0]) * bn_mean_invstd[1]).sum(0)


def _run(monkeypatch, fake, stats):
  from pocketflow_amd import graph as G
  monkeypatch.setattr(G, 'hip', fake)
  monkeypatch.setattr(G, 'fusable_tensor', lambda t: True)
  monkeypatch.setattr(G, 'PROJ_JOIN', True)
  monkeypatch.setattr(G, 'PROJ_JOIN_STATS', stats)
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
  proj = [b for b in net.blocks if b.proj is not None]
  return dict(logits=logits.detach().clone(), w_grad=st.w_grad.clone(), o_grad=st.o_grad.clone(), state=st.state.clone(),
              calls=dict(fake.calls), n_proj=len(proj), n_strided=sum(1 for b in proj if b.proj.strides > 1))


def test_compact_shortcut_gradient_is_the_same_arithmetic(monkeypatch):
  """Part 1 alone: no row scatter, one joined launch per strided projection block, every result EQUAL (the zero-filled tensor added
  0.0 where the compact one adds nothing)."""
  a = _run(monkeypatch, _Counting(), False)
  b = _run(monkeypatch, _JoinHip(), False)
  assert a['n_proj'] == 2 and a['n_strided'] == 1          # the network of test_fused_plumbing_cpu: strides [1, 2]
  assert a['calls'].get('conv1x1_ymap', 0) == a['n_strided'] and a['calls'].get('conv1x1_join', 0) == 0
  assert b['calls'].get('conv1x1_ymap', 0) == 0 and b['calls'].get('conv1x1_join', 0) == b['n_strided']
  assert b['calls'].get('conv1x1_join_stats', 0) == 0
  assert b['calls']['bn_bwd_stats'] == a['calls']['bn_bwd_stats']
  # the compact GEMM replaces the scatter launch, the joined launch the residual launch: one plain launch fewer per strided block
  assert b['calls']['conv1x1_plain'] == a['calls']['conv1x1_plain'] - b['n_strided']
  for k in ('logits', 'w_grad', 'o_grad', 'state'):
    assert torch.equal(a[k], b[k]), k


def test_bn_backward_sums_come_from_the_joined_launch(monkeypatch):
  """Both parts: every projection block (the stride-1 one of stage 1 included) loses its separate statistics pass."""
  a = _run(monkeypatch, _Counting(), True)
  b = _run(monkeypatch, _JoinHip(), True)
  assert b['calls'].get('conv1x1_ymap', 0) == 0
  assert b['calls'].get('conv1x1_join_stats', 0) == b['n_proj'] and b['calls'].get('conv1x1_join', 0) == 0
  assert b['calls']['bn_bwd_stats'] == a['calls']['bn_bwd_stats'] - b['n_proj']
  for k in ('logits', 'w_grad', 'o_grad', 'state'):
    err = float((a[k] - b[k]).abs().max() / (a[k].abs().max() + 1e-12))
    assert err <= 2e-5, (k, err)       # the bound of test_fused_plumbing_cpu for 8 filters without quantisers


def test_a_refused_shape_and_a_library_without_the_entry_keep_todays_route(monkeypatch):
  a = _run(monkeypatch, _Counting(), True)
  b = _run(monkeypatch, _JoinHip(accept=False), True)
  assert b['calls'] == a['calls']
  for k in ('logits', 'w_grad', 'o_grad', 'state'):
    assert torch.equal(a[k], b[k]), k
