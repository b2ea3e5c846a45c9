"""tests/wrw_exact.py checked without a GPU: the integer reference against autograd in float64 (torch.equal -- the inputs are integers),
the input generators against their stated bounds, the exactness guard, the guarded workspace, and every ROUTE the GPU cases of
tests/test_wrw_exact_gpu.py claim, against the library's own host-side queries."""
import pytest
import torch

import wrw_exact as WX
from wrw_exact import geom


def _autograd(dy, x, g, explicit_pad=None):
  """dW of torch's convolution, [N][th][tw][C] float64; explicit_pad = (top, bottom, left, right): pad x first, then convolve with pad 0."""
  xt = x.double().permute(0, 3, 1, 2)
  pad = [g.pad_h, g.pad_w]
  if explicit_pad is not None:
    t, b, l, r = explicit_pad
    xt = torch.nn.functional.pad(xt, (l, r, t, b))
    pad = [0, 0]
  w0 = torch.zeros(g.N, g.C, g.th, g.tw, dtype=torch.float64)
  dw = torch.ops.aten.convolution_backward(dy.double().permute(0, 3, 1, 2).contiguous(), xt.contiguous(), w0, None, [g.stride, g.stride], pad,
                                           [1, 1], False, [0, 0], 1, [False, True, False])[1]
  return dw.permute(0, 2, 3, 1).contiguous()


# (name, geometry, explicit padding for autograd or None)
REF_CASES = [
    ('3x3-s1', geom(3, 7, 7, 16, 8, 3, 3, 1, 1, 1), None),
    ('3x3-s2', geom(2, 9, 9, 8, 16, 3, 3, 2, 1, 1), None),
    ('3x3-s2-even-symmetric', geom(2, 8, 8, 8, 8, 3, 3, 2, 1, 1), None),     # the last input row / column is never read
    ('1x1-s2', geom(3, 7, 5, 16, 16, 1, 1, 2, 0, 0), None),
    ('5x5-pad2', geom(2, 6, 5, 8, 8, 5, 5, 1, 2, 2), None),
    ('3x1-pad1,0', geom(2, 5, 6, 8, 16, 3, 1, 1, 1, 0), None),
    ('1x3-pad0,1', geom(2, 5, 6, 8, 16, 1, 3, 1, 0, 1), None),
    ('tf-same-s2-even', geom(2, 8, 6, 8, 8, 3, 3, 2, 0, 0, 4, 3), (0, 1, 0, 1)),   # leading pad 0, one trailing row and column
    ('3x3-s1-nonsquare', geom(2, 4, 9, 8, 8, 3, 3, 1, 1, 1), None),
    ('3x3-s2-nonsquare-odd', geom(2, 9, 5, 8, 8, 3, 3, 2, 1, 1), None),
]


@pytest.mark.parametrize('name,g,explicit', REF_CASES, ids=[c[0] for c in REF_CASES])
def test_ref_wrw_equals_autograd(name, g, explicit):
  dy, x = WX.int_inputs(WX.seed_of(name), (g.imgs, g.Ho, g.Wo, g.N), (g.imgs, g.H, g.W, g.C))
  ref = WX.ref_wrw(dy, x, g.th, g.tw, g.stride, g.pad_h, g.pad_w, g.Ho, g.Wo)
  assert ref.dtype == torch.float64 and tuple(ref.shape) == (g.N, g.th, g.tw, g.C)
  assert torch.equal(ref, _autograd(dy, x, g, explicit))
  assert bool(ref.abs().max() > 0)
  assert torch.equal(WX.expected(ref, torch.float32).double(), ref)


def test_ref_prologue_values():
  x = torch.tensor([[-3., 0., 3.], [1., 2., -1.]]).to(torch.bfloat16)
  scale, shift = torch.tensor([1., 2., 2.]), torch.tensor([-4., 1., 4.])
  assert WX.ref_prologue(x, scale, shift, 'Relu').tolist() == [[0., 1., 10.], [0., 5., 2.]]
  assert WX.ref_prologue(x, scale, shift, 'Relu6').tolist() == [[0., 1., 6.], [0., 5., 2.]]
  assert WX.ref_prologue(x, scale, shift, None).tolist() == [[-7., 1., 10.], [-3., 5., 2.]]
  for act in ('Relu', 'Relu6'):
    _, xx = WX.int_inputs(5, (1,), (4000, 64))
    ss = WX.int_scale_shift(6, 64)
    q = WX.ref_prologue(xx, ss[0], ss[1], act)
    assert float(q.min()) == 0 and float(q.max()) == WX.prologue_bound(act)
    assert torch.equal(q, q.to(torch.bfloat16).double())           # exact in bf16


def test_generators_stay_inside_their_bounds():
  dy, x = WX.int_inputs(7, (50, 40), (60, 30))
  assert dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16
  assert sorted(set(dy.float().flatten().tolist())) == [-2., -1., 0., 1., 2.]
  assert sorted(set(x.float().flatten().tolist())) == [-3., -2., -1., 0., 1., 2., 3.]
  dy2, x2 = WX.int_inputs(7, (50, 40), (60, 30))
  assert torch.equal(dy, dy2) and torch.equal(x, x2)                # one seed, one case
  assert not torch.equal(x, WX.int_inputs(8, (50, 40), (60, 30))[1])
  ss = WX.int_scale_shift(3, 256)
  assert ss.dtype == torch.float32 and tuple(ss.shape) == (2, 256)
  assert set(ss[0].tolist()) == {1., 2.} and set(ss[1].tolist()) <= set(float(v) for v in range(-4, 5))
  assert int((ss[1] > 0).sum()) > 128 and int((ss[1] <= 0).sum()) > 0


def test_exact_regime_guard_fires():
  WX.assert_exact_regime(70000)
  WX.assert_exact_regime((2 ** 24 - 1) // 6)
  with pytest.raises(AssertionError):
    WX.assert_exact_regime(2 ** 24 // 6 + 1)
  WX.assert_exact_regime(2107, x_bound=10)
  with pytest.raises(AssertionError):
    WX.assert_exact_regime(2 ** 24 // 20 + 1, x_bound=10)


def test_guarded_workspace_layout_and_check():
  ws, check = WX.guarded_workspace(3, 10, device='cpu')
  assert ws.numel() == 35 * 10 and bool(torch.isnan(ws).all()) and ws.data_ptr() % 16 == 0 and WX.GUARD % 4 == 0
  check()
  ws.zero_()
  check()                                                          # the body is the caller's
  base = torch.as_strided(ws, (ws.numel() + 1,), (1,))             # one float past the documented size
  base[-1] = 0.0
  with pytest.raises(AssertionError, match='PAST'):
    check()
  ws, check = WX.guarded_workspace(1, 8, device='cpu')
  torch.as_strided(ws, (1,), (1,), ws.storage_offset() - 1)[0] = 1.0
  with pytest.raises(AssertionError, match='BELOW'):
    check()


def test_assert_equal_reports_where(capsys):
  ref = torch.zeros(4, 3, 3, 8)
  got = ref.clone()
  WX.assert_equal(got, ref)
  got[2, 1, 0, 5] = 2.0
  got[3, 2, 2, 7] = float('nan')
  with pytest.raises(AssertionError):
    WX.assert_equal(got, ref, 'demo')
  out = capsys.readouterr().out
  assert '2 of 288 entries differ' in out and '(n, tap, c) = (2, 3, 5)' in out and '(3, 8, 7)' in out and 'largest finite difference 2.0' in out


def test_fold_classes():
  assert WX.reduce_ranges(7, 4096) == (1, 7, [7])
  assert WX.reduce_ranges(9, 4096) == (2, 5, [5, 4])
  assert WX.reduce_ranges(130, 4096) == (16, 9, [9] * 14 + [4, 0])
  assert WX.reduce_ranges(33, 65536) == (1, 33, [33])


def test_every_gpu_case_is_on_the_route_it_names(monkeypatch):
  """The route assertions of tests/test_wrw_exact_gpu.py, run against the library's host-side queries: tile, map, slab count, fold class
  of every case, before any GPU is involved."""
  import test_wrw_exact_gpu as T
  from pocketflow_amd import hip
  n = 0
  for route, cases in T.ROUTES:
    for c in cases:
      route(hip, monkeypatch, *c)
      n += 1
  assert n == len(T.A_CASES) + len(T.B_CASES) + len(T.C_CASES) + len(T.D_CASES) + len(T.E_CASES) + len(T.F_CASES) + len(T.G_CASES) > 100
  # every shared-tile configuration of pf_wrw2_launch is reached with more than one tap, on both non-identity maps
  tiles = set((c[3], c[5]) for c in T.A_CASES)
  for tile in [(128, 256), (64, 256), (256, 128), (128, 128), (256, 64), (64, 128), (64, 64)]:
    assert (tile, 1) in tiles and (tile, 2) in tiles
