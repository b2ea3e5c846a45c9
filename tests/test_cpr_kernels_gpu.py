"""The 'chn-pruned-rmt' selection kernels (pocketflow_amd/csrc/pf_cpr.hip) against the NumPy restatement in tests/cpr_oracle.py."""
import numpy as np
import pytest
import torch

import cpr_oracle as O
from test_cpr_cpu import _case_inputs, _fixture, _pads

pytestmark = pytest.mark.gpu

# (B, H, W, C, Co, k, stride, padding): 1x1; 3x3 SAME; 3x3 stride 2 after a fixed pad; SAME stride 2 odd / even; 7x7 stem c_in = 3
GEOMS = [(4, 8, 8, 16, 24, 1, 1, 'SAME'), (3, 9, 7, 8, 16, 3, 1, 'SAME'), (2, 10, 10, 8, 8, 3, 2, 1), (2, 9, 9, 8, 12, 3, 2, 'SAME'),
         (2, 10, 10, 8, 12, 3, 2, 'SAME'), (2, 32, 32, 3, 16, 7, 2, 3)]


def _geom(H, W, k, stride, padding):
  if isinstance(padding, int):
    pt = pl = padding
    OH, OW = (H + 2 * padding - k) // stride + 1, (W + 2 * padding - k) // stride + 1
  else:
    pt, pl = O.same_pad(H, k, stride), O.same_pad(W, k, stride)
    OH, OW = -(-H // stride), -(-W // stride)
  return pt, pl, OH, OW


def _nhwc(a, dtype=torch.float32):
  return torch.from_numpy(a).to(dtype).cuda().permute(0, 3, 1, 2)          # logical NCHW, channels-last storage


@pytest.mark.parametrize('geom', GEOMS)
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_gather_is_the_reference_copy(geom, dtype):
  from pocketflow_amd import hip
  B, H, W, C, Co, k, stride, padding = geom
  pt, pl, OH, OW = _geom(H, W, k, stride, padding)
  rng = np.random.RandomState(1)
  x = rng.randn(B, H, W, C).astype(np.float32)
  y = rng.randn(B, OH, OW, Co).astype(np.float32)
  if dtype == torch.bfloat16:
    x = torch.from_numpy(x).bfloat16().float().numpy()
    y = torch.from_numpy(y).bfloat16().float().numpy()
  positions = [(0, 0), (OH - 1, OW - 1), (OH // 2, 0), (0, OW - 1), (rng.randint(OH), rng.randint(OW))]
  P_ref, Y_ref = O.gather(x, y, positions, k, k, stride, pt, pl)
  rows = 2 * len(positions) * B                       # second block at row0 = half: rows land where asked
  P = torch.full((rows * k * k * C,), float('nan'), device='cuda')
  Y = torch.full((rows * Co,), float('nan'), device='cuda')
  pos = torch.tensor(positions, dtype=torch.int32, device='cuda')
  hip.cpr_gather(_nhwc(x, dtype), _nhwc(y, dtype), pos, k, k, stride, pt, pl, P, Y, rows // 2)
  torch.cuda.synchronize()
  P = P.cpu().numpy().reshape(rows, k * k, C)
  Y = Y.cpu().numpy().reshape(rows, Co)
  assert np.isnan(P[:rows // 2]).all() and np.isnan(Y[:rows // 2]).all()
  assert np.array_equal(P[rows // 2:], P_ref) and np.array_equal(Y[rows // 2:], Y_ref)


@pytest.mark.parametrize('C,Co,k,n', [(16, 24, 1, 300), (8, 16, 3, 200), (3, 16, 7, 90), (130, 40, 1, 150), (64, 64, 3, 70)])
def test_gram_against_float64(C, Co, k, n):
  from pocketflow_amd import hip
  rng = np.random.RandomState(C + Co)
  rows = 2 * n
  P = rng.randn(rows, k * k, C).astype(np.float32)
  Y = rng.randn(rows, Co).astype(np.float32)
  w = (rng.randn(k, k, C, Co) * 0.1).astype(np.float32)
  idx = rng.choice(rows, n, replace=False)
  xtx_ref, xty_ref, (xtx64, xty64) = O.gram(P, Y, idx, w)
  w_krsc = torch.from_numpy(np.ascontiguousarray(w.transpose(3, 0, 1, 2))).cuda().reshape(-1)
  ws = torch.empty(hip.cpr_gram_ws(C), dtype=torch.float64, device='cuda')
  xtx = torch.empty(C * C, device='cuda')
  xty = torch.empty(C, device='cuda')
  hip.cpr_gram(torch.from_numpy(P).cuda().reshape(-1), torch.from_numpy(Y).cuda().reshape(-1),
               torch.from_numpy(idx.astype(np.int32)).cuda(), k * k, C, Co, w_krsc, ws, xtx, xty)
  xtx = xtx.cpu().numpy().reshape(C, C)
  xty = xty.cpu().numpy()
  for got, exact in ((xtx, xtx64), (xty, xty64)):
    ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
    floor = 1e-14 * np.abs(exact).max()                  # entries that cancel to ~0: float64 rounding of the sum itself
    assert np.all(np.abs(got - exact) <= 2 * ulp + floor)
  assert np.array_equal(xtx, xtx.T)
  assert np.mean(xtx == xtx_ref) > 0.95 and np.mean(xty == xty_ref) > 0.9


def _lasso_problem(C, Co, n, seed):
  rng = np.random.RandomState(seed)
  P = rng.randn(n, 1, C).astype(np.float32)
  w = (rng.randn(1, 1, C, Co) * 0.3).astype(np.float32)
  Y = (P.reshape(n, C) @ w.reshape(C, Co) + 0.1 * rng.randn(n, Co)).astype(np.float32)
  xtx, xty, __ = O.gram(P, Y, np.arange(n), w)
  return xtx, xty, rng.uniform(size=(C, 1))


def _ista_gpu(xtx, xty, m0, gamma, iters, lr=1e-2):
  from pocketflow_amd import hip
  C = xty.size
  A, b = torch.from_numpy(xtx).cuda().reshape(-1), torch.from_numpy(xty).cuda()
  m0_t = torch.from_numpy(m0.astype(np.float32).reshape(-1)).cuda()
  mask = torch.empty(C, device='cuda')
  nnz = torch.zeros(1, dtype=torch.int32, device='cuda')
  hip.cpr_ista(A, b, m0_t, torch.empty(2 * C, device='cuda'), mask, gamma, lr, iters, nnz)
  return mask.cpu().numpy(), int(nnz.item())


def test_ista_solve_against_float64():
  xtx, xty, m0 = _lasso_problem(48, 32, 400, 3)
  for gamma in (0.05, 0.2, 0.8):
    mask, nnz = _ista_gpu(xtx, xty, m0, gamma, 100)
    ref64 = O.ista(xtx, xty, m0, gamma, 1e-2, 100, dtype=np.float64)
    assert nnz == np.count_nonzero(mask)
    assert np.max(np.abs(mask - ref64)) <= 1e-5 * max(1.0, np.abs(ref64).max())
    thr = gamma * 1e-2
    margin = np.min(np.abs(np.abs(O.ista(xtx, xty, m0, gamma, 1e-2, 99, dtype=np.float64)) - thr))
    if margin > 1e-4:
      assert nnz == np.count_nonzero(ref64)


def test_bisection_path_matches_the_float32_oracle():
  from pocketflow_amd import hip  # noqa: F401
  xtx, xty, m0 = _lasso_problem(32, 24, 300, 5)
  target = 16
  mask_g, path_g = O.bisect(lambda x: _ista_gpu(xtx, xty, m0, x, 100), target)
  mask_o, path_o = O.bisect(lambda x: (lambda m: (m, int(np.count_nonzero(m))))(O.ista(xtx, xty, m0, x, 1e-2, 100)), target)
  assert [p[1] for p in path_g] == [p[1] for p in path_o] and [p[0] for p in path_g] == [p[0] for p in path_o]
  assert np.array_equal(mask_g != 0, mask_o != 0)


def _lstsq_gpu(P, Y, w_hwio, keep, iters, lrn_rate, wd, monkeypatch):
  from pocketflow_amd.learners.channel_pruning_rmt.learner import LayerSelector
  from pocketflow_amd.flags import FLAGS
  monkeypatch.setattr(FLAGS, 'cpr_lstsq_nb_iters', iters)
  monkeypatch.setattr(FLAGS, 'cpr_lstsq_lrn_rate', lrn_rate)
  kh, kw, C, Co = w_hwio.shape
  sel = LayerSelector(torch.device('cuda'))
  w_krsc = torch.from_numpy(np.ascontiguousarray(w_hwio.transpose(3, 0, 1, 2))).cuda().reshape(-1)
  w_new, before, after = sel.lstsq(torch.from_numpy(P).cuda().reshape(-1), torch.from_numpy(Y).cuda().reshape(-1), P.shape[0], w_krsc,
                                   kh * kw, C, Co, torch.from_numpy(keep).cuda(), wd)
  return w_new.cpu().numpy().reshape(Co, kh, kw, C).transpose(1, 2, 3, 0), before, after


@pytest.mark.parametrize('C,Co,k,N', [(16, 16, 3, 2000), (32, 64, 1, 3000), (3, 16, 7, 700)])
def test_lstsq_within_the_float32_noise_floor(C, Co, k, N, monkeypatch):
  rng = np.random.RandomState(C * Co)
  P = rng.randn(N, k * k, C).astype(np.float32)
  w = (rng.randn(k, k, C, Co) * 0.2).astype(np.float32)
  Y = rng.randn(N, Co).astype(np.float32)
  keep = rng.rand(C) < 0.6
  keep[0] = True
  w32, b32, a32 = O.lstsq(P, Y, w, keep, 100, 1e-3, 1e-4)
  w64, __, a64 = O.lstsq(P, Y, w, keep, 100, 1e-3, 1e-4, dtype=np.float64)
  wg, bg, ag = _lstsq_gpu(P, Y, w, keep, 100, 1e-3, 1e-4, monkeypatch)
  floor = np.max(np.abs(w32.astype(np.float64) - w64))                  # measured: float32 statements vs the same in float64
  assert np.all(wg[:, :, ~keep, :] == 0)
  assert np.max(np.abs(wg - w64)) <= 4 * floor + 1e-6, (np.max(np.abs(wg - w64)), floor)
  assert abs(bg[0] - b32[0]) <= 1e-5 * abs(b32[0]) and abs(ag[0] - a32[0]) <= 1e-3 * abs(a32[0])


@pytest.mark.parametrize('C,Co,k', [(2048, 512, 1), (512, 512, 3)])
def test_resnet50_extremes_stay_finite_and_masked(C, Co, k, monkeypatch):
  from pocketflow_amd import hip
  from pocketflow_amd.learners.channel_pruning_rmt.learner import LayerSelector
  from pocketflow_amd.flags import FLAGS
  for name, v in (('cpr_ista_nb_iters', 100), ('cpr_ista_lrn_rate', 1e-2), ('cpr_lstsq_nb_iters', 3), ('cpr_lstsq_lrn_rate', 1e-3)):
    monkeypatch.setattr(FLAGS, name, v)
  N = 50000
  g = torch.Generator(device='cuda').manual_seed(0)
  P = torch.randn(N * k * k * C, device='cuda', generator=g)
  Y = torch.randn(N * Co, device='cuda', generator=g)
  w = torch.randn(Co * k * k * C, device='cuda', generator=g) * 0.02
  sel = LayerSelector(torch.device('cuda'))
  rng = np.random.RandomState(0)
  idx = rng.choice(N, O.secondary_size(N, Co), replace=False)
  keep, path = sel.lasso(P, Y, idx, w, k * k, C, Co, rng.uniform(size=(C, 1)), C // 2)
  assert len(path) >= 1 and all(0 <= p[1] <= C for p in path)
  keep[: C // 4] = True
  keep[C // 4: C // 2] = False
  w_new, before, after = sel.lstsq(P, Y, N, w, k * k, C, Co, keep, 1e-4)
  w_new = w_new.view(Co, k * k, C)
  assert torch.isfinite(w_new).all() and np.isfinite(before).all() and np.isfinite(after).all()
  assert (w_new[:, :, ~keep] == 0).all() and (w_new[:, :, keep] != 0).any()
  assert hip.cpr_lstsq_splits(N, int(keep.sum()) * k * k, Co) >= 1


# ---- the reference-executed fixture (tests/golden/cpr) ---------------------------------------------------------------------
def test_gather_reproduces_the_fixture():
  """Unpadded taps (as this package holds a fixed-pad convolution's input), the fixture's positions: the reference's P / Y bit for bit."""
  from pocketflow_amd import hip
  meta, z = _fixture()
  crops = meta['crops']
  for case in meta['cases']:
    p, k, C, Co = case['name'] + '/', case['k'], case['C'], case['Co']
    x, y = _case_inputs(case, z)
    pos_all = z[p + 'positions'].astype(np.int32).reshape(-1, crops, 2)
    B = x.shape[1]
    rows = case['nb_mbtcs_used'] * crops * B
    P = torch.empty(rows * k * k * C, device='cuda')
    Y = torch.empty(rows * Co, device='cuda')
    pt, pl = _pads(case, x.shape[2], x.shape[3])
    for mb in range(case['nb_mbtcs_used']):
      hip.cpr_gather(_nhwc(x[mb]), _nhwc(y[mb]), torch.from_numpy(pos_all[mb]).cuda(), k, k, case['stride'], pt, pl, P, Y, mb * crops * B)
    sel = torch.from_numpy(z[p + 'idxs_inst']).cuda()
    assert np.array_equal(P.view(rows, k * k, C)[sel].cpu().numpy(), z[p + 'P']), case['name']
    assert np.array_equal(Y.view(rows, Co)[sel].cpu().numpy(), z[p + 'Y']), case['name']


def test_gram_and_gamma_path_reproduce_the_fixture():
  """X^T X / X^T y within 2 ulp of the reference's float32 values (equal almost everywhere); the device ISTA on the reference's
  float32 inputs walks the reference's (gamma, nnz) path to its mask."""
  from pocketflow_amd import hip
  meta, z = _fixture()
  same = total = 0
  for case in meta['cases']:
    p, k, C, Co = case['name'] + '/', case['k'], case['C'], case['Co']
    w_krsc = torch.from_numpy(np.ascontiguousarray(z[p + 'w'].transpose(3, 0, 1, 2))).cuda().reshape(-1)
    ws = torch.empty(hip.cpr_gram_ws(C), dtype=torch.float64, device='cuda')
    xtx, xty = torch.empty(C * C, device='cuda'), torch.empty(C, device='cuda')
    hip.cpr_gram(torch.from_numpy(z[p + 'P']).cuda().reshape(-1), torch.from_numpy(z[p + 'Y']).cuda().reshape(-1),
                 torch.from_numpy(z[p + 'idxs_rdc'].astype(np.int32)).cuda(), k * k, C, Co, w_krsc, ws, xtx, xty)
    for got, want in ((xtx.cpu().numpy(), z[p + 'xtx'].reshape(-1)), (xty.cpu().numpy(), z[p + 'xty'])):
      assert np.all(np.abs(got - want) <= 2 * np.spacing(np.abs(want)) + 1e-7 * np.abs(want).max()), case['name']
      same += int(np.sum(got == want))
      total += got.size
    mask, path = O.bisect(lambda g: _ista_gpu(z[p + 'xtx'], z[p + 'xty'], z[p + 'mask_init'], g, 100), case['target'])
    assert [list(q) for q in path] == case['path'], (case['name'], path)
    assert np.array_equal(mask != 0, z[p + 'mask'] != 0)
  assert same >= 0.9 * total, (same, total)


def test_lstsq_reproduces_the_fixture(monkeypatch):
  """100 Adam steps from the reference's mask: within 4x the float32-vs-float64 distance of the same statements (+1e-6)."""
  meta, z = _fixture()
  for case in meta['cases']:
    p = case['name'] + '/'
    keep = z[p + 'mask'] != 0
    w64, __, __ = O.lstsq(z[p + 'P'], z[p + 'Y'], z[p + 'w'], keep, 100, 1e-3, meta['loss_w_dcy'], dtype=np.float64)
    floor = np.max(np.abs(z[p + 'kernel'].astype(np.float64) - w64))
    wg, bg, ag = _lstsq_gpu(z[p + 'P'], z[p + 'Y'], z[p + 'w'], keep, 100, 1e-3, meta['loss_w_dcy'], monkeypatch)
    assert np.max(np.abs(wg - z[p + 'kernel'])) <= 4 * floor + 1e-6, case['name']
    assert np.all(wg[:, :, ~keep, :] == 0)
    assert abs(ag[0] - case['losses'][1][0]) <= 1e-4 * abs(case['losses'][1][0]), case['name']
