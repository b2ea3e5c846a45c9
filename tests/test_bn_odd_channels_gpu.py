"""The BatchNorm / quantiser passes at channel counts C % 8 == 0 whose groups of 8 do not divide the workgroup (pf_bn_vector_ok): the
(row, 8-channel) vector map with idle left-over lanes in the element-wise kernels, slabs with a guarded last slab in the two reductions.

Element-wise entries (pf_bn_act_quant_apply, pf_bn_bwd_apply[_add], pf_bn_act_quant_static in its three output kinds,
pf_bn_act_quant_codes, pf_bn_act_quant_pool): the vector route on an aligned tensor against the scalar loop, which the same entry takes
for a copy of the input placed 4 bytes off 16-byte alignment -- bit-identical outputs, float32 and bf16.
Reductions (pf_bn_stats, pf_bn_bwd_stats): float64 sums of the very terms the kernel adds, within the rounding of its float32 chain;
exact min / max; bit-equal repeats.  Outputs are filled with NaN first and read in full: a lane that skipped its work, or a thread that
wrote a channel >= C into the next row of the partial sums, shows."""
import numpy as np
import pytest
import torch

from oracle import pf_oracle as O

pytestmark = pytest.mark.gpu

# rows x C: 3 .. 255 groups of 8 channels; rows below / above one trip of a workgroup, one row, ragged tails
SHAPES = [(777, 24), (1000, 48), (3137, 96), (515, 144), (200, 576), (65, 960), (33, 1032), (3, 2040), (1, 96)]
DTYPES = [torch.float32, torch.bfloat16]
ACT = 'Relu6'


@pytest.fixture(scope='module')
def hip():
  from pocketflow_amd import hip as h
  assert torch.cuda.is_available(), 'gpu tests need a GPU'
  return h


def dev(a, dtype=None):
  t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
  return t if dtype is None else t.to(dtype)


def _off4(t):
  """A copy of t that starts 4 bytes behind a 16-byte boundary: the entries take their scalar loops for it."""
  n, skip = t.numel(), 4 // t.element_size()
  buf = torch.zeros(n + 16, dtype=t.dtype, device=t.device)
  assert buf.data_ptr() % 16 == 0
  view = buf[skip:skip + n].view(t.shape)
  view.copy_(t)
  assert view.data_ptr() % 16 == 4
  return view


def _nan(shape, dtype):
  return torch.full(shape, float('nan'), dtype=dtype, device='cuda') if dtype != torch.uint8 else torch.full(shape, 171, dtype=dtype, device='cuda')


@pytest.fixture(scope='module')
def data():
  """Per (rows, C, dtype): x, dq, addend in the storage type; scale / shift, mean / invstd, dgamma / dbeta in float32."""
  cache = {}

  def get(rows, C, dtype):
    key = (rows, C, dtype)
    if key not in cache:
      g = torch.Generator(device='cuda').manual_seed(rows * 31 + C)
      r = lambda *s: torch.randn(*s, device='cuda', generator=g)
      x = (r(rows, C) * 2 + r(C) * 3).to(dtype)
      scale = (torch.rand(C, device='cuda', generator=g) + 0.5) * torch.where(torch.rand(C, device='cuda', generator=g) > 0.8, -1.0, 1.0)
      cache[key] = dict(x=x, dq=r(rows, C).to(dtype), addend=r(rows, C).to(dtype),
                        ss=torch.stack([scale, r(C) + 1.0]).contiguous(),
                        mi=torch.stack([r(C) * 3, torch.rand(C, device='cuda', generator=g) + 0.25]).contiguous(),
                        dgamma=r(C) * rows ** 0.5, dbeta=r(C) * rows ** 0.5)
    return cache[key]
  return get


def _slot_of(hip, d):
  """A slot calibrated on act(scale * x + shift) itself, as the finalize pass leaves it."""
  y = torch.clamp(d['x'].float() * d['ss'][0] + d['ss'][1], 0.0, 6.0)
  slot = torch.empty((1, 2), dtype=torch.int32, device='cuda')
  hip.minmax_slots_init(slot)
  hip.minmax_tensor(y.contiguous(), slot[0], None)
  return slot


def _both_routes(x, run):
  """run(x_variant) -> output tensor, on the aligned tensor and on its copy 4 bytes off; the two outputs."""
  assert x.data_ptr() % 16 == 0
  return run(x), run(_off4(x))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('rows,C', SHAPES)
def test_elementwise_passes_vector_route_equals_scalar_route(hip, data, rows, C, dtype):
  assert hip.bn_vector_ok(C)
  d = data(rows, C, dtype)
  x, ss = d['x'], d['ss']
  slot = _slot_of(hip, d)

  def same(a, b, what):
    assert a.dtype == b.dtype and not torch.isnan(a.float()).any(), what
    assert torch.equal(a, b), (what, int((a != b).sum()))

  # forward apply: quantised and not
  for quantize in (True, False):
    def apply(xv):
      q = _nan((rows, C), dtype)
      hip.bn_act_quant_apply(xv, q, rows, C, ss, ACT, slot[0], 8, quantize)
      return q
    same(*_both_routes(x, apply), 'bn_act_quant_apply quantize=%s' % quantize)

  # backward apply, with and without the shortcut's gradient
  for addend in (None, d['addend']):
    def bwd(xv):
      dx = _nan((rows, C), dtype)
      hip.bn_bwd_apply(d['dq'], xv, dx, rows, C, ss, d['mi'], d['dgamma'], d['dbeta'], ACT, addend=addend)
      return dx
    same(*_both_routes(x, bwd), 'bn_bwd_apply addend=%s' % (addend is not None))

  # static quantiser: codes, float32 values, bf16 values
  ab = torch.tensor([5.5, 0.25], device='cuda')             # a range that clamps both ends of relu6(...)
  for out_dtype in (torch.uint8, torch.float32, torch.bfloat16):
    def static(xv):
      out = _nan((rows, C), out_dtype)
      hip.bn_act_quant_static(xv, out, rows, C, ss, ACT, ab, 8)
      return out
    a, b = _both_routes(x, static)
    assert torch.equal(a, b), ('bn_act_quant_static', out_dtype)
    assert out_dtype == torch.uint8 or not torch.isnan(a.float()).any()

  # codes of the per-batch quantiser
  def codes(xv):
    out = _nan((rows, C), torch.uint8)
    pair = _nan((2,), torch.float32)
    hip.bn_act_quant_codes(xv, out, rows, C, ss, ACT, slot[0], 8, pair)
    return torch.cat([out.reshape(-1).float(), pair])
  a, b = _both_routes(x, codes)
  same(a, b, 'bn_act_quant_codes')
  assert len(torch.unique(a[:-2])) > (1 if rows * C < 100 else 100)       # real codes, not the fill value

  # pooled apply of the head, HW = 7 (this entry kept its scalar form at these channel counts: the vector form lost the measurement)
  if rows % 7 == 0:
    def pool(xv):
      out = _nan((rows // 7, C), dtype)
      hip.bn_act_quant_pool(xv, out, rows, C, 7, ss, ACT, slot[0], 8, True)
      return out
    same(*_both_routes(x, pool), 'bn_act_quant_pool')


def _stats_plan(rows, C):
  """(n_blocks, depth): the row splits the graph gives the passes, and the longest chain of float32 additions behind one value of
  partial[split][stat][c] -- ceil(rows / (n_blocks * RL)) rows in a lane (RL = 1024 / CG row lanes, CG = bn_cg_of(C) groups per slab),
  log2(64 / CG) butterfly steps inside the wavefront, then the 16 wavefronts one after the other through LDS.  The n_blocks splits are
  folded in the tests, in float64."""
  from pocketflow_amd import graph
  G = C // 8
  CG = 8 if G >= 8 else (G if G <= 2 else (4 if G <= 4 else 8))
  RL = 1024 // CG
  n_blocks = graph._bn_blocks(rows, C)
  return n_blocks, -(-rows // (n_blocks * RL)) + int(np.log2(64 // CG)) + 15


def _check_sums(got, terms, depth, what):
  want = terms.sum(0)
  bound = 2.0 ** -24 * depth * terms.abs().sum(0)
  worst = float(((got - want).abs() / bound.clamp_min(1e-300)).max())
  print('%s: depth %d, worst error / bound %.3f' % (what, depth, worst))
  assert bool(((got - want).abs() <= bound).all()), (what, depth, worst)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('rows,C', SHAPES)
def test_bn_stats_against_float64_sums(hip, data, rows, C, dtype):
  x = data(rows, C, dtype)['x']
  n_blocks, depth = _stats_plan(rows, C)
  partial = _nan((n_blocks, 4, C), torch.float32)
  hip.bn_stats(x, rows, C, partial, n_blocks)
  assert not torch.isnan(partial).any()
  xf = x.float()
  dlt = (xf - xf[0]).double()                              # the kernel's terms: float32(x - row 0), exactly
  _check_sums(partial[:, 0].double().sum(0), dlt, depth, 'sum')
  _check_sums(partial[:, 1].double().sum(0), dlt * dlt, depth, 'sum of squares')
  assert torch.equal(partial[:, 2].min(0).values, xf.min(0).values)
  assert torch.equal(partial[:, 3].max(0).values, xf.max(0).values)
  again = _nan((n_blocks, 4, C), torch.float32)
  hip.bn_stats(x, rows, C, again, n_blocks)
  assert torch.equal(again, partial)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('rows,C', SHAPES)
def test_bn_bwd_stats_against_float64_sums(hip, data, rows, C, dtype):
  d = data(rows, C, dtype)
  x, dq, ss, mi = d['x'], d['dq'], d['ss'], d['mi']
  n_blocks, depth = _stats_plan(rows, C)
  partial = _nan((n_blocks, 2, C), torch.float32)
  hip.bn_bwd_stats(dq, x, rows, C, ss, mi, ACT, partial, n_blocks)
  assert not torch.isnan(partial).any()
  xf = x.float()
  u = (ss[0].double() * xf.double() + ss[1].double()).float()          # fmaf(scale, x, shift): the product is exact in float64
  dy = dq.float() * ((u > 0) & (u < 6)).float()                        # dq or 0, exact
  xhat = (xf - mi[0]) * mi[1]                                          # float32, rounded twice as in the kernel
  _check_sums(partial[:, 0].double().sum(0), dy.double(), depth, 'sum dy')
  _check_sums(partial[:, 1].double().sum(0), dy.double() * xhat.double(), depth, 'sum dy * xhat')
  again = _nan((n_blocks, 2, C), torch.float32)
  hip.bn_bwd_stats(dq, x, rows, C, ss, mi, ACT, again, n_blocks)
  assert torch.equal(again, partial)


@pytest.mark.parametrize('rows,C', [(3137, 96), (65, 960)])
@pytest.mark.parametrize('act,bits', [('Relu', 8), ('Relu6', 4), ('Relu', None)])
def test_bn_act_quant_forward_backward_odd_channels(hip, rows, C, act, bits):
  """tests/test_kernels_gpu.py::test_bn_act_quant_forward_backward, body and tolerances, at 12 and 120 groups of channels."""
  from pocketflow_amd.graph import BatchNormAct, Graph
  rng = np.random.RandomState(rows + C)
  x = (rng.randn(rows, C) * 2 + rng.randn(C) * 3).astype(np.float32)
  gamma = (rng.rand(C) + 0.5).astype(np.float32) * np.where(rng.rand(C) > 0.8, -1, 1).astype(np.float32)
  beta = rng.randn(C).astype(np.float32)
  g = Graph('model', 'cuda', torch.float32)
  layer = BatchNormAct(g, 'bn', C, act, 0.997, 1e-5)
  g.finalize()
  g.store.load_numpy({'model/bn/gamma': gamma, 'model/bn/beta': beta}, strict=False)
  layer.op.bits = bits
  g.begin_step()
  g.training = True
  xd = dev(x).view(rows, C, 1, 1).requires_grad_(True)
  q = layer(xd)
  # oracle
  y, mm, mv, (mean, inv_std) = O.batch_norm_train(x, gamma, beta, np.zeros(C), np.ones(C), 0.997, 1e-5)
  t = O.ACTIVATIONS[act](y)
  # un-quantised output of the same kernels (second graph, no fake-quant behind the activation)
  g2 = Graph('model', 'cuda', torch.float32)
  l2 = BatchNormAct(g2, 'bn', C, act, 0.997, 1e-5); g2.finalize()
  g2.store.load_numpy({'model/bn/gamma': gamma, 'model/bn/beta': beta}, strict=False)
  g2.begin_step(); g2.training = True
  y_gpu = l2(dev(x).view(rows, C, 1, 1)).detach().view(rows, C)
  # BN statistics are reduction-order dependent: 2e-5 absolute on O(1) values
  np.testing.assert_allclose(y_gpu.cpu().numpy(), t, rtol=1e-4, atol=2e-5)
  if bits is None:
    assert torch.equal(q.detach().view(rows, C), y_gpu)
  else:
    # the activation range is the exact whole-tensor min/max of what the kernel itself produced
    ab = g.act_alpha_beta().cpu().numpy()[0]
    mn, mx = y_gpu.min().item(), y_gpu.max().item()
    assert ab[1] == np.float32(mn) and ab[0] == np.float32(np.float32(mx) - np.float32(mn)) + np.float32(1e-10)
    ref_q, _ = O.uniform_quantize(y_gpu.cpu().numpy(), bits, mode='activation')
    np.testing.assert_array_equal(q.detach().view(rows, C).cpu().numpy(), ref_q)
  np.testing.assert_allclose(layer.moving_mean.tensor.cpu().numpy(), mm, rtol=1e-4, atol=1e-6)
  np.testing.assert_allclose(layer.moving_var.tensor.cpu().numpy(), mv, rtol=1e-4, atol=1e-6)
  # backward
  dq = rng.randn(rows, C).astype(np.float32)
  q.backward(dev(dq).view(rows, C, 1, 1))
  # ReLU mask from the GPU's own pre-activation sign (elements with |y| ~ 1e-7 may differ from fp64)
  yg = y_gpu.cpu().numpy()
  dy = dq * ((yg > 0) if act == 'Relu' else ((yg > 0) & (yg < 6))).astype(np.float32)
  dx_ref, dg_ref, db_ref = O.batch_norm_train_bwd(dy, x, gamma, mean, inv_std)
  scale = np.abs(dx_ref).max()
  np.testing.assert_allclose(xd.grad.view(rows, C).cpu().numpy(), dx_ref, rtol=1e-3, atol=1e-4 * scale)
  np.testing.assert_allclose(layer.gamma.tensor.grad.cpu().numpy(), dg_ref, rtol=1e-3, atol=1e-3 * np.abs(dg_ref).max())
  np.testing.assert_allclose(layer.beta.tensor.grad.cpu().numpy(), db_ref, rtol=1e-3, atol=1e-3 * np.abs(db_ref).max())
