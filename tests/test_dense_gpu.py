"""The dense kernels (pf_dense.hip) in exact integer arithmetic: operands are small integers stored as bf16 (x and the bias in {-3..3},
the kernel and dy in {-2..2}), so every float32 partial sum of every pass, in any order and any split, is an integer of magnitude
<= 2048 * 6 + 3 < 2**24 and the kernels' results must EQUAL the float64 reference of torch.nn.functional.linear on the CPU, rounded
once to the output's dtype."""
import functools

import pytest
import torch
import torch.nn.functional as F

from wrw_exact import expected, int_inputs, seed_of

pytestmark = pytest.mark.gpu

# (B, K, N): one k-step, one row, one column, no split | ResNet-20's head, N < 16 | row tail, column tail of one, odd pitch, K / 32 = 3 |
# the ragged production width with few rows | B crosses a 256-row block | the ResNet-50 head: the full split counts
CASES = [(1, 32, 1), (3, 64, 10), (17, 96, 17), (20, 256, 1001), (260, 128, 33), (256, 2048, 1001)]
INF, NAN = float('inf'), float('nan')


@functools.lru_cache(maxsize=None)
def _case(B, K, N):
  """Inputs (bf16, CPU) and the float64 results of one shape: computed once, shared by the tests, never written."""
  seed = seed_of('dense', B, K, N)
  dy, x = int_inputs(seed, (B, N), (B, K))
  w, bias = int_inputs(seed + 1, (N, K), (N,))
  xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, bias))
  yr = F.linear(xr, wr, br)
  yr.backward(dy.double())
  return dict(x=x, w=w, bias=bias, dy=dy, y=yr.detach(), dx=xr.grad, dw=wr.grad, db=br.grad)


def _check_layer(g, layer, B, K, N, x, run):
  """One forward + backward of `layer` on the dense route; compares all three passes and db with the reference."""
  from pocketflow_amd import profiling
  c = _case(B, K, N)
  g.begin_step()
  profiling.enable('dense_fwd')
  try:
    with g.as_default():
      y = run(x)
    assert profiling.count('dense_fwd') == 1
  finally:
    profiling.disable_all()
  y.backward(c['dy'].cuda().view(y.shape))
  assert torch.equal(y.detach().cpu().view(B, N), expected(c['y'], torch.bfloat16)), 'forward'
  assert torch.equal(x.grad.cpu().view(B, K), expected(c['dx'], torch.bfloat16)), 'backward-data'
  v = layer.kernel
  gw = g.store.w_grad[v.offset:v.offset + v.numel].view(N, K)
  assert torch.equal(gw.cpu(), expected(c['dw'], gw.dtype)), 'backward-filter'
  assert torch.equal(layer.bias.tensor.grad.cpu(), expected(c['db'], torch.float32)), 'bias gradient'


@pytest.mark.parametrize('B,K,N', CASES)
def test_dense_layer_is_exact(B, K, N, monkeypatch):
  import pocketflow_amd.graph as G
  from pocketflow_amd import hip
  c = _case(B, K, N)
  g = G.Graph('model', 'cuda', torch.bfloat16)
  with g.as_default():
    fc = G.Dense(g, 'fc', K, N)
  g.finalize(seed=11)
  with torch.no_grad():
    fc.kernel.tensor.copy_(c['w'].cuda())
    fc.bias.tensor.copy_(c['bias'].float().cuda())
  if (B, K, N) == (1, 32, 1):
    assert hip.dense_splits(B, K, N) == 1 and hip.dense_splits(B, K, N, True) == 1
  _check_layer(g, fc, B, K, N, c['x'].cuda().requires_grad_(True), fc)
  # the switch off: the same layer does not reach the node
  from pocketflow_amd import profiling
  monkeypatch.setattr(G, 'OWN_DENSE_MFMA', False)
  profiling.enable('dense_fwd')
  profiling.enable('convg_fwd')
  try:
    with g.as_default():
      y = fc(c['x'].cuda().requires_grad_(True))
    assert (profiling.count('dense_fwd'), profiling.count('convg_fwd')) == (0, 1)
  finally:
    profiling.disable_all()
  assert not isinstance(y.grad_fn, G._DenseMfma._backward_cls)
  assert torch.equal(y.detach().cpu(), expected(c['y'], torch.bfloat16))


def test_logits_convolution_takes_the_dense_node():
  """MobileNet's logits: a 1x1 convolution with a bias over 1x1 pixels."""
  import pocketflow_amd.graph as G
  B, K, N = 4, 64, 10
  c = _case(B, K, N)
  g = G.Graph('model', 'cuda', torch.bfloat16)
  with g.as_default():
    conv = G.Conv2D(g, 'logits', K, N, 1, 1, use_bias=True)
  g.finalize(seed=11)
  with torch.no_grad():
    conv.kernel.tensor.copy_(c['w'].cuda().view(N, K, 1, 1))
    conv.bias.tensor.copy_(c['bias'].float().cuda())
  _check_layer(g, conv, B, K, N, c['x'].cuda().view(B, K, 1, 1).requires_grad_(True), conv)


def _mid(pad, dtype, values=None, n=None):
  """(buffer, slice): `values` (or n NaNs) in the middle of a buffer whose remainder, `pad` elements on either side, is +inf."""
  n = values.numel() if values is not None else n
  buf = torch.full((pad + n + pad,), INF, dtype=dtype, device='cuda')
  mid = buf[pad:pad + n]
  mid.copy_(values.flatten()) if values is not None else mid.fill_(NAN)
  return buf, mid


def test_c_abi_on_slices_between_inf_sentinels():
  """Every operand lies between +inf; outputs and workspace start as NaN.  Y / dY start at an ODD element (2-byte alignment only)."""
  from pocketflow_amd import hip
  B, K, N = 17, 96, 17
  c = _case(B, K, N)
  bf, f32 = torch.bfloat16, torch.float32
  _, x = _mid(64, bf, c['x'].cuda())
  _, w = _mid(64, bf, c['w'].cuda())
  _, dy = _mid(65, bf, c['dy'].cuda())
  _, bias = _mid(1, f32, c['bias'].float().cuda())
  sf, sb = hip.dense_splits(B, K, N), hip.dense_splits(B, K, N, True)
  assert sf == 3
  _, ws_f = _mid(64, f32, n=sf * B * N)
  _, ws_b = _mid(64, f32, n=sb * B * K)
  outs = dict(y=_mid(65, bf, n=B * N), dx=_mid(64, bf, n=B * K), dw=_mid(64, f32, n=N * K), db=_mid(1, f32, n=N))
  hip.dense_fwd(x, w, bias, outs['y'][1], B, K, N, ws_f)
  hip.dense_bwd_data(dy, w, outs['dx'][1], B, K, N, ws_b)
  hip.dense_wrw(dy, x, outs['dw'][1], outs['db'][1], B, K, N)
  for name, (buf, mid) in outs.items():
    assert torch.equal(mid.cpu(), expected(c[name], mid.dtype).flatten()), name
    pad = (buf.numel() - mid.numel()) // 2
    assert bool(torch.isposinf(buf[:pad]).all()) and bool(torch.isposinf(buf[pad + mid.numel():]).all()), name + ': sentinels'
