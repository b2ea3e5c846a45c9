"""Every route of the convolution launch plan writes exactly the statistics rows its query names (pf_conv.hip: conv1x1_plan; the
queries and the launches read one decision).

Method: no route may have more than 1024 rows (tests/test_abi_host.py asserts that bound over the whole shape grid), so `partial` is
allocated with 1032: rows below the queried G are filled with NaN, the rows from G up with a finite sentinel.  After the launch no
NaN may remain below G and every row from G up must still be the sentinel, bit for bit -- a launch that disagrees with its query
about G shows up inside the same allocation instead of writing past it."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = 1032
SENTINEL = -12345.5


@pytest.fixture(scope='module')
def hip():
  from pocketflow_amd import hip as h
  return h


def _bf(x):
  return x.to(torch.bfloat16)


def _guarded(G, nstat, N):
  assert 1 <= G <= 1024
  partial = torch.full((ROWS, nstat, N), SENTINEL, device='cuda')
  partial[:G] = float('nan')
  return partial


def _check_guard(partial, G, what):
  torch.cuda.synchronize()
  nan_rows = int(torch.isnan(partial[:G]).flatten(1).any(1).sum())
  touched = int((partial[G:] != SENTINEL).flatten(1).any(1).sum())
  print('%s: G = %d, rows below G still NaN: %d, guard rows touched: %d' % (what, G, nan_rows, touched))
  assert nan_rows == 0, '%s: %d of the %d rows the query names were not written' % (what, nan_rows, G)
  assert torch.equal(partial[G:], torch.full_like(partial[G:], SENTINEL)), '%s: %d rows from G = %d up were written' % (what, touched, G)


def _prologue(K, g):
  return torch.stack([torch.rand(K, device='cuda', generator=g) + 0.5, torch.randn(K, device='cuda', generator=g)])


# tiles: plain, prologue (K % 64 != 0); resident kernel: one slice, two slices; staged GEMM: prologue (128 x 256 and 256 x 128 tiles), plain
@pytest.mark.parametrize('M,N,K,pro', [(1000, 64, 64, False), (3000, 128, 96, True), (4096, 64, 64, False), (6001, 512, 128, False),
                                       (3000, 256, 1024, True), (2600, 128, 2048, True), (3000, 256, 1024, False)])
def test_conv1x1_fwd_writes_the_rows_the_query_names(hip, M, N, K, pro):
  g = torch.Generator(device='cuda').manual_seed(M + N + K)
  X = _bf(torch.randn(M, K, device='cuda', generator=g))
  W = _bf(torch.randn(N, K, device='cuda', generator=g) * 0.1)
  Y = torch.empty(M, N, device='cuda', dtype=torch.bfloat16)
  G = hip.conv1x1_stats_groups(M, N, K, prologue=pro)
  partial = _guarded(G, 4, N)
  hip.conv1x1_fwd(X, W, Y, M, N, K, scale_shift=_prologue(K, g) if pro else None, act='Relu' if pro else None, partial=partial)
  _check_guard(partial, G, 'conv1x1_fwd %s' % ((M, N, K, pro),))


def _bn_operands(M, K, g):
  x = _bf(torch.randn(M, K, device='cuda', generator=g))
  ss = torch.stack([torch.rand(K, device='cuda', generator=g) + 0.5, torch.randn(K, device='cuda', generator=g) * 0.3])
  mi = torch.stack([torch.randn(K, device='cuda', generator=g) * 0.1, torch.rand(K, device='cuda', generator=g) + 0.5])
  return x, ss, mi


@pytest.mark.parametrize('M,N,K', [(4800, 64, 256), (3000, 256, 128)])
def test_conv1x1_bwd_data_bnstats_writes_the_rows_the_query_names(hip, M, N, K):
  g = torch.Generator(device='cuda').manual_seed(11)
  dY = _bf(torch.randn(M, N, device='cuda', generator=g) * 0.1)
  Wt = _bf(torch.randn(K, N, device='cuda', generator=g) * 0.1)
  x, ss, mi = _bn_operands(M, K, g)
  dQ = torch.empty(M, K, device='cuda', dtype=torch.bfloat16)
  G = hip.conv1x1_stats_groups(M, K, N)
  partial = _guarded(G, 2, K)
  hip.conv1x1_bwd_data_bnstats(dY, Wt, dQ, x, ss, mi, 'Relu', partial, M, N, K)
  _check_guard(partial, G, 'conv1x1_bwd_data_bnstats %s' % ((M, N, K),))


# the smallest shape of each plan in tests/test_proj_join_gpu.py's lists: the resident kernel (2 x 47 x 49, 64 -> 64) and the staged
# GEMM (3 x 7 x 9, 512 -> 1024), each with a compact residual behind the inverse row map (stride 2)
@pytest.mark.parametrize('B,H,W,N,K,stride,plan', [(2, 47, 49, 64, 64, 2, 1), (3, 7, 9, 512, 1024, 2, 2)])
def test_conv1x1_bwd_data_join_with_sums_writes_the_rows_the_query_names(hip, B, H, W, N, K, stride, plan):
  g = torch.Generator(device='cuda').manual_seed(13)
  M, Ho, Wo = B * H * W, -(-H // stride), -(-W // stride)
  assert hip.conv1x1_join_plan(M, N, K, False) == plan
  dY = _bf(torch.randn(M, N, device='cuda', generator=g) * 0.1)
  Wt = _bf(torch.randn(K, N, device='cuda', generator=g) * 0.1)
  Rc = _bf(torch.randn(B * Ho * Wo, K, device='cuda', generator=g) * 0.1)
  x, ss, mi = _bn_operands(M, K, g)
  dQ = torch.empty(M, K, device='cuda', dtype=torch.bfloat16)
  G = hip.conv1x1_stats_groups(M, K, N)
  partial = _guarded(G, 2, K)
  hip.conv1x1_bwd_data_join(dY, Wt, dQ, Rc, M, N, K, rgeom=(Ho, Wo, H, W, stride), bn_x=x, bn_scale_shift=ss, bn_mean_invstd=mi,
                            bn_act='Relu', partial=partial)
  _check_guard(partial, G, 'conv1x1_bwd_data_join %s' % ((B, H, W, N, K, stride),))


# 3 x 3 / stride 1 / pad 1: the window-staged kernel (56 x 56, 64 -> 64) and the implicit GEMM
@pytest.mark.parametrize('imgs,H,C,N', [(2, 56, 64, 64), (4, 14, 256, 256)])
def test_conv2d_fwd_writes_the_rows_the_query_names(hip, imgs, H, C, N):
  g = torch.Generator(device='cuda').manual_seed(C)
  x = _bf(torch.randn(imgs, H, H, C, device='cuda', generator=g))
  w = _bf(torch.randn(N, 3, 3, C, device='cuda', generator=g) * 0.05)
  y = torch.empty(imgs, H, H, N, device='cuda', dtype=torch.bfloat16)
  G = hip.conv2d_stats_groups(imgs * H * H, N, geom=(imgs, H, H, C, N, 3, 3, 1, 1, 1, H, H))
  partial = _guarded(G, 4, N)
  hip.conv2d_fwd(x, w, y, imgs, H, H, C, N, 3, 3, 1, 1, 1, H, H, partial=partial)
  _check_guard(partial, G, 'conv2d_fwd %s' % ((imgs, H, C, N),))


def test_limit_case_input_at_the_staged_kernels_addressing_limit(hip):
  """Prologue launch, M = 2^21, N = 128, K = 512, stride 1: X holds exactly 2^30 elements (2 GiB of bf16), the first size the staged
  GEMM's 31-bit byte offsets refuse, so the launch runs on the register-staged tiles with G = 512 -- and the query must say so.
  (Before the plan the query answered 256, the staged GEMM's count for 256 x 128 tiles, and the launch wrote 512 rows.)
  The sum of the statistics is compared with the stored output within the tolerance tests/test_conv_gpu.py uses for the same sum."""
  M, N, K = 2 ** 21, 128, 512
  g = torch.Generator(device='cuda').manual_seed(5)
  X = torch.empty(M, K, device='cuda', dtype=torch.bfloat16)
  X.normal_(generator=g)                                        # in place: no float32 copy of the 2 GiB input
  W = _bf(torch.randn(N, K, device='cuda', generator=g) * (K ** -0.5))
  Y = torch.empty(M, N, device='cuda', dtype=torch.bfloat16)
  G = hip.conv1x1_stats_groups(M, N, K, prologue=True)
  partial = _guarded(G, 4, N)
  hip.conv1x1_fwd(X, W, Y, M, N, K, scale_shift=_prologue(K, g), act='Relu', partial=partial)
  _check_guard(partial, G, 'limit case')
  s, ref = partial[:G, 0].sum(0), Y.float().sum(0)
  print('limit case: max |sum - ref| = %.3e, max |ref| = %.3e' % (float((s - ref).abs().max()), float(ref.abs().max())))
  torch.testing.assert_close(s, ref, rtol=1e-4, atol=1e-2)
