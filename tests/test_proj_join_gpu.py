"""The joined backward-data of a projection block (pf_conv1x1_bwd_data_join): conv1's backward-data reads the strided shortcut's
COMPACT input gradient through the inverse row map (part 1) and takes bn1's BN-backward sums from the joined gradient in the same
launch (part 2).

Part 1 changes no bit: the compact residual lands on the fp32 accumulators exactly where the zero-filled full-size tensor held it,
and +0.0f everywhere else.  It is therefore compared with `torch.equal` against today's formulation through the existing entries.
Part 2 changes the summation order of the sums only: same bound as tests/test_conv_gpu.py applies to the single-consumer form."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hip():
  from pocketflow_amd import hip as h
  return h


def _bf(x):
  return x.to(torch.bfloat16)


# (B, H, W, N, K, stride, plan): dY [B*H*W][N], dQ [B*H*W][K]; the shortcut has 4 N output channels.  `plan` is the kernel
# pf_conv1x1_join_plan names for the shape (pf_conv.hip: the resident kernel takes M >= 4096 with N, K <= 512 and K * N <= 32 Ki per
# slice; otherwise the staged GEMM from a contraction of 256 channels up): 1 = k_conv1x1_stream, 2 = k_igemm
_STRIDED = [
    (2, 48, 48, 128, 256, 2, 1),     # resident kernel, NW = 256 (one 16-row strip per pass; M = 4608 = 288 strips)
    (2, 48, 48, 64, 64, 2, 1),       # resident kernel, NW = 64 (32-row strips)
    (2, 47, 49, 64, 64, 2, 1),       # ... odd sizes, M = 4606: the last strip is partial
    (2, 14, 14, 256, 512, 2, 2),     # staged kernel 128 x 128, M = 392: the last row tile is partial
    (3, 7, 9, 512, 1024, 2, 2),      # staged kernel, odd sizes: Ho = 4, Wo = 5
    (2, 14, 14, 256, 192, 2, 2),     # staged kernel 128 x 64 (K % 128 != 0)
    (1, 15, 15, 256, 128, 3, 2),     # stride 3
]
_DENSE = [
    (2, 48, 48, 64, 64, 1, 1),       # resident kernel, NW = 64: stage 1's projection
    (2, 48, 48, 128, 256, 1, 1),     # resident kernel, NW = 256
    (3, 7, 9, 512, 1024, 1, 2),      # staged kernel 128 x 128
    (2, 14, 14, 256, 192, 1, 2),     # staged kernel 128 x 64
]


def _case(B, H, W, N, K, stride, seed=11):
  """Inputs built as in tests/test_conv_gpu.py::test_conv1x1_bwd_data_with_bn_backward_statistics, plus the shortcut's operands."""
  g = torch.Generator(device='cuda').manual_seed(seed)
  M = B * H * W
  Ho, Wo = -(-H // stride), -(-W // stride)
  Mc, Ns = B * Ho * Wo, 4 * N
  c = dict(M=M, Mc=Mc, Ns=Ns, geom=(Ho, Wo, H, W, stride))
  c['dY'] = _bf(torch.randn(M, N, device='cuda', generator=g) * 0.1)
  Wk = _bf(torch.randn(N, K, device='cuda', generator=g) * 0.1)
  c['Wt'] = Wk.t().contiguous()
  c['x'] = _bf(torch.randn(M, K, device='cuda', generator=g))
  c['ss'] = torch.stack([torch.rand(K, device='cuda', generator=g) + 0.5, torch.randn(K, device='cuda', generator=g) * 0.3])
  c['mi'] = torch.stack([torch.randn(K, device='cuda', generator=g) * 0.1, torch.rand(K, device='cuda', generator=g) + 0.5])
  c['dYs'] = _bf(torch.randn(Mc, Ns, device='cuda', generator=g) * 0.1)
  c['Wts'] = _bf(torch.randn(Ns, K, device='cuda', generator=g) * 0.1).t().contiguous()
  return c


def _today(hip, c, N, K, stride):
  """(full-size shortcut gradient, dQ) of today's formulation through the existing entries."""
  M, Mc, Ns = c['M'], c['Mc'], c['Ns']
  if stride == 1:
    full = torch.empty(M, K, device='cuda', dtype=torch.bfloat16)
    hip.conv1x1_fwd(c['dYs'], c['Wts'], full, M, K, Ns)
  else:
    B = M // (c['geom'][2] * c['geom'][3])
    full = torch.zeros(B, K, c['geom'][2], c['geom'][3], device='cuda', dtype=torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    hip.conv1x1_fwd(c['dYs'], c['Wts'], full, Mc, K, Ns, geom=c['geom'], ymap=True)
    full = full.permute(0, 2, 3, 1).reshape(M, K)
  dQ = torch.empty(M, K, device='cuda', dtype=torch.bfloat16)
  hip.conv1x1_fwd(c['dY'], c['Wt'], dQ, M, K, N, R=full)
  return full, dQ


def _compact(hip, c, K):
  Rc = torch.empty(c['Mc'], K, device='cuda', dtype=torch.bfloat16)
  hip.conv1x1_fwd(c['dYs'], c['Wts'], Rc, c['Mc'], K, c['Ns'])
  return Rc


def _partner_mask(B, H, W, stride):
  m = torch.zeros(B, H, W, dtype=torch.bool, device='cuda')
  m[:, ::stride, ::stride] = True
  return m.reshape(-1)


@pytest.mark.parametrize('B,H,W,N,K,stride,plan', _STRIDED + _DENSE)
def test_join_with_a_compact_residual_changes_no_bit(hip, B, H, W, N, K, stride, plan):
  c = _case(B, H, W, N, K, stride)
  M = c['M']
  assert hip.conv1x1_join_plan(M, N, K, False) == plan
  full, ref = _today(hip, c, N, K, stride)
  dQ = torch.full((M, K), float('nan'), device='cuda', dtype=torch.bfloat16)
  if stride == 1:
    hip.conv1x1_bwd_data_join(c['dY'], c['Wt'], dQ, full, M, N, K)
    assert torch.equal(dQ, ref)
    return
  Rc = _compact(hip, c, K)
  mask = _partner_mask(B, H, W, stride)
  # the plain dense GEMM leaves the values the row-scatter launch wrote (same kernel family, same accumulation order)
  assert torch.equal(full[mask], Rc) and not bool(full[~mask].any())
  hip.conv1x1_bwd_data_join(c['dY'], c['Wt'], dQ, Rc, M, N, K, rgeom=c['geom'])
  assert torch.equal(dQ, ref)
  # rows without a partner: the launch without a residual (the residual there is exactly +0.0f)
  plain = torch.empty_like(dQ)
  hip.conv1x1_fwd(c['dY'], c['Wt'], plain, M, K, N)
  assert torch.equal(dQ[~mask], plain[~mask])
  assert not torch.equal(dQ[mask], plain[mask])


@pytest.mark.parametrize('B,H,W,N,K,stride,plan', _STRIDED + _DENSE)
def test_join_with_bn_backward_sums(hip, B, H, W, N, K, stride, plan):
  """dQ of the launch with sums == the launch without; the finalized sums == pf_bn_bwd_stats + pf_bn_bwd_finalize on (dQ, x)."""
  c = _case(B, H, W, N, K, stride, seed=13)
  M = c['M']
  assert hip.conv1x1_join_plan(M, N, K, False) == plan
  if stride == 1:
    R, rgeom = _today(hip, c, N, K, stride)[0], None
  else:
    R, rgeom = _compact(hip, c, K), c['geom']
  ref = torch.empty(M, K, device='cuda', dtype=torch.bfloat16)
  hip.conv1x1_bwd_data_join(c['dY'], c['Wt'], ref, R, M, N, K, rgeom=rgeom)
  G = hip.conv1x1_stats_groups(M, K, N)
  partial = torch.full((G, 2, K), float('nan'), device='cuda')
  dQ = torch.full((M, K), float('nan'), device='cuda', dtype=torch.bfloat16)
  hip.conv1x1_bwd_data_join(c['dY'], c['Wt'], dQ, R, M, N, K, rgeom=rgeom, bn_x=c['x'], bn_scale_shift=c['ss'],
                            bn_mean_invstd=c['mi'], bn_act='Relu', partial=partial)
  assert torch.equal(dQ, ref)
  assert not torch.isnan(partial).any()
  nblk = 32
  ref_partial = torch.empty(nblk * 2 * K, device='cuda')
  hip.bn_bwd_stats(dQ, c['x'], M, K, c['ss'], c['mi'], 'Relu', ref_partial, nblk)
  dgamma, dbeta = torch.empty(K, device='cuda'), torch.empty(K, device='cuda')
  hip.bn_bwd_finalize(ref_partial, nblk, K, dgamma, dbeta)
  dg2, db2 = torch.empty(K, device='cuda'), torch.empty(K, device='cuda')
  hip.bn_bwd_finalize(partial, G, K, dg2, db2)
  print('max |dbeta diff| %.3e  max |dgamma diff| %.3e' % (float((db2 - dbeta).abs().max()), float((dg2 - dgamma).abs().max())))
  torch.testing.assert_close(db2, dbeta, rtol=1e-4, atol=1e-3)
  torch.testing.assert_close(dg2, dgamma, rtol=1e-4, atol=1e-3)


def test_plan_asks_for_the_sums_only_where_they_pay(hip):
  """The flagship's four projection blocks at batch 256: the resident kernel and the staged GEMM of stage 3 take the sums, stage 4
  (14 x 14: six tiles per workgroup) keeps the separate pass -- the compact residual is taken everywhere."""
  for M, N, K, plan, stats in [(256 * 56 * 56, 64, 64, 1, 1), (256 * 56 * 56, 128, 256, 1, 1), (256 * 28 * 28, 256, 512, 2, 2),
                               (256 * 14 * 14, 512, 1024, 2, 0)]:
    assert hip.conv1x1_join_plan(M, N, K, False) == plan and hip.conv1x1_join_plan(M, N, K, True) == stats


def test_join_refuses_what_the_plan_refuses(hip):
  """Shapes of the register-staged tiles (a short contraction on few rows) stay on the separate launches: the plan says so and the
  entry returns an error instead of running something else."""
  M, N, K = 392, 64, 64
  assert hip.conv1x1_join_plan(M, N, K, False) == 0 and hip.conv1x1_join_plan(M, N, K, True) == 0
  dY = torch.zeros(M, N, device='cuda', dtype=torch.bfloat16)
  Wt = torch.zeros(K, N, device='cuda', dtype=torch.bfloat16)
  R = torch.zeros(M, K, device='cuda', dtype=torch.bfloat16)
  dQ = torch.empty(M, K, device='cuda', dtype=torch.bfloat16)
  with pytest.raises(RuntimeError):
    hip.conv1x1_bwd_data_join(dY, Wt, dQ, R, M, N, K)
