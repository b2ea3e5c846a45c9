"""The pair that never writes conv1's input gradient in an identity bottleneck block: pf_conv1x1_bwd_data_bnsums (the backward-data
launch with BN-backward sums, without its store) and pf_conv1x1_bwd_data_bnapply (the product again, with bn1's backward apply pass
and the shortcut add as its row pass).

The reference is today's route through the existing entries of the same library: conv1x1_bwd_data_bnstats -> bn_bwd_finalize ->
bn_bwd_apply.  Both routes round dq to bf16 once (the stored tensor there, the staged tile here) and run the same per-element
function on it (bn_bwd_dx, pf_common.h), so every comparison is `torch.equal`: there is no tolerance in this file."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_STRIP = 16          # pixel rows per strip of the 256-wide resident kernel (pf_conv_stream.hip: RS at NW = 256)
_WAVES = 8           # wavefronts per workgroup


@pytest.fixture(scope='module')
def hip():
  from pocketflow_amd import hip as h
  return h


def _bf(x):
  return x.to(torch.bfloat16)


# (B, H, W, N, K): dY [B*H*W][N], x / addend / dx [B*H*W][K]
_SHAPES = [
    (2, 48, 48, 64, 256),       # NW = 256, one slice, 288 full strips
    (2, 47, 49, 64, 256),       # M = 4606: the last strip is partial
    (2, 48, 48, 128, 512),      # two column slices
    (2, 47, 49, 128, 512),      # two slices and a partial last strip
    (6, 111, 113, 64, 256),     # M = 75258: wavefronts own two and three strips, the last strip is partial (checked below)
]


def _case(B, H, W, N, K, seed=11):
  """Inputs built as in tests/test_proj_join_gpu.py::_case, plus the shortcut's gradient."""
  g = torch.Generator(device='cuda').manual_seed(seed)
  M = B * H * W
  c = dict(M=M)
  c['dY'] = _bf(torch.randn(M, N, device='cuda', generator=g) * 0.1)
  Wk = _bf(torch.randn(N, K, device='cuda', generator=g) * 0.1)
  c['Wt'] = Wk.t().contiguous()
  c['x'] = _bf(torch.randn(M, K, device='cuda', generator=g))
  c['ss'] = torch.stack([torch.rand(K, device='cuda', generator=g) + 0.5, torch.randn(K, device='cuda', generator=g) * 0.3])
  c['mi'] = torch.stack([torch.randn(K, device='cuda', generator=g) * 0.1, torch.rand(K, device='cuda', generator=g) + 0.5])
  c['addend'] = _bf(torch.randn(M, K, device='cuda', generator=g) * 0.1)
  return c


_REF = {}


def _today(hip, shape, act):
  """Today's route, computed once per (shape, activation) and left unchanged: (case, partial, G, dgamma, dbeta, dx with the addend,
  dx without)."""
  key = shape + (act,)
  if key not in _REF:
    B, H, W, N, K = shape
    c = _case(*shape)
    M = c['M']
    G = hip.conv1x1_stats_groups(M, K, N)
    partial = torch.full((G, 2, K), float('nan'), device='cuda')
    dQ = torch.full((M, K), float('nan'), device='cuda', dtype=torch.bfloat16)
    hip.conv1x1_bwd_data_bnstats(c['dY'], c['Wt'], dQ, c['x'], c['ss'], c['mi'], act, partial, M, N, K)
    dgamma, dbeta = torch.empty(K, device='cuda'), torch.empty(K, device='cuda')
    hip.bn_bwd_finalize(partial, G, K, dgamma, dbeta)
    dx_add, dx = torch.empty_like(dQ), torch.empty_like(dQ)
    hip.bn_bwd_apply(dQ, c['x'], dx_add, M, K, c['ss'], c['mi'], dgamma, dbeta, act, addend=c['addend'])
    hip.bn_bwd_apply(dQ, c['x'], dx, M, K, c['ss'], c['mi'], dgamma, dbeta, act)
    assert not torch.isnan(dx_add.float()).any() and not torch.isnan(dx.float()).any()
    _REF[key] = (c, partial, G, dgamma, dbeta, dx_add, dx)
  return _REF[key]


def test_the_large_case_gives_a_wavefront_two_strips_and_a_partial_last_one(hip):
  B, H, W, N, K = _SHAPES[-1]
  M = B * H * W
  G = hip.conv1x1_stats_groups(M, K, N)            # row-panel sets of the launch = workgroups per column slice
  strips = -(-M // _STRIP)
  assert strips > G * _WAVES and M % _STRIP != 0


@pytest.mark.parametrize('B,H,W,N,K', _SHAPES)
def test_sums_only_launch_leaves_the_partials_of_the_storing_launch(hip, B, H, W, N, K):
  c, ref_partial, G, _, _, _, _ = _today(hip, (B, H, W, N, K), 'Relu')
  M = c['M']
  assert hip.conv1x1_bwd_apply_plan(M, N, K) != 0
  partial = torch.full((G, 2, K), float('nan'), device='cuda')
  hip.conv1x1_bwd_data_bnsums(c['dY'], c['Wt'], c['x'], c['ss'], c['mi'], 'Relu', partial, M, N, K)
  assert torch.equal(partial, ref_partial)


# every shape with ReLU; the ReLU6 instantiation differs in the mask alone: the two odd-sized shapes
@pytest.mark.parametrize('B,H,W,N,K,act', [s + ('Relu',) for s in _SHAPES] + [_SHAPES[1] + ('Relu6',), _SHAPES[3] + ('Relu6',)])
def test_apply_launch_gives_the_bits_of_bn_bwd_apply(hip, B, H, W, N, K, act):
  c, _, _, dgamma, dbeta, ref_add, ref = _today(hip, (B, H, W, N, K), act)
  M = c['M']
  for addend, want in ((c['addend'], ref_add), (None, ref)):
    dx = torch.full((M, K), float('nan'), device='cuda', dtype=torch.bfloat16)
    hip.conv1x1_bwd_data_bnapply(c['dY'], c['Wt'], c['x'], c['ss'], c['mi'], act, dgamma, dbeta, addend, dx, M, N, K)
    same = dx.view(torch.int16) == want.view(torch.int16)
    print('%s addend=%s: %d of %d elements differ' % ((B, H, W, N, K), addend is not None, int((~same).sum()), same.numel()))
    assert torch.equal(dx.view(torch.int16), want.view(torch.int16))
  assert not torch.equal(ref_add, ref)


def _refused(hip, M, N, K, dtype=torch.bfloat16):
  assert hip.conv1x1_bwd_apply_plan(M, N, K, dtype) == 0
  dY = torch.zeros(M, N, device='cuda', dtype=dtype)
  Wt = torch.zeros(K, N, device='cuda', dtype=dtype)
  x = torch.zeros(M, K, device='cuda', dtype=dtype)
  dx = torch.empty(M, K, device='cuda', dtype=dtype)
  ss, mi = torch.ones(2, K, device='cuda'), torch.ones(2, K, device='cuda')
  dg, db = torch.zeros(K, device='cuda'), torch.zeros(K, device='cuda')
  partial = torch.zeros(max(1, hip.conv1x1_stats_groups(M, K, N)), 2, K, device='cuda')
  with pytest.raises(RuntimeError):
    hip.conv1x1_bwd_data_bnsums(dY, Wt, x, ss, mi, 'Relu', partial, M, N, K)
  with pytest.raises(RuntimeError):
    hip.conv1x1_bwd_data_bnapply(dY, Wt, x, ss, mi, 'Relu', dg, db, None, dx, M, N, K)


def test_plan_refuses_a_narrow_output(hip):
  """K < 2 N: the second read of dY eats the saving (64 -> 64 is the resident kernel's shape otherwise)."""
  _refused(hip, 2 * 48 * 48, 64, 64)
  _refused(hip, 2 * 48 * 48, 256, 256)


def test_plan_refuses_shapes_of_other_kernels(hip):
  """Stage 3's conv1 (256 -> 1024 at 14 x 14) runs on the staged GEMM, few rows on the register-staged tiles."""
  _refused(hip, 2 * 14 * 14, 256, 1024)
  _refused(hip, 392, 64, 256)


def test_plan_refuses_float32(hip):
  M, N, K = 2 * 48 * 48, 64, 256
  assert hip.conv1x1_bwd_apply_plan(M, N, K) != 0
  _refused(hip, M, N, K, torch.float32)


def test_plan_takes_the_identity_blocks_of_stages_1_and_2_at_batch_256(hip):
  assert hip.conv1x1_bwd_apply_plan(256 * 56 * 56, 64, 256) != 0 and hip.conv1x1_bwd_apply_plan(256 * 28 * 28, 128, 512) != 0
  assert hip.conv1x1_bwd_apply_plan(256 * 14 * 14, 256, 1024) == 0 and hip.conv1x1_bwd_apply_plan(256 * 7 * 7, 512, 2048) == 0


_CHILD = r'''
import os, sys
sys.path[:0] = [sys.argv[1], os.path.join(sys.argv[1], 'tests')]
from bn1_recompute_child import run
run(sys.argv[2])
'''


def test_uq_learner_reaches_the_same_parameters_on_both_routes(tmp_path):
  """Two seeded steps of the UQ learner on a small ResNet-v2 bottleneck model with PF_BN1_RECOMPUTE=0 and =1, each in a fresh child
  process: every parameter is `torch.equal` afterwards, and the new route did run on the second (its launch counter says so)."""
  out = {}
  for flag in ('0', '1'):
    path = str(tmp_path / ('params_%s.pt' % flag))
    env = dict(os.environ, PF_BN1_RECOMPUTE=flag, PYTHONPATH=_ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-c', _CHILD, _ROOT, path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out[flag] = torch.load(path)
  assert out['0']['launches'] == 0 and out['1']['launches'] > 0, (out['0']['launches'], out['1']['launches'])
  a, b = out['0']['params'], out['1']['params']
  assert a.keys() == b.keys() and len(a) > 0
  for k in a:
    assert torch.equal(a[k], b[k]), k
