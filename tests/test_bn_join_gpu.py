"""pf_bn_join.hip on the GPU: pf_bn_add_act_fwd / pf_bn_add_act_bwd_gate[_add] / pf_bn_add_act_groups, kernel by kernel.

Shapes (rows x C): one row; a ragged few rows of one channel group; C = 24 (three groups: lanes idle in every workgroup); 56^2 + 1
rows of 256 channels (a ragged last tile, several slabs); 2048 channels (32 slabs); and the smallest row count at which the
grid-stride loop makes a second trip, read from pf_bn_add_act_groups (C = 64: one full slab; 2 MB in float32).
Inputs: seeded normal x and r, scale in [0.5, 2], shift in [-1, 1]: about half of u = relu(scale * x + shift + r) is positive.

float32 forward: bit-identical to the unfused route of existing kernels (pf_bn_act_quant_apply without activation or quantiser,
torch add, torch relu -- the same three float32 operations), and the decoded slot is exactly (min, max) of the stored tensor.
bf16 forward: against float64 rounded once to bf16, every element within one bf16 ulp; the share of elements off by that ulp no
larger than the share the same comparison shows for pf_bn_act_quant_apply (same x, scale, shift, activation; r = 0) -- that run
is the bar.  Backward: g bit-exact against the float64 gate outside |u| < 1e-6 max|u| (at most 0.1 % of the elements, checked on
the CPU for these seeds by test_gate_exclusion_stays_under_its_cap), dx / dgamma / dbeta against float64 with the tolerances of the
existing pf_bn_bwd_* tests (tests/test_kernels_gpu.py float32: rtol 1e-3, atol 1e-4 / 1e-3 of the largest value; tests/
test_zz_search_gpu.py bf16: 3e-2 of the largest value)."""
import numpy as np
import pytest
import torch

FIXED = [(1, 8), (37, 8), (130, 24), (3137, 256), (196, 2048)]
STRIDE_C = 64                                  # the grid-stride case: channels; its rows come from pf_bn_add_act_groups
DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16}
# float32: all six shapes; bf16: the first four and the grid-stride one
CASES = [('f32', i) for i in range(6)] + [('bf16', i) for i in (0, 1, 2, 3, 5)]


def grid_stride_rows(groups, C):
  """Smallest row count at which a workgroup makes a second trip: the launcher gives every row split one trip of
  256 / min(C / 8, 8) rows until pf_bn_add_act_groups stops growing (include/pocketflow_hip.h)."""
  per_trip = 256 // min(C // 8, 8)
  cap = groups(1 << 40, C)
  assert groups(cap * per_trip, C) == cap and groups((cap - 1) * per_trip, C) == cap - 1 and groups(cap * per_trip + 1, C) == cap
  return cap * per_trip + 1


def shape_of(index, groups):
  return FIXED[index] if index < len(FIXED) else (grid_stride_rows(groups, STRIDE_C), STRIDE_C)


def make_inputs(index, rows, C, dtype):
  """Host tensors, x / r / dq already rounded to `dtype`; scale_shift and mean_invstd float32 [2][C]."""
  gen = torch.Generator(device='cpu').manual_seed(4100 + index)
  x = torch.randn(rows, C, generator=gen).to(dtype)
  r = torch.randn(rows, C, generator=gen).to(dtype)
  dq = torch.randn(rows, C, generator=gen).to(dtype)
  ss = torch.stack([0.5 + 1.5 * torch.rand(C, generator=gen), 2.0 * torch.rand(C, generator=gen) - 1.0]).float().contiguous()
  mi = torch.stack([0.3 * torch.randn(C, generator=gen), 0.5 + torch.rand(C, generator=gen)]).float().contiguous()
  return x, r, dq, ss, mi


def u64_of(x, r, ss):
  return ss[0].double() * x.double() + ss[1].double() + r.double()


def excluded(u64):
  return u64.abs() < 1e-6 * u64.abs().max()


def _reference_groups(rows, C):
  """Mirror of pf_bn_add_act_groups for the CPU-side check below (no library call)."""
  per_trip = 256 // min(C // 8, 8)
  nslab = -(-(C // 8) // min(C // 8, 8))
  return min(-(-rows // per_trip), max(1, min(256, 2048 // nslab)))


def test_gate_exclusion_stays_under_its_cap():
  """CPU, float64 alone: with these seeds at most 0.1 % of the elements have |u| < 1e-6 max|u| (in fact none or a handful), and
  about half of u is positive."""
  for dt, index in CASES:
    rows, C = shape_of(index, _reference_groups)
    x, r, _, ss, _ = make_inputs(index, rows, C, DTYPES[dt])
    u = u64_of(x, r, ss)
    share = float(excluded(u).double().mean())
    assert share <= 1e-3, (dt, rows, C, share)
    if rows * C >= 1000:
      assert 0.4 < float((u > 0).double().mean()) < 0.6


def _ulp_distance_bf16(a, b):
  """Distance in bf16 steps between two bf16 tensors of finite values (sign-magnitude patterns mapped to a line)."""
  def line(t):
    v = t.view(torch.int16).int()
    return torch.where(v < 0, -(v & 0x7FFF), v)
  return (line(a) - line(b)).abs()


@pytest.mark.gpu
@pytest.mark.parametrize('dt,index', CASES)
def test_forward(dt, index):
  from pocketflow_amd import hip
  dtype = DTYPES[dt]
  rows, C = shape_of(index, hip.bn_add_act_groups)
  assert rows * C * 4 < 64 << 20
  x, r, _, ss, _ = make_inputs(index, rows, C, dtype)
  xd, rd, ssd = x.cuda(), r.cuda(), ss.cuda()
  slot = torch.zeros(2, dtype=torch.int32, device='cuda')
  hip.minmax_slots_init(slot)
  u = torch.full((rows, C), float('nan'), dtype=dtype, device='cuda')
  hip.bn_add_act_fwd(xd, rd, u, rows, C, ssd, 'Relu', slot)
  plain = torch.full((rows, C), float('nan'), dtype=dtype, device='cuda')
  hip.bn_add_act_fwd(xd, rd, plain, rows, C, ssd, 'Relu', None)
  assert torch.equal(u, plain) and not bool(torch.isnan(u.float()).any())
  ab = hip.minmax_decode(slot).cpu()
  mn, mx = u.float().min().cpu(), u.float().max().cpu()
  assert float(ab[0, 1]) == float(mn) and float(ab[0, 0]) == float((mx - mn) + torch.tensor(1e-10))
  # no activation: the plain sum
  lin = torch.full((rows, C), float('nan'), dtype=dtype, device='cuda')
  hip.bn_add_act_fwd(xd, rd, lin, rows, C, ssd, None, None)
  assert torch.equal(torch.relu(lin), u)
  if dtype == torch.float32:
    y = torch.empty_like(xd)
    hip.bn_act_quant_apply(xd, y, rows, C, ssd, None, None, 8, False)
    unfused = torch.relu(y + rd)
    assert torch.equal(u.view(torch.int32), unfused.view(torch.int32)), (rows, C)
    assert torch.equal(lin.view(torch.int32), (y + rd).view(torch.int32)), (rows, C)
    return
  ref = _round_f64_to_bf16(torch.relu(u64_of(x, r, ss)))
  d = _ulp_distance_bf16(u.cpu(), ref)
  share = float((d != 0).double().mean())
  # the bar: the existing BN apply pass against ITS float64 reference
  bar_out = torch.empty_like(xd)
  hip.bn_act_quant_apply(xd, bar_out, rows, C, ssd, 'Relu', None, 8, False)
  bar_ref = _round_f64_to_bf16(torch.relu(u64_of(x, torch.zeros_like(x), ss)))
  bar_d = _ulp_distance_bf16(bar_out.cpu(), bar_ref)
  bar = float((bar_d != 0).double().mean())
  print('bn_join_parity %5d x %-4d bf16: join off by one ulp %.3e (%d of %d) | pf_bn_act_quant_apply, r = 0: %.3e (%d)'
        % (rows, C, share, int((d != 0).sum()), d.numel(), bar, int((bar_d != 0).sum())))
  assert int(d.max()) <= 1 and int(bar_d.max()) <= 1, (rows, C)
  assert share <= bar, (rows, C, share, bar)


def _round_f64_to_bf16(v):
  """ONE rounding (nearest, ties to even) of float64 values to bf16, on the bit pattern of the double."""
  bits = v.contiguous().view(torch.int64)
  drop = 52 - 7                                   # mantissa bits a bf16 does not keep
  half, odd = (1 << (drop - 1)) - 1, (bits >> drop) & 1
  kept = ((bits + half + odd) >> drop) << drop
  out = kept.view(torch.float64).float()          # exact: 8 significant bits, and the values are far from float32's range limits
  out = torch.where(v == 0, torch.zeros_like(out), out)
  return out.to(torch.bfloat16)


@pytest.mark.gpu
@pytest.mark.parametrize('dt,index', CASES)
def test_backward_gate_and_bn_backward(dt, index):
  from pocketflow_amd import hip
  dtype = DTYPES[dt]
  rows, C = shape_of(index, hip.bn_add_act_groups)
  x, r, dq, ss, mi = make_inputs(index, rows, C, dtype)
  xd, rd, dqd, ssd, mid = x.cuda(), r.cuda(), dq.cuda(), ss.cuda(), mi.cuda()
  nblk = hip.bn_add_act_groups(rows, C)
  assert nblk >= 1
  partial = torch.full((nblk, 2, C), float('nan'), device='cuda')
  g = torch.full((rows, C), float('nan'), dtype=dtype, device='cuda')
  hip.bn_add_act_bwd_gate(dqd, xd, rd, g, rows, C, ssd, mid, 'Relu', partial)
  assert not bool(torch.isnan(partial).any()) and not bool(torch.isnan(g.float()).any())
  u = u64_of(x, r, ss)
  ex = excluded(u)
  assert float(ex.double().mean()) <= 1e-3
  g_ref = (dq.double() * (u > 0)).to(dtype)
  gc = g.cpu()
  assert torch.equal(gc[~ex], g_ref[~ex]), (rows, C)
  assert bool(((gc[ex] == 0) | (gc[ex] == dq[ex])).all())
  # the BN backward on g through the existing kernels, against float64 on the kernel's own g
  dgamma, dbeta = torch.empty(C, device='cuda'), torch.empty(C, device='cuda')
  hip.bn_bwd_finalize(partial, nblk, C, dgamma, dbeta)
  dx = torch.full((rows, C), float('nan'), dtype=dtype, device='cuda')
  hip.bn_bwd_apply(g, xd, dx, rows, C, ssd, mid, dgamma, dbeta, None)
  g64, xh = gc.double(), (x.double() - mi[0].double()) * mi[1].double()
  db_ref, dg_ref = g64.sum(0), (g64 * xh).sum(0)
  dx_ref = ss[0].double() * (g64 - db_ref / rows - xh * dg_ref / rows)
  got = dict(dx=dx.cpu().double(), dgamma=dgamma.cpu().double(), dbeta=dbeta.cpu().double())
  want = dict(dx=dx_ref, dgamma=dg_ref, dbeta=db_ref)
  for k in ('dx', 'dgamma', 'dbeta'):
    scale = float(want[k].abs().max())
    if dtype == torch.float32:
      atol = (1e-4 if k == 'dx' else 1e-3) * scale
      np.testing.assert_allclose(got[k].numpy(), want[k].numpy(), rtol=1e-3, atol=atol, err_msg='%s %d x %d' % (k, rows, C))
    else:
      assert float((got[k] - want[k]).abs().max()) <= 3e-2 * max(1.0, scale), (k, rows, C)
  # two consumers: dq + addend, rounded to the storage type as autograd's accumulation stores it, then the same gate
  a = torch.randn(rows, C, generator=torch.Generator().manual_seed(9 + index)).to(dtype)
  g2 = torch.full((rows, C), float('nan'), dtype=dtype, device='cuda')
  p2 = torch.full((nblk, 2, C), float('nan'), device='cuda')
  hip.bn_add_act_bwd_gate(dqd, xd, rd, g2, rows, C, ssd, mid, 'Relu', p2, addend=a.cuda())
  gs = torch.full((rows, C), float('nan'), dtype=dtype, device='cuda')
  ps = torch.full((nblk, 2, C), float('nan'), device='cuda')
  hip.bn_add_act_bwd_gate(dqd + a.cuda(), xd, rd, gs, rows, C, ssd, mid, 'Relu', ps)
  assert torch.equal(g2, gs) and torch.equal(p2, ps)
  # no activation: g = dq
  g3 = torch.full((rows, C), float('nan'), dtype=dtype, device='cuda')
  hip.bn_add_act_bwd_gate(dqd, xd, rd, g3, rows, C, ssd, mid, None, p2)
  assert torch.equal(g3, dqd)


@pytest.mark.gpu
def test_bad_arguments_are_refused_without_a_launch():
  """Every documented hipErrorInvalidValue case, with valid device buffers behind the call; the output keeps its NaN fill."""
  from pocketflow_amd import hip
  rows, C = 16, 16
  buf = lambda: torch.zeros(rows * C + 8, dtype=torch.float32, device='cuda')
  x, r, dq = buf(), buf(), buf()
  ss, mi = torch.ones(2, C, device='cuda'), torch.ones(2, C, device='cuda')
  partial = torch.full((4, 2, C), float('nan'), device='cuda')
  out = torch.full((rows * C + 8,), float('nan'), device='cuda')
  slot = torch.zeros(2, dtype=torch.int32, device='cuda')
  hip.minmax_slots_init(slot)
  slot0 = slot.clone()
  lib, P, S = hip._lib, hip._ptr, hip._stream
  from ctypes import c_int, c_int64
  INVALID = 1                                     # hipErrorInvalidValue

  def fwd(x=x, r=r, u=out, dtype=0, rows=rows, C=C, ss=ss, act=1):
    return lib.pf_bn_add_act_fwd(P(x), P(r), P(u), c_int(dtype), c_int64(rows), c_int(C), P(ss), c_int(act), P(slot), S())

  def gate(dq=dq, x=x, r=r, g=out, dtype=0, rows=rows, C=C, ss=ss, mi=mi, act=1, partial=partial):
    return lib.pf_bn_add_act_bwd_gate(P(dq), P(x), P(r), P(g), c_int(dtype), c_int64(rows), c_int(C), P(ss), P(mi), c_int(act),
                                      P(partial), S())

  def gate_add(addend):
    return lib.pf_bn_add_act_bwd_gate_add(P(dq), P(addend), P(x), P(r), P(out), c_int(0), c_int64(rows), c_int(C), P(ss), P(mi),
                                          c_int(1), P(partial), S())
  off = lambda t: t[1:]                           # 4 bytes past a 16-byte boundary
  bad = [fwd(x=None), fwd(r=None), fwd(u=None), fwd(ss=None), fwd(x=off(x)), fwd(r=off(r)), fwd(u=off(out)), fwd(C=12), fwd(C=0),
         fwd(rows=0), fwd(rows=-3), fwd(act=2), fwd(act=7), fwd(dtype=5),
         gate(dq=None), gate(x=None), gate(r=None), gate(g=None), gate(ss=None), gate(mi=None), gate(partial=None),
         gate(dq=off(dq)), gate(x=off(x)), gate(r=off(r)), gate(g=off(out)), gate(C=12), gate(rows=0), gate(act=2), gate(dtype=5),
         gate_add(off(dq))]
  torch.cuda.synchronize()
  assert all(e == INVALID for e in bad), bad
  assert bool(torch.isnan(out).all()) and bool(torch.isnan(partial).all()) and torch.equal(slot, slot0)
  assert hip.bn_add_act_groups(0, 16) == 0 and hip.bn_add_act_groups(16, 12) == 0 and hip.bn_add_act_groups(16, 16) == 1
  # and the same buffers are accepted when nothing is wrong
  assert fwd() == 0 and gate() == 0 and gate_add(None) == 0
  torch.cuda.synchronize()
  assert not bool(torch.isnan(out[:rows * C]).any())
