"""Bit-exact checks of the backward-filter kernels (pf_wrw.hip, pf_conv.hip, pf_wrw3x3_c64.hip): inputs, reference, guarded
workspace, and the launchers' published rules.  A helper module -- no conftest, nothing here is collected.

THE EXACTNESS CONDITION.  The operands are small INTEGERS stored as bf16 (exact), the MFMA products and every accumulator of
the kernels and of the slab fold are float32.  dW[n][tap][c] = sum over the M output pixels of dy * x; with |x| <= X_MAX = 3 and
|dy| <= DY_MAX = 2 every partial sum of every summation order is an integer of magnitude <= 6 * M.  float32 represents every
integer below 2**24, so as long as

    6 * M < 2**24        (in general  2 * x_bound * M < 2**24,  x_bound the largest |x| after a prologue)

no addition ever rounds, whatever the tile, the split, the wavefront order or the fold: the kernel's float32 result must EQUAL the
integer reference bit for bit, and its bf16 result must equal the round-to-nearest-even of it.  `assert_exact_regime` checks the
condition per case, so that a case edited later cannot silently leave the regime.
"""
import collections
import zlib

import torch

X_MAX, DY_MAX = 3, 2
GUARD = 4096                     # floats per guard: a multiple of 4, so the body stays 16-byte aligned
SENTINEL = 0x5A5AA5A5            # bit pattern of the guards (int32)

Geom = collections.namedtuple('Geom', 'imgs H W C N th tw stride pad_h pad_w Ho Wo')


def geom(imgs, H, W, C, N, th, tw, stride, pad_h, pad_w, Ho=None, Wo=None):
  """Ho / Wo default to the symmetric-padding output size; pad_h / pad_w are LEADING pads, the trailing ones are what Ho / Wo imply."""
  if Ho is None:
    Ho = (H + 2 * pad_h - th) // stride + 1
  if Wo is None:
    Wo = (W + 2 * pad_w - tw) // stride + 1
  return Geom(imgs, H, W, C, N, th, tw, stride, pad_h, pad_w, Ho, Wo)


def pixels(g):
  return g.imgs * g.Ho * g.Wo


def smallest_imgs(Ho, Wo, floor=2048):
  """The smallest image count with M >= floor and M % 32 != 0 (a tail in the last 32-pixel step)."""
  imgs = -(-floor // (Ho * Wo))
  while (imgs * Ho * Wo) % 32 == 0:
    imgs += 1
  return imgs


def assert_exact_regime(M, x_bound=X_MAX):
  assert 2 * x_bound * M < 2 ** 24, 'M = %d leaves the exact regime: %d * M >= 2**24' % (M, 2 * x_bound)


def seed_of(*key):
  return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def int_inputs(seed, dy_shape, x_shape, device='cpu'):
  """(dy, x) as bf16: dy uniform in {-2..2}, x uniform in {-3..3}; generated on the CPU, so one seed gives one case everywhere."""
  g = torch.Generator().manual_seed(seed)
  dy = torch.randint(-DY_MAX, DY_MAX + 1, tuple(dy_shape), generator=g)
  x = torch.randint(-X_MAX, X_MAX + 1, tuple(x_shape), generator=g)
  return dy.to(torch.bfloat16).to(device), x.to(torch.bfloat16).to(device)


def int_scale_shift(seed, C, device='cpu'):
  """[2][C] float32: scale in {1, 2}, integer shift in {-4..4}.  Three channels of four draw their shift from {1..4}: the zero rows a
  kernel reads past a split's end become relu(shift) != 0 there, and only dY's bound makes their products vanish."""
  g = torch.Generator().manual_seed(seed)
  scale = torch.randint(1, 3, (C,), generator=g)
  shift = torch.randint(-4, 5, (C,), generator=g)
  pos = torch.randint(1, 5, (C,), generator=g)
  shift = torch.where(torch.arange(C) % 4 != 0, pos, shift)
  return torch.stack([scale, shift]).to(torch.float32).to(device)


def ref_prologue(x, scale, shift, act):
  """act(scale * x + shift) per channel (last dimension) in float64: small integers, exact in bf16 and float32."""
  y = x.double() * scale.double() + shift.double()
  if act in ('Relu', 'Relu6'):
    y = y.clamp(min=0.0)
  if act == 'Relu6':
    y = y.clamp(max=6.0)
  return y


def prologue_bound(act):
  """Largest |value| ref_prologue can return: 2 * 3 + 4 under Relu (and with no activation), 6 under Relu6."""
  return 6 if act == 'Relu6' else 2 * X_MAX + 4


def ref_wrw(dy, x, th, tw, stride, pad_h, pad_w, Ho, Wo):
  """dW[n][r][s][c] = sum over (img, ho, wo) of dy[img][ho][wo][n] * xpad[img][ho * stride + r][wo * stride + s][c], float64.
  dy: [imgs][Ho][Wo][N], x: [imgs][H][W][C] (any dtype).  x is zero-padded explicitly by pad_h / pad_w in front and by whatever the
  last window needs behind; each tap is one strided slice and one matrix product.  No convolution routine is called."""
  imgs, H, W, C = x.shape
  N = dy.shape[-1]
  assert tuple(dy.shape[:3]) == (imgs, Ho, Wo)
  Hp = max(pad_h + H, (Ho - 1) * stride + th)
  Wp = max(pad_w + W, (Wo - 1) * stride + tw)
  xp = torch.zeros(imgs, Hp, Wp, C, dtype=torch.float64, device=x.device)
  xp[:, pad_h:pad_h + H, pad_w:pad_w + W, :] = x.double()
  dy2 = dy.double().reshape(imgs * Ho * Wo, N)
  out = torch.empty(N, th, tw, C, dtype=torch.float64, device=x.device)
  for r in range(th):
    for s in range(tw):
      xs = xp[:, r:r + (Ho - 1) * stride + 1:stride, s:s + (Wo - 1) * stride + 1:stride, :]
      out[:, r, s, :] = dy2.t() @ xs.reshape(imgs * Ho * Wo, C)
  return out


def expected(ref64, dtype):
  """What a kernel must return for the exact value ref64: it as float32, or the round-to-nearest-even of that to bf16."""
  ref = ref64.float()
  assert torch.equal(ref.double(), ref64), 'the reference itself left the exact regime'
  return ref if dtype == torch.float32 else ref.to(torch.bfloat16)


def assert_equal(dW, ref, what=''):
  """torch.equal(dW, ref), with a diagnosis: a misplaced pixel shows as a tap or border pattern, a lost slab as a uniform offset."""
  assert dW.dtype == ref.dtype and dW.shape == ref.shape, (what, dW.dtype, ref.dtype, tuple(dW.shape), tuple(ref.shape))
  if torch.equal(dW, ref):
    return
  N, C = dW.shape[0], dW.shape[-1]
  a, b = dW.double().reshape(N, -1, C), ref.double().reshape(N, -1, C)
  bad = ~(a == b)                                     # (NaN counts as different)
  idx = bad.nonzero()
  diff = (a - b).abs()
  finite = diff[bad & torch.isfinite(diff)]
  lines = ['%s: %d of %d entries differ, %d of them not finite; largest finite difference %s' % (
      what, int(bad.sum()), bad.numel(), int((bad & ~torch.isfinite(a)).sum()), float(finite.max()) if finite.numel() else None)]
  for n, t, c in idx[:8].tolist():
    lines.append('  (n, tap, c) = (%d, %d, %d): got %r, expected %r' % (n, t, c, float(a[n, t, c]), float(b[n, t, c])))
  per_tap = bad.sum(dim=(0, 2)).tolist()
  lines.append('  differing entries per tap: %s' % per_tap)
  msg = '\n'.join(lines)
  print(msg)
  raise AssertionError(msg)


def guarded_workspace(S, n, device='cuda'):
  """One allocation [guard | body | guard]: body = (S + 32) * n floats of NaN -- the documented workspace size -- between two guards
  of GUARD floats holding SENTINEL.  Returns (ws, check): ws is the body, check() asserts that no guard word changed."""
  body = (S + 32) * n
  buf = torch.empty(GUARD + body + GUARD, dtype=torch.float32, device=device)
  bits = buf.view(torch.int32)
  bits[:GUARD] = SENTINEL
  bits[GUARD + body:] = SENTINEL
  ws = buf[GUARD:GUARD + body]
  ws.fill_(float('nan'))
  assert ws.data_ptr() % 16 == 0

  def check():
    lo, hi = bits[:GUARD] != SENTINEL, bits[GUARD + body:] != SENTINEL
    assert not bool(lo.any()), 'write BELOW the workspace: %d words, first at -%d' % (int(lo.sum()), GUARD - int(lo.nonzero()[0]))
    assert not bool(hi.any()), 'write PAST (S + 32) * n floats: %d words, first at +%d' % (int(hi.sum()), int(hi.nonzero()[0]))
  return ws, check


# ---- the launchers' published rules (pf_wrw.hip: wrw2_pick, pf_wrw2_splits, pf_wrw2_launch, wrw_tr_splits, pf_wrw_plan;
# ---- pf_conv.hip: pf_wrw_scatter_splits, pf_wrw_reduce; pf_wrw3x3_c64.hip: pf_wrw3x3_c64_geom / _splits) ---------------------------
# Recomputed here so that a test can say which tile, map, split and fold class a case is on, and fail when a later change to the
# planner moves it elsewhere.  `sw` are the PF_* switches of a case: dict(PF_WRW2=..., PF_WRW_TR=..., PF_WRW2_TARGET=...,
# PF_WRW2_TK256=..., PF_CONV3X3_C64=...), library defaults where absent.
DEFAULTS = dict(PF_WRW2=1, PF_WRW_TR=0, PF_WRW2_TARGET=0, PF_WRW2_TK256=1, PF_CONV3X3_C64=1)


def _sw(sw, name):
  return int((sw or {}).get(name, DEFAULTS[name]))


def _cdiv(a, b):
  return -(-a // b)


def wrw2_pick(N, C, sw=None):
  tn = 256 if N % 256 == 0 else (128 if N % 128 == 0 else 64)
  tk = 128 if C % 128 == 0 else 64
  if tn <= 128 and C % 256 == 0 and _sw(sw, 'PF_WRW2_TK256') != 0:
    tk = 256
  if tn == 128 and tk == 64:
    return 64, 64
  return tn, tk


def wrw2_splits(M, N, C, taps, sw=None):
  if _sw(sw, 'PF_WRW2') == 0 or C % 64 or N % 64 or M < 2048:
    return 0
  tn, tk = wrw2_pick(N, C, sw)
  tiles = (N // tn) * (taps * C // tk)
  forced = _sw(sw, 'PF_WRW2_TARGET')
  target = forced if forced > 0 else (256 if taps == 1 else 384)
  S = max(1, min(_cdiv(target, tiles), _cdiv(M, 256)))
  return _cdiv(M, wrw2_rows(M, S))


def wrw2_rows(M, S):
  return _cdiv(_cdiv(M, S), 32) * 32


def wrw2_map(th, tw, stride, H, W, Ho, Wo, prologue=False):
  if stride == 1 and th * tw == 1:
    return 0
  m = 1 if (stride == 1 and Ho == H and Wo == W and 32 // Wo + 1 <= Ho) else 2
  return 2 if (prologue and m == 1) else m


def wrw_tr_splits(M, N, C, taps):
  if C % 64 or N % 64 or M < 2048:
    return 0
  bn = 128 if N % 128 == 0 else 64
  tiles = (N // bn) * (taps * C // 64)
  S = max(1, min(_cdiv(256, tiles), _cdiv(M, 512)))
  return _cdiv(M, wrw_tr_rows(M, S))


def wrw_tr_rows(M, S):
  return _cdiv(_cdiv(M, S), 128) * 128


def scatter_splits(M, N, K):
  tiles = _cdiv(N, 128) * _cdiv(K, 64)
  S = max(1, min(_cdiv(768, tiles), _cdiv(M, 256)))
  return _cdiv(M, scatter_rows(M, S))


def scatter_rows(M, S):
  return _cdiv(_cdiv(M, S), 64) * 64


def window_geom(g, sw=None):
  return (_sw(sw, 'PF_CONV3X3_C64') != 0 and (g.th, g.tw, g.stride, g.pad_h, g.pad_w) == (3, 3, 1, 1, 1) and g.C == 64 and g.N == 64 and
          (g.H, g.W, g.Ho, g.Wo) == (56, 56, 56, 56))


def window_splits(imgs):
  return min(imgs * 28, 512)


Plan = collections.namedtuple('Plan', 'kernel S rows tile mapm')      # rows: pixel rows per split (None: window kernel)


def plan(M, N, C, taps, entry_1x1, sw=None, window_imgs=0):
  """pf_wrw_plan, for operands inside the shared-tile kernel's 2 GiB addressing (the tests' are)."""
  if window_imgs > 0:
    return Plan('window', window_splits(window_imgs), None, None, None)
  s2 = wrw2_splits(M, N, C, taps, sw)
  if s2 > 0:
    return Plan('shared', s2, wrw2_rows(M, s2), wrw2_pick(N, C, sw), None)
  s1 = wrw_tr_splits(M, N, C, taps) if (not entry_1x1 or _sw(sw, 'PF_WRW_TR') != 0) else 0
  if s1 > 0:
    return Plan('wave', s1, wrw_tr_rows(M, s1), (128 if N % 128 == 0 else 64, 64), None)
  if entry_1x1:
    S = scatter_splits(M, N, C)
    return Plan('scatter', S, scatter_rows(M, S), (128, 64), None)
  return Plan(None, 0, None, None, None)


def plan_rxs(g, sw=None):
  """What pf_conv2d_wrw launches for geometry g: kernel, slabs it writes and folds, rows per split, tile, pixel map."""
  p = plan(pixels(g), g.N, g.C, g.th * g.tw, False, sw, g.imgs if window_geom(g, sw) else 0)
  mapm = wrw2_map(g.th, g.tw, g.stride, g.H, g.W, g.Ho, g.Wo) if p.kernel == 'shared' else None
  return p._replace(mapm=mapm)


def query_rxs(M, N, C, taps, sw=None):
  """pf_conv2d_wrw_splits: it does not see the image, and answers with the larger count where the window kernel COULD take the launch."""
  s = plan(M, N, C, taps, False, sw).S
  if _sw(sw, 'PF_CONV3X3_C64') != 0 and taps == 9 and N == 64 and C == 64 and M % 3136 == 0:
    s = max(s, window_splits(M // 3136))
  return s


def plan_1x1(M, N, K, sw=None, stride=1, prologue=False):
  p = plan(M, N, K, 1, True, sw)
  mapm = wrw2_map(1, 1, stride, 0, 0, 0, 0, prologue) if p.kernel == 'shared' else None
  return p._replace(mapm=mapm)


def reduce_ranges(S, n):
  """pf_wrw_reduce: (ry, per, [slabs of each of the ry first-stage ranges]); ry == 1 is the one-stage fold."""
  gx = _cdiv(n, 64)
  ry = 1
  while ry < 32 and gx * ry < 1024 and ry * 8 <= S:
    ry *= 2
  per = _cdiv(S, ry)
  return ry, per, [max(0, min(S, (y + 1) * per) - y * per) for y in range(ry)]


def last_split_steps(M, p, step=32):
  """32-pixel steps of the last pixel split of plan p."""
  return _cdiv(M - (p.S - 1) * p.rows, step)
