"""The backward-filter kernels against an integer reference, BIT FOR BIT (tests/wrw_exact.py states why that is possible: small integer
operands, 6 * M < 2**24, so no float32 sum of any order rounds).  Every comparison is torch.equal; there is no tolerance in this file.

Every case
  * first asserts the ROUTE it is on -- kernel, tile, pixel map, slab count, fold class -- from the launchers' published rules
    (wrw_exact.plan_*: wrw2_pick, pf_wrw2_splits, the map rule of pf_wrw2_launch, wrw_tr_splits, pf_wrw_scatter_splits, pf_wrw_reduce)
    and checks the library's own query against them, so a case that a later planner change moves elsewhere FAILS instead of passing
    vacuously (tests/test_wrw_exact_cpu.py walks the same tables without a GPU);
  * runs on a NaN-filled workspace of the documented (S + 32) * n floats between two guards: intact guards = no write outside it, a
    finite exact result = the fold read only slabs that were written;
  * writes into a NaN-filled dW.

Sections (the parametrisations below are the coverage; read them against wrw2_pick / pf_wrw2_launch / pf_wrw_reduce):
  a. RxS entry, shared-tile kernel: all seven tile configurations x {map 1, map 2} on 7 x 7 images at M = 2107, plus the 64 x 64
     fallbacks, PF_WRW2_TK256=0, ResNet-50's stage 4 (512 -> 512), bf16 dW;
  b. map selection and wrap arithmetic of map 1: the rule at equality, several row wraps per step, adv_q == 0, non-square images;
  c. 5x5, 3x1 / 1x3, TF-SAME stride 2, odd images, 1x1 stride 2 through the RxS entry -- shared-tile and wave-private kernels;
  d. split boundaries and short pipelines: last splits of one and two steps, no tail, wavefronts without a step, the scatter
     kernel's partial tiles (M = 333, N = 72, K = 40);
  e. the non-quantising prologue with integer scale / shift (tail rows become relu(shift) != 0 and must still contribute nothing);
  f. the slab fold: one stage, two ranges, sixteen ranges with an empty last one, many slabs in one stage;
  g. the query that knowingly answers with an upper bound (M % 3136 == 0, 64 -> 64, 3x3) and the window kernel itself.

Measured on an MI355X: the 112 cases of this file take 3.3 s of wall time together (pytest's own figure, the allocator poisoning of
tests/conftest.py included); the slowest single case 0.3 s (the first launch of a kernel family), a typical one 10 ms.
"""
import functools

import pytest
import torch

import wrw_exact as WX
from wrw_exact import geom

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope='module')
def hip():
  from pocketflow_amd import hip as h
  assert torch.cuda.is_available(), 'gpu tests need a GPU'
  return h


SHARED = dict(PF_WRW2=1, PF_WRW_TR=0)
WAVE = dict(PF_WRW2=0, PF_WRW_TR=1)          # (the RxS entry takes the wave-private kernel whenever the shared-tile one is off)
SCATTER = dict(PF_WRW2=0, PF_WRW_TR=0)
IMPL = {'shared-tile': SHARED, 'wave-private': WAVE, 'scatter': SCATTER}


def set_switches(monkeypatch, sw):
  """Every PF_* switch the backward-filter plan reads, explicitly: defaults where the case names none."""
  full = dict(WX.DEFAULTS)
  full.update(sw)
  for name, value in full.items():
    monkeypatch.setenv(name, str(value))
  return full


def g1x1(M, N, K):
  """The identity-map 1x1 problem [M][N] x [M][K] as a geometry: one image of 1 x M pixels."""
  return geom(1, 1, M, K, N, 1, 1, 1, 0, 0)


# ---- route assertions (no GPU needed: the queries are host code) -----------------------------------------------------------------
def route_rxs(hip, monkeypatch, g, sw, kernel, tile=None, mapm=None):
  sw = set_switches(monkeypatch, sw)
  M = WX.pixels(g)
  WX.assert_exact_regime(M)
  p = WX.plan_rxs(g, sw)
  S = hip.conv2d_wrw_splits(M, g.N, g.C, g.th * g.tw)
  assert S == WX.query_rxs(M, g.N, g.C, g.th * g.tw, sw), ('the query left the published rules', g, S)
  assert S >= p.S > 0, (g, S, p)
  assert (p.kernel, p.tile, p.mapm) == (kernel, tile, mapm), (g, p)
  return p, S


def route_1x1(hip, monkeypatch, M, N, K, sw, kernel, tile=None, mapm=None, stride=1, prologue=False, x_bound=WX.X_MAX):
  sw = set_switches(monkeypatch, sw)
  WX.assert_exact_regime(M, x_bound)
  p = WX.plan_1x1(M, N, K, sw, stride, prologue)
  S = hip.conv1x1_wrw_splits(M, N, K)
  assert S == p.S > 0, ('the query left the published rules', (M, N, K), S, p)
  assert p.kernel == kernel and p.mapm == mapm and (tile is None or p.tile == tile), ((M, N, K), p)
  return p, S


# ---- inputs and references: one per geometry, shared by every kernel / dtype / switch that runs it ------------------------------------
@functools.lru_cache(maxsize=None)
def case(g, act=None):
  """(dy [imgs][Ho][Wo][N], x [imgs][H][W][C], ss or None, exact dW [N][th][tw][C] in float64), on the device."""
  seed = WX.seed_of(tuple(g), act)
  dy, x = WX.int_inputs(seed, (g.imgs, g.Ho, g.Wo, g.N), (g.imgs, g.H, g.W, g.C), device='cuda')
  ss, xq = None, x
  if act is not None:
    ss = WX.int_scale_shift(seed + 1, g.C, device='cuda')
    xq = WX.ref_prologue(x, ss[0], ss[1], act)
  ref = WX.ref_wrw(dy, xq, g.th, g.tw, g.stride, g.pad_h, g.pad_w, g.Ho, g.Wo)
  return dy, x, ss, ref


def run_rxs(hip, g, S, dtypes=(F32,), twice=False):
  dy, x, _, ref = case(g)
  n = g.N * g.th * g.tw * g.C
  for dt in dtypes:
    outs = []
    for _ in range(2 if twice else 1):
      ws, check = WX.guarded_workspace(S, n)
      dw = torch.full((g.N, g.th, g.tw, g.C), float('nan'), device='cuda', dtype=dt)
      hip.conv2d_wrw(dy, x, dw, ws, g.imgs, g.H, g.W, g.C, g.N, g.th, g.tw, g.stride, g.pad_h, g.pad_w, g.Ho, g.Wo)
      torch.cuda.synchronize()
      check()
      WX.assert_equal(dw, WX.expected(ref, dt), '%s %s' % (g, dt))
      outs.append(dw)
    assert all(torch.equal(outs[0], o) for o in outs[1:])


def run_1x1(hip, g, S, dtypes=(F32,), act=None, twice=False):
  """g through the 1x1 entry (g.th == g.tw == 1, no padding): dW [N][K]."""
  assert (g.th, g.tw, g.pad_h, g.pad_w) == (1, 1, 0, 0)
  dy, x, ss, ref = case(g, act)
  M = WX.pixels(g)
  gm = None if g.stride == 1 else (g.Ho, g.Wo, g.H, g.W, g.stride)
  for dt in dtypes:
    outs = []
    for _ in range(2 if twice else 1):
      ws, check = WX.guarded_workspace(S, g.N * g.C)
      dw = torch.full((g.N, g.C), float('nan'), device='cuda', dtype=dt)
      hip.conv1x1_wrw(dy, x, dw, ws, M, g.N, g.C, scale_shift=ss, act=act, geom=gm)
      torch.cuda.synchronize()
      check()
      WX.assert_equal(dw, WX.expected(ref, dt).reshape(g.N, g.C), '%s %s %s' % (g, act, dt))
      outs.append(dw)
    assert all(torch.equal(outs[0], o) for o in outs[1:])


# ==== a. RxS entry, shared-tile kernel, every tile configuration ======================================================================
# (N, C, PF_WRW2_TK256, the tile wrw2_pick must give, dW dtypes)
A_TILES = [
    (256, 128, 1, (256, 128), (F32, BF16)),
    (128, 128, 1, (128, 128), (F32,)),
    (128, 256, 1, (128, 256), (F32,)),
    (64, 256, 1, (64, 256), (F32,)),
    (256, 64, 1, (256, 64), (F32,)),
    (64, 128, 1, (64, 128), (F32,)),
    (64, 64, 1, (64, 64), (F32, BF16)),
    (192, 64, 1, (64, 64), (F32,)),             # three N-tiles
    (128, 64, 1, (64, 64), (F32,)),             # N % 128 == 0, C % 128 != 0: "(128, 64) has no instantiation"
    (128, 256, 0, (128, 128), (F32,)),          # the 128- and 64-wide tiles by the other path
    (64, 256, 0, (64, 128), (F32,)),
]
# 7 x 7 output images, 43 of them: M = 2107 = 65 * 32 + 27
A_GEOMS = {1: lambda N, C: geom(43, 7, 7, C, N, 3, 3, 1, 1, 1), 2: lambda N, C: geom(43, 14, 14, C, N, 3, 3, 2, 1, 1)}
A_CASES = [(N, C, tk, tile, dts, m) for (N, C, tk, tile, dts) in A_TILES for m in (1, 2)]
A_CASES.append((512, 512, 1, (256, 128), (F32, BF16), 1))       # conv2 of ResNet-50's stage 4 as it runs


def route_a(hip, monkeypatch, N, C, tk256, tile, dtypes, mapm):
  g = A_GEOMS[mapm](N, C)
  assert WX.pixels(g) == 2107 and (g.Ho, g.Wo) == (7, 7)
  p, S = route_rxs(hip, monkeypatch, g, dict(SHARED, PF_WRW2_TK256=tk256), 'shared', tile, mapm)
  assert S == p.S
  if (N, C) == (192, 64):
    assert N // tile[0] == 3
  if (N, C) == (128, 64):
    assert N % 128 == 0 and C % 128 != 0
  # splits begin mid-row and mid-image, and the last one is short
  assert p.S > 1 and p.rows % 7 != 0 and p.rows % 49 != 0 and 2107 % p.rows != 0
  return g, S


@pytest.mark.parametrize('N,C,tk256,tile,dtypes,mapm', A_CASES,
                         ids=['%dx%d-tk256_%d-tile%dx%d-map%d' % (c[0], c[1], c[2], c[3][0], c[3][1], c[5]) for c in A_CASES])
def test_a_every_tile_configuration(hip, monkeypatch, N, C, tk256, tile, dtypes, mapm):
  g, S = route_a(hip, monkeypatch, N, C, tk256, tile, dtypes, mapm)
  run_rxs(hip, g, S, dtypes)


# ==== b. map selection and wrap arithmetic ============================================================================================
# (Ho, Wo, the map pf_wrw2_launch must select, what the case is)
B_IMAGES = [
    (5, 8, 1, 'rule at equality: four row wraps and an image wrap inside one step'),
    (3, 16, 1, 'rule at equality'),
    (2, 8, 2, 'rule fails'),
    (4, 4, 2, 'rule fails'),
    (3, 40, 1, 'Wo > 32: adv_q == 0'),
    (40, 3, 1, 'ten rows and two pixels per step'),
    (9, 23, 1, 'non-square, nothing divides 32'),
    (23, 9, 1, 'non-square, nothing divides 32'),
]
B_CASES = [(64, 64, (64, 64)) + im for im in B_IMAGES] + [(128, 128, (128, 128)) + B_IMAGES[0]]


def route_b(hip, monkeypatch, N, C, tile, Ho, Wo, mapm, what):
  g = geom(WX.smallest_imgs(Ho, Wo), Ho, Wo, C, N, 3, 3, 1, 1, 1)
  M = WX.pixels(g)
  assert (g.Ho, g.Wo) == (Ho, Wo) and M >= 2048 and M % 32 != 0 and (M - Ho * Wo < 2048 or (M - Ho * Wo) % 32 == 0)
  rule = 32 // Wo + 1 <= Ho
  assert rule == (mapm == 1)
  if 'equality' in what:
    assert 32 // Wo + 1 == Ho
  if 'adv_q' in what:
    assert 32 // Wo == 0
  p, S = route_rxs(hip, monkeypatch, g, SHARED, 'shared', tile, mapm)
  assert S == p.S
  return g, S


@pytest.mark.parametrize('N,C,tile,Ho,Wo,mapm,what', B_CASES, ids=['%dx%d-%dx%d-map%d' % (c[0], c[1], c[3], c[4], c[5]) for c in B_CASES])
def test_b_map_selection_and_wraps(hip, monkeypatch, N, C, tile, Ho, Wo, mapm, what):
  g, S = route_b(hip, monkeypatch, N, C, tile, Ho, Wo, mapm, what)
  run_rxs(hip, g, S)


# ==== c. window and padding shapes ====================================================================================================
# (name, geometry for `imgs` images, the shared-tile kernel's map); 64 -> 64 channels
C_SHAPES = [
    ('5x5-pad2', lambda i: geom(i, 12, 10, 64, 64, 5, 5, 1, 2, 2), 1),
    ('3x1-pad1,0', lambda i: geom(i, 9, 11, 64, 64, 3, 1, 1, 1, 0), 1),
    ('1x3-pad0,1', lambda i: geom(i, 9, 11, 64, 64, 1, 3, 1, 0, 1), 1),
    ('3x3-s2-tf-same-even', lambda i: geom(i, 14, 14, 64, 64, 3, 3, 2, 0, 0, 7, 7), 2),      # leading pad 0, one trailing row / column
    ('3x3-s2-odd-15x9', lambda i: geom(i, 15, 9, 64, 64, 3, 3, 2, 1, 1), 2),
    ('1x1-s2-15x9', lambda i: geom(i, 15, 9, 64, 64, 1, 1, 2, 0, 0), 2),
]
C_CASES = [(name, mk, mapm, impl) for (name, mk, mapm) in C_SHAPES for impl in ('shared-tile', 'wave-private')]


def route_c(hip, monkeypatch, name, mk, mapm, impl):
  g1 = mk(1)
  g = mk(WX.smallest_imgs(g1.Ho, g1.Wo))
  if 'tf-same' in name:
    assert (g.Ho - 1) * g.stride + g.th == g.H + 1 and g.pad_h == 0        # the last window hangs one row over the image
  if '15x9' in name:
    assert (g.Ho, g.Wo) == (8, 5)
  if impl == 'shared-tile':
    p, S = route_rxs(hip, monkeypatch, g, SHARED, 'shared', (64, 64), mapm)
  else:
    p, S = route_rxs(hip, monkeypatch, g, WAVE, 'wave', (64, 64), None)
  assert S == p.S
  return g, S


@pytest.mark.parametrize('name,mk,mapm,impl', C_CASES, ids=['%s-%s' % (c[0], c[3]) for c in C_CASES])
def test_c_window_and_padding_shapes(hip, monkeypatch, name, mk, mapm, impl):
  g, S = route_c(hip, monkeypatch, name, mk, mapm, impl)
  run_rxs(hip, g, S)


# ==== d. split boundaries and short pipelines =========================================================================================
# 64 -> 64 channels.  (entry, impl, geometry, slabs, 32-pixel steps of the last split)
def _g3(imgs, H, W, stride=1):
  return geom(imgs, H, W, 64, 64, 3, 3, stride, 1, 1)


D_CASES = [
    # shared-tile kernel, 256-row splits: the ring's start-up branches nsteps == 1, nsteps == 2, and no tail at all
    ('1x1', 'shared-tile', g1x1(2049, 64, 64), 9, 1),
    ('1x1', 'shared-tile', g1x1(2088, 64, 64), 9, 2),
    ('1x1', 'shared-tile', g1x1(2048, 64, 64), 8, 8),
    ('3x3', 'shared-tile', _g3(1, 3, 683), 9, 1),                  # M = 2049, map 1
    ('3x3', 'shared-tile', _g3(683, 1, 3), 9, 1),                  # M = 2049, map 2 (32 / 3 + 1 > 1)
    ('3x3', 'shared-tile', _g3(29, 8, 9), 9, 2),                   # M = 2088, map 1
    ('3x3', 'shared-tile', _g3(29, 16, 18, 2), 9, 2),              # M = 2088, map 2
    ('3x3', 'shared-tile', _g3(32, 8, 8), 8, 8),                   # M = 2048, map 1
    ('3x3', 'shared-tile', _g3(32, 16, 16, 2), 8, 8),              # M = 2048, map 2
    # wave-private kernel, 512-row splits, wavefront w takes steps w, w + 4, ...: one step (three wavefronts idle), three steps
    # (one idle), five steps (wavefront 0 takes two)
    ('1x1', 'wave-private', g1x1(2049, 64, 64), 5, 1),
    ('1x1', 'wave-private', g1x1(2118, 64, 64), 5, 3),
    ('1x1', 'wave-private', g1x1(2177, 64, 64), 5, 5),
    ('3x3', 'wave-private', _g3(1, 3, 683), 5, 1),
    ('3x3', 'wave-private', _g3(1, 6, 353), 5, 3),
    ('3x3', 'wave-private', _g3(1, 7, 311), 5, 5),
    # scatter kernel, 256-row splits in 64-pixel steps; partial tiles in N and K, and M below every other kernel's floor
    ('1x1', 'scatter', g1x1(2049, 64, 64), 9, 1),
    ('1x1', 'scatter', g1x1(2088, 64, 64), 9, 2),
    ('1x1', 'scatter', g1x1(2048, 64, 64), 8, 8),
    ('1x1', 'scatter', g1x1(333, 64, 64), 2, 5),
    ('1x1', 'scatter', g1x1(333, 72, 40), 2, 5),
    ('1x1', 'scatter', g1x1(2049, 72, 40), 9, 1),
    ('1x1', 'default', g1x1(2049, 72, 40), 9, 1),                  # N % 64 != 0: the scatter kernel with no switch set
]


def route_d(hip, monkeypatch, entry, impl, g, S_want, last_steps):
  M = WX.pixels(g)
  kernel = {'shared-tile': 'shared', 'wave-private': 'wave', 'scatter': 'scatter', 'default': 'scatter'}[impl]
  sw = IMPL.get(impl, {})
  if entry == '1x1':
    p, S = route_1x1(hip, monkeypatch, M, g.N, g.C, sw, kernel, mapm=0 if kernel == 'shared' else None)
  else:
    p, S = route_rxs(hip, monkeypatch, g, sw, kernel, (64, 64),
                     WX.wrw2_map(3, 3, g.stride, g.H, g.W, g.Ho, g.Wo) if kernel == 'shared' else None)
  assert S == p.S == S_want, (S, p)
  assert WX.last_split_steps(M, p) == last_steps, (M, p)
  return S


@pytest.mark.parametrize('entry,impl,g,S_want,last_steps', D_CASES, ids=['%s-%s-M%d-N%d-C%d-%dx%d-s%d' % (
    c[0], c[1], WX.pixels(c[2]), c[2].N, c[2].C, c[2].H, c[2].W, c[2].stride) for c in D_CASES])
def test_d_split_boundaries_and_short_pipelines(hip, monkeypatch, entry, impl, g, S_want, last_steps):
  S = route_d(hip, monkeypatch, entry, impl, g, S_want, last_steps)
  (run_1x1 if entry == '1x1' else run_rxs)(hip, g, S)


# ==== e. the non-quantising prologue, exact ===========================================================================================
E_TILES = [(64, 64, (64, 64)), (256, 128, (256, 128)), (64, 256, (64, 256))]
E_MAPS = {'identity': lambda N, C: g1x1(2107, N, C), 'stride2': lambda N, C: geom(43, 14, 14, C, N, 1, 1, 2, 0, 0)}
E_CASES = [(act, mp, N, C, tile, impl) for act in ('Relu', 'Relu6') for mp in ('identity', 'stride2') for (N, C, tile) in E_TILES
           for impl in ('shared-tile', 'scatter', 'wave-private')]


def route_e(hip, monkeypatch, act, mp, N, C, tile, impl):
  g = E_MAPS[mp](N, C)
  M = WX.pixels(g)
  assert M == 2107 and M % 32 != 0
  kernel = {'shared-tile': 'shared', 'wave-private': 'wave', 'scatter': 'scatter'}[impl]
  mapm = (0 if mp == 'identity' else 2) if kernel == 'shared' else None
  p, S = route_1x1(hip, monkeypatch, M, N, C, IMPL[impl], kernel, tile if kernel == 'shared' else None, mapm, g.stride, True,
                   x_bound=WX.prologue_bound(act))
  assert M % p.rows != 0 and (M % p.rows) % 32 != 0          # the last split ends inside a step: tail rows are staged and transformed
  return g, S


@pytest.mark.parametrize('act,mp,N,C,tile,impl', E_CASES, ids=['%s-%s-%dx%d-%s' % (c[0], c[1], c[2], c[3], c[5]) for c in E_CASES])
def test_e_prologue_exact(hip, monkeypatch, act, mp, N, C, tile, impl):
  g, S = route_e(hip, monkeypatch, act, mp, N, C, tile, impl)
  ss = case(g, act)[2]
  assert int((ss[1] > 0).sum()) > C // 2                     # tail rows become relu(shift) > 0 on most channels: not vacuous
  assert set(ss[0].tolist()) <= {1.0, 2.0} and float(ss[1].abs().max()) <= 4
  run_1x1(hip, g, S, act=act)


# ==== f. the fold =====================================================================================================================
# 1x1 entry, shared-tile kernel, S forced through PF_WRW2_TARGET.  (N, C, M, target, S, ry, slabs per first-stage range)
F_CASES = [
    (64, 64, 2107, 7, 7, 1, [7]),                                  # one stage
    (64, 64, 2107, 9, 9, 2, [5, 4]),                               # two ranges
    (64, 64, 130 * 256, 130, 130, 16, [9] * 14 + [4, 0]),          # sixteen ranges: a short one and an EMPTY one
    (256, 256, 33 * 256, 66, 33, 1, [33]),                         # gx = 1024: one stage despite 33 slabs
]


def route_f(hip, monkeypatch, N, C, M, target, S_want, ry, ranges):
  p, S = route_1x1(hip, monkeypatch, M, N, C, dict(SHARED, PF_WRW2_TARGET=target), 'shared', mapm=0)
  assert S == S_want
  assert WX.reduce_ranges(S, N * C) == (ry, -(-S // ry), ranges)
  return S


@pytest.mark.parametrize('N,C,M,target,S_want,ry,ranges', F_CASES, ids=['%dx%d-S%d-ry%d' % (c[0], c[1], c[4], c[5]) for c in F_CASES])
def test_f_fold(hip, monkeypatch, N, C, M, target, S_want, ry, ranges):
  S = route_f(hip, monkeypatch, N, C, M, target, S_want, ry, ranges)
  run_1x1(hip, g1x1(M, N, C), S, dtypes=(F32, BF16), twice=True)


# ==== g. the over-sized query =========================================================================================================
# 64 -> 64, 3x3 / stride 1 / pad 1, M % 3136 == 0.  (H, W, imgs, PF_CONV3X3_C64, kernel, slabs the launch folds, slabs the query names)
G_CASES = [
    (28, 112, 1, 1, 'shared', 13, 28),                             # not 56 x 56: the launch folds fewer slabs than the caller sized for
    (28, 112, 2, 1, 'shared', 25, 56),
    (56, 56, 1, 1, 'window', 28, 28),
    (56, 56, 3, 1, 'window', 84, 84),
    (56, 56, 1, 0, 'shared', 13, 13),
    (56, 56, 3, 0, 'shared', 37, 37),
]


def route_g(hip, monkeypatch, H, W, imgs, c64, kernel, S_launch, S_query):
  g = geom(imgs, H, W, 64, 64, 3, 3, 1, 1, 1)
  assert WX.pixels(g) == 3136 * imgs
  if kernel == 'shared':
    assert 32 // g.Wo == 0                                         # map 1 with adv_q == 0
    p, S = route_rxs(hip, monkeypatch, g, dict(SHARED, PF_CONV3X3_C64=c64), 'shared', (64, 64), 1)
  else:
    p, S = route_rxs(hip, monkeypatch, g, dict(SHARED, PF_CONV3X3_C64=c64), 'window')
  assert (p.S, S) == (S_launch, S_query)
  return g, S


@pytest.mark.parametrize('H,W,imgs,c64,kernel,S_launch,S_query', G_CASES,
                         ids=['%dx%d-imgs%d-c64_%d-%s' % (c[0], c[1], c[2], c[3], c[4]) for c in G_CASES])
def test_g_query_upper_bound_and_window_kernel(hip, monkeypatch, H, W, imgs, c64, kernel, S_launch, S_query):
  g, S = route_g(hip, monkeypatch, H, W, imgs, c64, kernel, S_launch, S_query)
  run_rxs(hip, g, S, dtypes=(F32, BF16))          # the workspace is sized by the QUERY, as graph.py sizes it


ROUTES = [(route_a, A_CASES), (route_b, B_CASES), (route_c, C_CASES), (route_d, D_CASES), (route_e, E_CASES), (route_f, F_CASES),
          (route_g, G_CASES)]
