"""Host side of the int8 inference path: the layer formula (int8.conv_reference) against a float64 convolution of the decoded
operands, the signed-byte identities the kernel rests on, packing, eligibility, the raw-codes loader, and the register budget of the
compiled kernels.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from pocketflow_amd import int8
from pocketflow_amd.tools.conversion import export_quant_int8_model as ex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMS = [(1, 1, 0), (1, 2, 0), (3, 1, 1), (3, 2, 1)]          # (R = S, stride, pad)


def _operands(rng, C, N, R, bits_a=8, bits_w=8, B=2, H=13, W=11):
  c = rng.integers(0, 2 ** bits_a, size=(B, H, W, C), dtype=np.int64).astype(np.uint8)
  d = rng.integers(0, 2 ** bits_w, size=(N, R, R, C), dtype=np.int64).astype(np.uint8)
  alpha_w = rng.uniform(0.05, 0.6, N)
  beta_w = -rng.uniform(0.02, 0.3, N)
  return c, d, alpha_w, beta_w


def _conv64(a, w, stride, pad):
  """Plain float64 convolution: a [B][H][W][C] (zeros outside the image), w [N][R][S][C]."""
  B, H, W, C = a.shape
  N, R, S, _ = w.shape
  Ho, Wo = int8.out_size(H, R, stride, pad), int8.out_size(W, S, stride, pad)
  ap = np.zeros((B, H + 2 * pad, W + 2 * pad, C))
  ap[:, pad:pad + H, pad:pad + W] = a
  y = np.zeros((B, Ho, Wo, N))
  for r in range(R):
    for s in range(S):
      y += ap[:, r:r + (Ho - 1) * stride + 1:stride, s:s + (Wo - 1) * stride + 1:stride] @ w[:, r, s].T
  return y


@pytest.mark.parametrize('beta_a', [0.0, 0.37])
@pytest.mark.parametrize('C', [16, 48, 64])
@pytest.mark.parametrize('R,stride,pad', GEOMS)
def test_conv_reference_is_the_convolution_of_the_decoded_operands(R, stride, pad, C, beta_a):
  rng = np.random.default_rng(1000 * R + 100 * stride + C + int(beta_a * 100))
  N = 24
  c, d, alpha_w, beta_w = _operands(rng, C, N, R)
  alpha_a = 2.71
  a = beta_a + alpha_a * c.astype(np.float64) / 255.0
  w = beta_w[:, None, None, None] + alpha_w[:, None, None, None] * d.astype(np.float64) / 255.0
  want = _conv64(a, w, stride, pad)
  got = int8.conv_reference(c, alpha_a, beta_a, 8, d, alpha_w, beta_w, 8, stride, pad, pad)
  assert got.shape == want.shape == (2, int8.out_size(13, R, stride, pad), int8.out_size(11, R, stride, pad), N)
  assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))
  res = rng.standard_normal(want.shape)
  got_r, mag = int8.conv_reference(c, alpha_a, beta_a, 8, d, alpha_w, beta_w, 8, stride, pad, pad, residual=res, terms=True)
  assert np.max(np.abs(got_r - (want + res))) <= 1e-12 * np.max(np.abs(want))
  assert np.all(mag >= np.abs(got_r) - 1e-9)


@pytest.mark.parametrize('R,stride,pad', GEOMS)
def test_signed_byte_identities_are_exact(R, stride, pad):
  """P = sum s t + 128 sum s + 128 sum_all t[n] + 16384 K and Sc = sum s + 128 K with s = c - 128, t = d - 128, padding taps held as
  s = -128 (code 0) and the K tail as s = t = 0: what pf_conv_i8_fwd computes from its int32 accumulators."""
  rng = np.random.default_rng(7 + R + stride)
  C, N = 48, 8
  c, d, _, _ = _operands(rng, C, N, R)
  K = R * R * C
  ones = np.ones(N)
  P = int8.conv_reference(c, 255.0, 0.0, 8, d, 255.0 * ones, 0.0 * ones, 8, stride, pad, pad)              # scales 1: y = P
  Sc = int8.conv_reference(c, 255.0, 0.0, 8, d, 0.0 * ones, ones, 8, stride, pad, pad)[..., 0]          # y = Sc
  s_img = c.astype(np.int64) - 128
  t = d.astype(np.int64) - 128
  B, H, W, _ = c.shape
  sp = np.full((B, H + 2 * pad, W + 2 * pad, C), -128, np.int64)
  sp[:, pad:pad + H, pad:pad + W] = s_img
  Ho, Wo = P.shape[1:3]
  st = np.zeros((B, Ho, Wo, N), np.int64)
  ss = np.zeros((B, Ho, Wo), np.int64)
  for r in range(R):
    for q in range(R):
      win = sp[:, r:r + (Ho - 1) * stride + 1:stride, q:q + (Wo - 1) * stride + 1:stride]
      st += win @ t[:, r, q].T
      ss += win.sum(axis=3)
  assert np.abs(st).max() < 2 ** 31 and K * 2 ** 14 < 2 ** 31
  tsum = t.reshape(N, -1).sum(axis=1)
  assert np.array_equal(P.astype(np.int64), st + 128 * ss[..., None] + 128 * tsum + 16384 * K) and np.array_equal(P, np.rint(P))
  assert np.array_equal(Sc.astype(np.int64), ss + 128 * K)


@pytest.mark.parametrize('mode', [ex.MODE_TENSOR, ex.MODE_CHANNEL])
@pytest.mark.parametrize('bits', [4, 8])
def test_pack_layer_round_trips(mode, bits):
  rng = np.random.default_rng(bits + mode)
  R, S, C, N = 3, 3, 16, 24                               # K = 144: the packed rows carry a 48-byte zero tail
  nb = 1 if mode == ex.MODE_TENSOR else N
  d_hwio = rng.integers(0, 2 ** bits, size=(R, S, C, N)).astype(np.uint8)
  alpha = rng.uniform(0.1, 1.0, nb).astype(np.float32)
  beta = -rng.uniform(0.1, 1.0, nb).astype(np.float32)
  meta = np.array([bits, mode, 0, R, S, C, N], np.int64)
  p = int8.pack_layer(ex.pack_codes(d_hwio.reshape(-1), bits), alpha, beta, meta)
  assert p['w'].dtype == np.int8 and p['w'].shape == (N, 192) and not p['w'][:, 144:].any()
  krsc = np.transpose(d_hwio, (3, 0, 1, 2))
  assert np.array_equal(int8.unpack_layer(p), krsc) and np.array_equal(p['d'], krsc)
  assert np.array_equal(p['tsum'], (krsc.astype(np.int64) - 128).reshape(N, -1).sum(axis=1))
  assert np.array_equal(p['tapsum'], krsc.astype(np.int64).sum(axis=3).reshape(N, R * S))
  k = np.float32(2 ** bits - 1)
  assert np.array_equal(p['scale_beta'][:, 0], np.broadcast_to(alpha / k, (N,))) and p['scale_beta'].dtype == np.float32
  assert np.array_equal(p['scale_beta'][:, 1], np.broadcast_to(beta, (N,)))
  # the decoded kernel of the artefact is beta + alpha * d / k, channel by channel
  dec = ex.decode_tensor(ex.pack_codes(d_hwio.reshape(-1), bits), alpha, beta, meta)
  mine = p['beta'][:, None, None, None].astype(np.float64) + p['alpha'][:, None, None, None].astype(np.float64) * krsc / float(k)
  assert np.allclose(np.transpose(dec, (3, 0, 1, 2)), mine, rtol=1e-6, atol=1e-7)


def test_pack_layer_rejects_what_the_path_does_not_cover():
  codes = ex.pack_codes(np.zeros(16 * 8, np.uint8), 8)
  one = np.ones(1, np.float32)
  with pytest.raises(ValueError, match='split'):
    int8.pack_layer(codes, one, one, np.array([8, ex.MODE_SPLIT, 64, 1, 1, 16, 8]))
  with pytest.raises(ValueError, match='bit'):
    int8.pack_layer(codes, one, one, np.array([9, ex.MODE_TENSOR, 0, 1, 1, 16, 8]))
  with pytest.raises(ValueError, match='Conv2D'):
    int8.pack_layer(codes, one, one, np.array([8, ex.MODE_TENSOR, 0, 16, 8]))
  with pytest.raises(ValueError, match='pairs'):
    int8.pack_layer(codes, one, one, np.array([8, ex.MODE_CHANNEL, 0, 1, 1, 16, 8]))


def test_supported_grid_matches_the_library():
  from pocketflow_amd import hip
  for C in (3, 8, 16, 24, 48, 64, 2048, 8192, 14576, 16384):
    for N in (4, 8, 12, 72, 1000, 1024):
      for R in (1, 3, 7):
        for stride in (1, 2, 3):
          want = C % 16 == 0 and N % 8 == 0 and stride in (1, 2) and R * R * C * 2 ** 14 < 2 ** 31
          assert hip.conv_i8_supported(C, N, R, R, stride) == want == int8.supported(C, N, R, R, stride), (C, N, R, stride)
  assert hip.conv_i8_supported(14560, 8, 3, 3, 1) and not hip.conv_i8_supported(14576, 8, 3, 3, 1)       # 9 C 2^14 around 2^31
  assert not hip.conv_i8_supported(0, 8, 1, 1, 1) and not hip.conv_i8_supported(16, 8, 1, 0, 1)


def test_load_codes_returns_the_raw_tensors_beside_the_decoded_ones(tmp_path):
  rng = np.random.default_rng(3)
  shape = (3, 3, 16, 8)
  w = rng.standard_normal(shape).astype(np.float32)
  flat = w.reshape(-1, shape[-1])
  beta = flat.min(axis=0)
  alpha = (flat.max(axis=0) - beta + np.float32(1e-10)).astype(np.float32)
  k = np.float32(255)
  wq = (alpha * (np.rint((w - beta) / alpha * k) / k).astype(np.float32)).astype(np.float32) + beta
  packed, meta = ex.encode_tensor(wq, alpha, beta, 8, ex.MODE_CHANNEL, 0)
  path = str(tmp_path / 'model_int8.npz')
  np.savez(path, **{'m/conv/kernel/codes': packed, 'm/conv/kernel/alpha': alpha, 'm/conv/kernel/beta': beta, 'm/conv/kernel/meta': meta,
                    'm/bn/gamma': np.ones(8, np.float32)})
  variables, raw = ex.load_codes(path)
  assert sorted(variables) == ['m/bn/gamma', 'm/conv/kernel'] and list(raw) == ['m/conv/kernel']
  assert np.array_equal(variables['m/conv/kernel'].view(np.uint32), wq.view(np.uint32))
  r = raw['m/conv/kernel']
  assert np.array_equal(r['codes'], packed) and np.array_equal(r['alpha'], alpha) and np.array_equal(r['meta'], meta)
  p = int8.pack_layer(r['codes'], r['alpha'], r['beta'], r['meta'])
  assert p['shape'] == shape and np.array_equal(p['d'], np.transpose(ex.unpack_codes(packed, 8, w.size).reshape(shape), (3, 0, 1, 2)))


def test_int8_kernels_compile_without_spills(tmp_path):
  """pf_conv_i8.hip for gfx950: no kernel of the file may spill vector registers or need more than 256 of them."""
  hipcc = '/opt/rocm/bin/hipcc'
  if not os.path.exists(hipcc):
    pytest.skip('no hipcc')
  out = str(tmp_path / 'pf_conv_i8.s')
  flags = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fhip-fp32-correctly-rounded-divide-sqrt', '-S',
           '--cuda-device-only']
  r = subprocess.run([hipcc] + flags + [os.path.join(ROOT, 'pocketflow_amd', 'csrc', 'pf_conv_i8.hip'), '-o', out], capture_output=True,
                     text=True, timeout=600)
  assert r.returncode == 0, r.stderr[-2000:]
  seen = []
  for m in re.finditer(r'\.name:\s+(\S+)(.*?)\.wavefront_size', open(out).read(), re.S):
    name, blk = m.group(1), m.group(2)
    vg = int(re.search(r'\.vgpr_count:\s+(\d+)', blk).group(1))
    sp = int(re.search(r'\.vgpr_spill_count:\s+(\d+)', blk).group(1))
    print(name, vg, sp)
    assert sp == 0 and vg <= 256, (name, vg, sp)
    seen.append(name)
  assert sum('k_conv_i8' in n for n in seen) == 2 and sum('k_bn_codes' in n for n in seen) == 12


def test_takes_codes_truth_table():
  """`takes_codes(shape, is_cuda)` -- the one test of "this layer will multiply codes" that __call__ and a requantising producer
  share -- on shapes alone: no tensor, no GPU, no finalised graph.  Stride 2 on 8 x 8 makes the 'SAME' pads (0, 1), which the
  kernel on codes (symmetric pads only) does not take; on 7 x 7 they are (1, 1)."""
  import torch
  from pocketflow_amd import graph as G
  g = G.Graph('model', 'cpu', torch.float32)
  slot = {'packed': True}                                             # any non-None value: takes_codes only asks whether it is there
  with g.as_default():
    c1 = G.Conv2D(g, 'c1', 16, 8, 3, stride=1)
    c2 = G.Conv2D(g, 'c2', 16, 8, 3, stride=2)
    cb = G.Conv2D(g, 'cb', 16, 8, 3, stride=1, use_bias=True)
    cg = G.Conv2D(g, 'cg', 16, 8, 3, stride=1)
    dw = G.DepthwiseConv2D(g, 'dw', 48, 3, 1)
  for layer in (c1, c2, cb, cg, dw):
    assert not layer.takes_codes((2, layer.kernel.ref_shape[2], 8, 8), True)          # no slot
    layer.int8 = slot
  cg.kernel.gather_host = np.arange(8, dtype=np.int32)
  assert c1.takes_codes((2, 16, 8, 8), True)
  assert not c2.takes_codes((2, 16, 8, 8), True) and c2.takes_codes((2, 16, 7, 7), True)
  assert not cb.takes_codes((2, 16, 8, 8), True)
  assert not c1.takes_codes((2, 24, 8, 8), True)
  assert not c1.takes_codes((2, 16), True)
  assert not c1.takes_codes((2, 16, 8, 8), False)
  assert not cg.takes_codes((2, 16, 8, 8), True)
  assert dw.takes_codes((2, 48, 8, 8), True)
  assert not dw.takes_codes((2, 32, 8, 8), True) and not dw.takes_codes((2, 48), True) and not dw.takes_codes((2, 48, 8, 8), False)
  g.taps = {}
  assert not c1.takes_codes((2, 16, 8, 8), True) and not dw.takes_codes((2, 48, 8, 8), True)
