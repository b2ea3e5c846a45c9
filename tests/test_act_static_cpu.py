"""Host side of int8 inference with fixed activation ranges: the NumPy statement of the static quantiser (int8.static_codes /
static_value / requant_reference), ranges in the artefact and their validation, the consumer wiring of MobileNet-v1, and the register
budget of the new kernel files.  No GPU."""
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from pocketflow_amd import int8
from pocketflow_amd.tools.conversion import export_quant_int8_model as ex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _values(rng, n, lo, hi):
  """Values that cover the range, its surroundings, both ends and the exact grid points and mid-points."""
  u = rng.uniform(lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo), n).astype(np.float32)
  grid = (lo + (hi - lo) * np.arange(0, 511) / 510.0).astype(np.float32)          # grid points and half-way points of an 8-bit grid
  return np.concatenate([u, grid, np.array([lo, hi, np.nextafter(np.float32(lo), np.float32(-9)), np.nextafter(np.float32(hi), np.float32(9))],
                                           np.float32)])


@pytest.mark.parametrize('bits', [4, 8])
@pytest.mark.parametrize('lo,hi', [(0.0, 6.0), (0.37, 2.9), (-1.25, 0.8)])
def test_static_codes_is_the_per_batch_chain_inside_the_range_and_clamps_outside(lo, hi, bits):
  rng = np.random.default_rng(bits + int(hi * 10))
  u = _values(rng, 20000, lo, hi)
  alpha, beta = int8.range_alpha_beta(lo, hi)
  assert alpha.dtype == np.float32 and alpha == np.float32(np.float32(hi) - np.float32(lo)) + np.float32(1e-10) and beta == np.float32(lo)
  k = np.float32(2 ** bits - 1)
  codes = int8.static_codes(u, alpha, beta, bits)
  assert codes.dtype == np.uint8 and codes.shape == u.shape
  inside = (u >= beta) & (u <= beta + alpha)
  chain = np.rint((((u - beta).astype(np.float32) / alpha).astype(np.float32) * k).astype(np.float32))       # uq_code without its clamp
  assert inside.sum() > 5000 and np.array_equal(codes[inside], chain[inside].astype(np.uint8))
  assert (u < beta).sum() > 1000 and np.all(codes[u < beta] == 0)
  assert (u > beta + alpha).sum() > 1000 and np.all(codes[u > beta + alpha] == int(k))
  assert codes.min() == 0 and codes.max() == int(k)
  # values: multiply, then add, each rounded to float32
  val = int8.static_value(codes, alpha, beta, bits)
  want = (alpha * (codes.astype(np.float32) / k).astype(np.float32)).astype(np.float32) + beta
  assert val.dtype == np.float32 and np.array_equal(val.view(np.uint32), want.astype(np.float32).view(np.uint32))
  with pytest.raises(ValueError):
    int8.static_codes(u, alpha, beta, 9)


@pytest.mark.parametrize('bits', [4, 8])
def test_static_codes_against_float64_differs_only_at_half_integers(bits):
  """The float32 chain and the float64 statement of the same quantiser pick different codes only where t = (u - beta) / alpha * k lies
  within a few float32 ulps of a half-integer: every differing element is enumerated and checked, none is merely counted.  The bound
  is 4 ulp(k): the chain makes three float32 roundings (subtract, divide, multiply) of numbers that map to at most k, half an ulp
  each, and alpha itself carries one more from its own subtraction."""
  rng = np.random.default_rng(17 + bits)
  lo, hi = 0.37, 2.9
  u = _values(rng, 200000, lo, hi)
  alpha, beta = int8.range_alpha_beta(lo, hi)
  k = float(2 ** bits - 1)
  got = int8.static_codes(u, alpha, beta, bits).astype(np.int64)
  t64 = np.clip((u.astype(np.float64) - float(beta)) / float(alpha) * k, 0.0, k)
  want = np.rint(t64).astype(np.int64)
  bad = np.flatnonzero(got != want)
  print('bits %d: %d of %d elements differ from the float64 statement' % (bits, bad.size, u.size))
  ulp = np.spacing(np.float32(k)).astype(np.float64)                   # the coarsest float32 spacing t can have
  for i in bad:
    assert abs(int(got[i]) - int(want[i])) == 1, (i, u[i], got[i], want[i])
    assert abs(t64[i] - (np.floor(t64[i]) + 0.5)) <= 4 * ulp, (i, u[i], t64[i])
  assert bad.size < u.size // 100


def test_requant_reference_composes_the_layer_the_consumer_and_the_quantiser():
  rng = np.random.default_rng(5)
  C, N = 16, 8
  c = rng.integers(0, 256, size=(2, 6, 5, C)).astype(np.uint8)
  d = rng.integers(0, 256, size=(N, 3, 3, C)).astype(np.uint8)
  aw, bw = rng.uniform(0.05, 0.6, N), -rng.uniform(0.02, 0.3, N)
  scale, shift = rng.uniform(0.5, 1.5, N), rng.standard_normal(N)
  y = int8.conv_reference(c, 2.5, 0.0, 8, d, aw, bw, 8, 1, 1, 1)
  u = np.clip(scale * y + shift, 0.0, 6.0)
  lo, hi = float(np.percentile(u, 10)), float(np.percentile(u, 90))
  codes, val = int8.requant_reference(c, 2.5, 0.0, 8, d, aw, bw, 8, 1, scale, shift, 'Relu6', lo, hi, 4, pad_h=1, pad_w=1)
  assert codes.shape == y.shape and codes.min() == 0 and codes.max() == 15
  assert np.array_equal(codes, np.rint(np.clip((u - lo) / ((hi - lo) + 1e-10) * 15.0, 0, 15)).astype(np.int64))
  assert np.allclose(val, ((hi - lo) + 1e-10) * codes / 15.0 + lo, rtol=0, atol=1e-12)
  dd = rng.integers(0, 256, size=(C, 3, 3)).astype(np.uint8)
  yd = int8.depthwise_reference(c, 2.5, 0.1, 8, dd, 0.3, -0.1, 8, 2)
  codes_d, _ = int8.requant_reference(c, 2.5, 0.1, 8, dd, 0.3, -0.1, 8, 2, np.ones(C), np.zeros(C), 'Relu', 0.0, float(yd.max()), 8)
  assert codes_d.shape == yd.shape and codes_d.max() == 255


def test_decode_slots_inverts_the_device_encoding():
  def enc(f):
    v = np.float32(f).view(np.uint32)
    return np.uint32(~v) if v & np.uint32(0x80000000) else np.uint32(v | np.uint32(0x80000000))
  pairs = [(0.0, 6.0), (-1.5, 2.25), (0.37, 0.37), (-3.0, -1.0)]
  slots = np.array([[enc(mn), ~enc(mx)] for mn, mx in pairs], np.uint32).view(np.int32)
  mn, mx = ex.decode_slots(slots)
  assert mn.dtype == mx.dtype == np.float32
  assert np.array_equal(mn, np.array([p[0] for p in pairs], np.float32)) and np.array_equal(mx, np.array([p[1] for p in pairs], np.float32))


def _artefact(tmp_path):
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
  return path


def test_ranges_travel_with_the_artefact_and_stay_out_of_the_variables(tmp_path):
  path = _artefact(tmp_path)
  keys0 = sorted(np.load(path).files)
  assert not any(k.endswith('/act_range') for k in keys0) and ex.load_act_ranges(path) == {}
  vars0, (vars0b, raw0) = ex.load_exported(path), ex.load_codes(path)
  ranges = {'m/bn/Relu': (0.0, 5.25), 'm/bn_1/Relu6': (0.125, 6.0)}
  ex.write_act_ranges(path, ranges)
  keys1 = sorted(np.load(path).files)
  assert sorted(set(keys1) - set(keys0)) == ['m/bn/Relu/act_range', 'm/bn_1/Relu6/act_range'] and set(keys0) <= set(keys1)
  z = np.load(path)
  assert z['m/bn/Relu/act_range'].dtype == np.float32 and z['m/bn/Relu/act_range'].shape == (2,)
  vars1, (vars1b, raw1) = ex.load_exported(path), ex.load_codes(path)
  for a, b in ((vars0, vars1), (vars0b, vars1b)):
    assert sorted(a) == sorted(b) == ['m/bn/gamma', 'm/conv/kernel']
    assert all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a)
  assert list(raw0) == list(raw1) and all(np.array_equal(raw0[n][f], raw1[n][f]) for n in raw0 for f in raw0[n])
  assert ex.load_act_ranges(path) == ranges
  ex.write_act_ranges(path, {'m/bn/Relu': (0.0, 1.0)})                       # a second calibration replaces the first
  assert ex.load_act_ranges(path) == {'m/bn/Relu': (0.0, 1.0)}
  ex.write_act_ranges(path, {})
  assert sorted(np.load(path).files) == keys0                                # and without ranges the file has the keys it had
  bad = dict(np.load(path))
  bad['m/bn/Relu/act_range'] = np.zeros(3, np.float32)
  np.savez(path, **bad)
  with pytest.raises(ValueError, match='m/bn/Relu/act_range'):
    ex.load_act_ranges(path)


def test_malformed_ranges_raise_and_name_the_op_and_the_keyword_is_validated(tmp_path):
  from pocketflow_amd import inference
  graph = SimpleNamespace(activation_ops=[SimpleNamespace(type='Relu', name='m/a/Relu', index=0),
                                          SimpleNamespace(type='Relu6', name='m/b/Relu6', index=1)])
  good = {'m/a/Relu': (0.0, 1.0), 'm/b/Relu6': (0.5, 0.5)}
  inference._check_act_ranges('f.npz', graph, good)
  with pytest.raises(ValueError, match=r'f\.npz.*m/b/Relu6'):
    inference._check_act_ranges('f.npz', graph, {'m/a/Relu': (0.0, 1.0)})
  with pytest.raises(ValueError, match='m/c/Relu'):
    inference._check_act_ranges('f.npz', graph, dict(good, **{'m/c/Relu': (0.0, 1.0)}))
  for pair in ((0.0, float('inf')), (float('nan'), 1.0), (2.0, 1.0)):
    with pytest.raises(ValueError, match='m/a/Relu'):
      inference._check_act_ranges('f.npz', graph, dict(good, **{'m/a/Relu': pair}))
  with pytest.raises(ValueError, match="'batch' or 'static'"):
    inference.load_int8(None, str(tmp_path / 'missing.npz'), 'cpu', act_ranges='fixed')


def test_mobilenet_names_the_one_consumer_of_every_batch_norm():
  import pocketflow_amd.graph as G
  from pocketflow_amd.utils.external.mobilenet_v1 import MobilenetV1
  g = G.Graph('model', 'cpu')
  net = MobilenetV1(g, num_classes=11, depth_multiplier=0.25)
  bns = [(i, l) for i, l in enumerate(net.layers) if isinstance(l, G.BatchNormAct)]
  assert len(bns) == 27
  for i, bn in bns[:-1]:
    assert bn.consumer is net.layers[i + 1] and isinstance(bn.consumer, (G.Conv2D, G.DepthwiseConv2D))
  assert bns[-1][1].consumer is None and bns[-1][0] == len(net.layers) - 1
  # a BatchNorm in front of a depthwise layer may hand out codes, and that layer is its consumer
  assert all(isinstance(bn.consumer, G.DepthwiseConv2D) == bool(bn.codes_ok and not bn.lazy_ok) for _, bn in bns[:-1])
  assert g.act_static is None and g.requant_ran == set()
  assert isinstance(G.int8_pays_static(1, 512, 512, 1, None), bool) and isinstance(G.int8_dw_pays_static(512, 1, None), bool)


def _compile(tmp_path, name):
  hipcc = '/opt/rocm/bin/hipcc'
  if not os.path.exists(hipcc):
    pytest.skip('no hipcc')
  out = str(tmp_path / (name + '.s'))
  flags = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fhip-fp32-correctly-rounded-divide-sqrt', '-S',
           '--cuda-device-only']
  r = subprocess.run([hipcc] + flags + [os.path.join(ROOT, 'pocketflow_amd', 'csrc', name + '.hip'), '-o', out], capture_output=True,
                     text=True, timeout=600)
  assert r.returncode == 0, r.stderr[-2000:]
  seen = []
  for m in re.finditer(r'\.name:\s+(\S+)(.*?)\.wavefront_size', open(out).read(), re.S):
    kname, blk = m.group(1), m.group(2)
    vg = int(re.search(r'\.vgpr_count:\s+(\d+)', blk).group(1))
    sp = int(re.search(r'\.vgpr_spill_count:\s+(\d+)', blk).group(1))
    print(kname, vg, sp)
    assert sp == 0 and vg <= 256, (kname, vg, sp)
    seen.append(kname)
  return seen


def test_static_pass_kernels_compile_without_spills(tmp_path):
  """pf_act_static.hip: 2 input types x 3 output kinds x 3 activations x (vector, scalar) = 36 kernels."""
  seen = _compile(tmp_path, 'pf_act_static')
  assert len(seen) == 36 and all('k_bn_static' in n for n in seen)


def test_requantising_conv_kernels_compile_without_spills(tmp_path):
  """pf_conv_i8_q.hip: 3 output kinds x 3 activations = 9 kernels, and nothing else (the parent kernels stay in pf_conv_i8.hip)."""
  seen = _compile(tmp_path, 'pf_conv_i8_q')
  assert len(seen) == 9 and all('k_conv_i8_q' in n for n in seen)


def test_requantising_depthwise_kernels_compile_without_spills(tmp_path):
  """pf_depthwise_i8_q.hip: 3 output kinds x 2 strides x 3 activations = 18 kernels, and nothing else."""
  seen = _compile(tmp_path, 'pf_depthwise_i8_q')
  assert len(seen) == 18 and all('k_dw_i8_q' in n for n in seen)
