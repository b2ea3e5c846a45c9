"""Host side of the int8 depthwise route: the layer formula (int8.depthwise_reference) against a float64 grouped convolution of the
decoded operands under TensorFlow 'SAME' pads, the exact integer sums, packing, eligibility, the register budget of the compiled
kernels, and MobileNet-v1's wiring.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pocketflow_amd import int8
from pocketflow_amd.tools.conversion import export_quant_int8_model as ex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (5, 7), (8, 6), (9, 4)]


def _operands(rng, H, W, C=16, bits_a=8, bits_w=8, B=2):
  c = rng.integers(0, 2 ** bits_a, size=(B, H, W, C), dtype=np.int64).astype(np.uint8)
  d = rng.integers(0, 2 ** bits_w, size=(C, 3, 3), dtype=np.int64).astype(np.uint8)
  return c, d


def _depthwise64(a, w, stride):
  """float64 F.conv2d(groups=C) of a [B][H][W][C] with w [C][3][3] under 'SAME' pads (zeros outside the image) -> [B][Ho][Wo][C]."""
  from pocketflow_amd.graph import _same_pads
  B, H, W, C = a.shape
  ph, pw = _same_pads(H, 3, stride), _same_pads(W, 3, stride)
  x = F.pad(torch.from_numpy(a).permute(0, 3, 1, 2), (pw[0], pw[1], ph[0], ph[1]))
  y = F.conv2d(x, torch.from_numpy(w).reshape(C, 1, 3, 3), None, stride=stride, groups=C)
  return y.permute(0, 2, 3, 1).numpy()


def test_same_pads_are_the_graphs():
  from pocketflow_amd.graph import _same_pads
  for size in range(1, 20):
    for stride in (1, 2):
      assert int8.same_pads(size, 3, stride) == _same_pads(size, 3, stride)
  assert int8.same_pads(8, 3, 2) == (0, 1) and int8.same_pads(9, 3, 2) == (1, 1)          # asymmetric on even sizes


@pytest.mark.parametrize('bits', [8, 4])
@pytest.mark.parametrize('beta_a', [0.0, 0.37])
@pytest.mark.parametrize('H,W', SIZES)
@pytest.mark.parametrize('stride', [1, 2])
def test_depthwise_reference_is_the_convolution_of_the_decoded_operands(stride, H, W, beta_a, bits):
  rng = np.random.default_rng(1000 * stride + 100 * H + W + bits + int(beta_a * 100))
  c, d = _operands(rng, H, W, bits_a=bits, bits_w=bits)
  k = float(2 ** bits - 1)
  alpha_a, alpha_w, beta_w = 2.71, 0.43, -0.19
  a = beta_a + alpha_a * c.astype(np.float64) / k
  w = beta_w + alpha_w * d.astype(np.float64) / k
  want = _depthwise64(a, w, stride)
  got, mag = int8.depthwise_reference(c, alpha_a, beta_a, bits, d, alpha_w, beta_w, bits, stride, terms=True)
  assert got.shape == want.shape == (2, -(-H // stride), -(-W // stride), 16)
  assert np.all(np.abs(got - want) <= 1e-12 * mag), float((np.abs(got - want) / mag).max())
  assert np.array_equal(got, int8.depthwise_reference(c, alpha_a, beta_a, bits, d, alpha_w, beta_w, bits, stride))


@pytest.mark.parametrize('H,W', SIZES)
@pytest.mark.parametrize('stride', [1, 2])
def test_exact_sums(stride, H, W):
  """Scales 1 (alpha = k, beta = 0): y = P, the integer sum of code * d over the taps inside the image; alpha_w = 0, beta_w = 1: y = Sc."""
  rng = np.random.default_rng(7 + stride + H * W)
  c, d = _operands(rng, H, W)
  ph, pw = int8.same_pads(H, 3, stride)[0], int8.same_pads(W, 3, stride)[0]
  Ho, Wo = -(-H // stride), -(-W // stride)
  P = np.zeros((2, Ho, Wo, 16), np.int64)
  Sc = np.zeros((2, Ho, Wo, 16), np.int64)
  for ho in range(Ho):
    for wo in range(Wo):
      for r in range(3):
        for s in range(3):
          hi, wi = ho * stride + r - ph, wo * stride + s - pw
          if 0 <= hi < H and 0 <= wi < W:
            P[:, ho, wo] += c[:, hi, wi].astype(np.int64) * d[:, r, s].astype(np.int64)
            Sc[:, ho, wo] += c[:, hi, wi]
  y = int8.depthwise_reference(c, 255.0, 0.0, 8, d, 255.0, 0.0, 8, stride)
  assert np.array_equal(y, np.rint(y)) and np.array_equal(y.astype(np.int64), P) and P.max() < 2 ** 24
  y = int8.depthwise_reference(c, 255.0, 0.0, 8, d, 0.0, 1.0, 8, stride)
  assert np.array_equal(y.astype(np.int64), Sc)


@pytest.mark.parametrize('mode', [ex.MODE_TENSOR, ex.MODE_CHANNEL])
@pytest.mark.parametrize('bits', [4, 8])
def test_pack_depthwise_round_trips(mode, bits):
  rng = np.random.default_rng(bits + mode)
  C = 48
  d_hwio = rng.integers(0, 2 ** bits, size=(3, 3, C, 1)).astype(np.uint8)
  alpha, beta = np.array([0.37], np.float32), np.array([-0.21], np.float32)
  meta = np.array([bits, mode, 0, 3, 3, C, 1], np.int64)
  p = int8.pack_depthwise(ex.pack_codes(d_hwio.reshape(-1), bits), alpha, beta, meta)
  crs = np.transpose(d_hwio[..., 0], (2, 0, 1))
  assert p['wcol'].dtype == np.uint32 and p['wcol'].shape == (C, 3) and p['d'].dtype == np.uint8
  assert np.array_equal(p['d'], crs) and np.array_equal(int8.unpack_depthwise(p), crs)
  assert p['wcol'][5, 2] == int(crs[5, 0, 2]) | int(crs[5, 1, 2]) << 8 | int(crs[5, 2, 2]) << 16
  k = np.float32(2 ** bits - 1)
  assert p['scale_beta'].dtype == np.float32 and np.array_equal(p['scale_beta'], np.array([alpha[0] / k, beta[0]], np.float32))
  assert p['bits'] == bits and p['shape'] == (3, 3, C, 1)
  dec = ex.decode_tensor(ex.pack_codes(d_hwio.reshape(-1), bits), alpha, beta, meta)
  assert np.allclose(np.transpose(dec[..., 0], (2, 0, 1)), p['beta'] + p['alpha'] * crs / float(k), rtol=1e-6, atol=1e-7)


def test_pack_depthwise_rejects_what_the_path_does_not_cover():
  codes = ex.pack_codes(np.zeros(9 * 16, np.uint8), 8)
  one = np.ones(1, np.float32)
  with pytest.raises(ValueError, match='split'):
    int8.pack_depthwise(codes, one, one, np.array([8, ex.MODE_SPLIT, 64, 3, 3, 16, 1]))
  with pytest.raises(ValueError, match='bit'):
    int8.pack_depthwise(codes, one, one, np.array([9, ex.MODE_TENSOR, 0, 3, 3, 16, 1]))
  for shape in ([3, 3, 16, 2], [5, 5, 16, 1], [3, 3, 16], [1, 1, 16, 8]):
    with pytest.raises(ValueError, match='depthwise kernel is'):
      int8.pack_depthwise(codes, one, one, np.array([8, ex.MODE_TENSOR, 0] + shape))
  with pytest.raises(ValueError, match='pairs'):
    int8.pack_depthwise(codes, np.ones(16, np.float32), np.ones(16, np.float32), np.array([8, ex.MODE_CHANNEL, 0, 3, 3, 16, 1]))


def test_supported_grid_matches_the_library():
  from pocketflow_amd import hip
  for C in (0, 3, 8, 16, 24, 32, 48, 64, 1000, 1024, 4112, 8192):
    for k in (1, 3, 5):
      for stride in (0, 1, 2, 3):
        want = C > 0 and C % 16 == 0 and k == 3 and stride in (1, 2)
        assert hip.dw_i8_supported(C, k, stride) == want == int8.depthwise_supported(C, k, stride), (C, k, stride)


def test_depthwise_i8_kernels_compile_without_spills(tmp_path):
  """pf_depthwise_i8.hip for gfx950: no kernel of the file may spill vector registers or need more than 256 of them."""
  hipcc = '/opt/rocm/bin/hipcc'
  if not os.path.exists(hipcc):
    pytest.skip('no hipcc')
  out = str(tmp_path / 'pf_depthwise_i8.s')
  flags = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fhip-fp32-correctly-rounded-divide-sqrt', '-S',
           '--cuda-device-only']
  r = subprocess.run([hipcc] + flags + [os.path.join(ROOT, 'pocketflow_amd', 'csrc', 'pf_depthwise_i8.hip'), '-o', out],
                     capture_output=True, text=True, timeout=600)
  assert r.returncode == 0, r.stderr[-2000:]
  seen = []
  for m in re.finditer(r'\.name:\s+(\S+)(.*?)\.wavefront_size', open(out).read(), re.S):
    name, blk = m.group(1), m.group(2)
    vg = int(re.search(r'\.vgpr_count:\s+(\d+)', blk).group(1))
    sp = int(re.search(r'\.vgpr_spill_count:\s+(\d+)', blk).group(1))
    print(name, vg, sp)
    assert sp == 0 and vg <= 256, (name, vg, sp)
    seen.append(name)
  assert sum('k_dw_i8' in n for n in seen) == 4                       # float32 / bf16 output x stride 1 / 2


def test_mobilenet_wiring():
  """Every BatchNormAct a depthwise layer reads may hand out codes, the last one (it feeds the average pool) may not, and
  DepthwiseConv2D carries the slot the loader fills."""
  from pocketflow_amd import graph as G
  from pocketflow_amd.utils.external.mobilenet_v1 import MobilenetV1
  g = G.Graph('model', 'cpu', torch.float32)
  with g.as_default():
    net = MobilenetV1(g, num_classes=11, depth_multiplier=0.5)
  layers = net.layers
  dws = [i for i, l in enumerate(layers) if isinstance(l, G.DepthwiseConv2D)]
  assert len(dws) == 13 and g.depthwise_layers == [layers[i] for i in dws]
  for i in dws:
    assert isinstance(layers[i - 1], G.BatchNormAct) and layers[i - 1].codes_ok, i
    assert isinstance(layers[i + 1], G.BatchNormAct) and layers[i + 1].codes_ok          # read by the pointwise convolution alone
  assert isinstance(layers[-1], G.BatchNormAct) and not layers[-1].codes_ok
  assert all(hasattr(dw, 'int8') and dw.int8 is None for dw in g.depthwise_layers)
