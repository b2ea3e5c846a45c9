"""pf_conv_gather.hip (the forward convolution of a shrunk channel-pruned layer: reduction over the kept input channels only) through
the C ABI (pocketflow_amd/hip.py), float32 and bf16, against a float64 convolution of the gathered input on the same
(storage-rounded) operands.  Bars: the project's own for this class of kernel (tests/test_convg_gpu.py): max |err| / max |ref| at most
2e-5 in float32 and 6e-3 with bf16 storage."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 2e-5, torch.bfloat16: 6e-3}
IMGS, H, W = 2, 13, 11
# (R, stride, pad)
GEOMS = [(1, 1, 0), (1, 2, 0), (3, 1, 1), (3, 2, 1)]
CHANNELS = [(3, 2), (16, 1), (64, 37), (64, 63), (256, 128), (512, 384), (2048, 1024)]
NS = [10, 64, 256]
CASES = [(R, s, p, C, Ck, N) for (R, s, p) in GEOMS for (C, Ck) in CHANNELS for N in NS]
CASES += [(7, 2, 3, 3, 2, N) for N in NS]                       # the 7x7 / 2 stem, 3 -> 2 kept channels


def _ref64(xg, w, stride, pad):
  """float64 convolution as im2col + matmul on the device.  xg: [B][Ck][H][W], w: [N][Ck][R][R] -> [B][N][Ho][Wo]."""
  B, _, Hh, Ww = xg.shape
  N, _, R, _ = w.shape
  Ho, Wo = (Hh + 2 * pad - R) // stride + 1, (Ww + 2 * pad - R) // stride + 1
  cols = F.unfold(xg.double(), R, padding=pad, stride=stride)            # [B][Ck*R*R][Ho*Wo]
  return torch.matmul(w.double().reshape(N, -1), cols).reshape(B, N, Ho, Wo)


def _act(y, act):
  if act == 'Relu':
    return y.clamp_min(0)
  if act == 'Relu6':
    return y.clamp(0, 6)
  return y


def _err(got, ref):
  got, ref = got.double(), ref.double()
  assert torch.isfinite(got).all()
  return float((got - ref).abs().max()) / (float(ref.abs().max()) + 1e-30)


def _dense(hip, xs, wfull_krsc, y, C, N, R, stride, pad, Ho, Wo):
  """An existing dense forward kernel that takes the shape, on the zero-filled full-shape kernel (the MFMA kernels where their channel
  limits allow, else k_convg; not necessarily the one graph.Conv2D would pick)."""
  if xs.dtype == torch.bfloat16 and R == 1 and C % 8 == 0 and N % 8 == 0:
    geom = None if stride == 1 else (Ho, Wo, H, W, stride)
    hip.conv1x1_fwd(xs, wfull_krsc.reshape(N, C), y, IMGS * Ho * Wo, N, C, geom=geom)
  elif xs.dtype == torch.bfloat16 and R > 1 and C % 64 == 0 and N % 8 == 0:
    hip.conv2d_fwd(xs, wfull_krsc, y, IMGS, H, W, C, N, R, R, stride, pad, pad, Ho, Wo)
  else:
    hip.convg_fwd(xs, wfull_krsc, None, y, IMGS, H, W, C, N, R, R, stride, pad, pad, Ho, Wo)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['float32', 'bfloat16'])
@pytest.mark.parametrize('R,stride,pad,C,Ck,N', CASES)
def test_conv_gather_forward(dtype, R, stride, pad, C, Ck, N):
  from pocketflow_amd import hip
  tol = TOL[dtype]
  g = torch.Generator(device='cpu').manual_seed(99 + 7 * C + 3 * N + R + stride)
  rs = np.random.RandomState(C * 31 + Ck)
  gather_np = hip.check_gather(np.sort(rs.permutation(C)[:Ck]), C, Ck)
  gather = torch.from_numpy(gather_np).cuda()
  gl = gather.long()
  Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
  x = torch.randn((IMGS, C, H, W), generator=g).cuda().contiguous(memory_format=torch.channels_last)
  w = (torch.randn((N, Ck, R, R), generator=g) / float(np.sqrt(Ck * R * R))).cuda()
  bias = torch.randn((N,), generator=g).cuda()
  res = torch.randn((IMGS, N, Ho, Wo), generator=g).cuda().contiguous(memory_format=torch.channels_last).to(dtype)
  ss = torch.stack([torch.rand((N,), generator=g) * 4 + 0.5, torch.randn((N,), generator=g) * 2 + 1]).cuda().contiguous()
  xs, ws = x.to(dtype), w.to(dtype)
  wk = ws.permute(0, 2, 3, 1).contiguous()                                  # [N][R][S][Ck]
  ref = _ref64(xs[:, gl], ws, stride, pad)

  def run(xin, **kw):
    y = torch.full((IMGS, N, Ho, Wo), float('nan'), dtype=dtype, device='cuda').contiguous(memory_format=torch.channels_last)
    hip.conv_gather_fwd(xin, wk, gather, y, IMGS, H, W, C, N, R, R, stride, pad, pad, Ho, Wo, **kw)
    return y

  y0 = run(xs)
  e = _err(y0, ref)
  assert e <= tol, 'no epilogue: max |err| / max |ref| = %.3e' % e
  # two calls on the same inputs: identical bits
  assert torch.equal(y0, run(xs))
  # dropped channels never reach Y: NaN there (a multiply by a zero weight would spread it)
  drop = torch.ones(C, dtype=torch.bool, device='cuda')
  drop[gl] = False
  xn = xs.clone()
  xn[:, drop] = float('nan')
  assert torch.equal(y0, run(xn.contiguous(memory_format=torch.channels_last)))
  # each epilogue alone
  e = _err(run(xs, bias=bias), ref + bias.double().view(1, N, 1, 1))
  assert e <= tol, 'bias: %.3e' % e
  e = _err(run(xs, residual=res), ref + res.double())
  assert e <= tol, 'residual: %.3e' % e
  for act in (None, 'Relu', 'Relu6'):
    want = _act(ref * ss[0].double().view(1, N, 1, 1) + ss[1].double().view(1, N, 1, 1), act)
    e = _err(run(xs, scale_shift=ss, act=act), want)
    assert e <= tol, 'scale_shift + %s: %.3e' % (act, e)
  # the dense inference kernel on the zero-filled kernel: both within the bar of float64, so within twice the bar of each other
  wfull = torch.zeros((N, R, R, C), dtype=dtype, device='cuda')
  wfull[:, :, :, gl] = wk
  yd = torch.full_like(y0, float('nan'))
  _dense(hip, xs, wfull, yd, C, N, R, stride, pad, Ho, Wo)
  ed = _err(yd, ref)
  e = _err(y0, yd.double())
  assert ed <= tol and e <= 2 * tol, 'dense kernel vs float64 %.3e, gather vs dense %.3e' % (ed, e)


def test_conv_gather_binding_rejects_bad_operands():
  from pocketflow_amd import hip
  with pytest.raises(ValueError):
    hip.check_gather(np.array([0, 2, 2], dtype=np.int32), 8, 3)
  with pytest.raises(ValueError):
    hip.check_gather(np.array([0, 8], dtype=np.int32), 8, 2)
  x = torch.zeros((1, 8, 4, 4), device='cuda').contiguous(memory_format=torch.channels_last)
  wk = torch.zeros((4, 1, 1, 2), device='cuda')
  y = torch.zeros((1, 4, 4, 4), device='cuda').contiguous(memory_format=torch.channels_last)
  gather = torch.tensor([1, 5], dtype=torch.int32, device='cuda')
  with pytest.raises(TypeError):
    hip.conv_gather_fwd(x, wk.bfloat16(), gather, y, 1, 4, 4, 8, 4, 1, 1, 1, 0, 0, 4, 4)
  with pytest.raises(ValueError):
    hip.conv_gather_fwd(x, wk, gather, y, 1, 4, 4, 8, 8, 1, 1, 1, 0, 0, 4, 4)
  hip.conv_gather_fwd(x, wk, gather, y, 1, 4, 4, 8, 4, 1, 1, 1, 0, 0, 4, 4)
  torch.cuda.synchronize()
