"""Host side of the int8 inference path: packing an exported layer for `pf_conv_i8_fwd` and the NumPy statement of what
that kernel computes.  No device work here.

The artefact of tools/conversion/export_quant_int8_model.py keeps every quantised kernel as unsigned codes d in [0, k_w] with
per-bucket (alpha, beta): w = beta + alpha * d / k_w.  A quantising BatchNormAct produces unsigned activation codes c in [0, k_a] with
one (alpha_a, beta_a) per tensor: a = beta_a + alpha_a * c / k_a.  Their convolution, taps outside the image contributing a = 0, is

    y[m][n] = (alpha_a/k_a)(alpha_w[n]/k_w) P + (alpha_a/k_a) beta_w[n] Sc + beta_a ((alpha_w[n]/k_w) Dv + beta_w[n] V)
    P  = sum_window c d        (padding positions hold code 0)
    Sc = sum_window c
    Dv = sum of d[n] over the positions INSIDE the image,  V = their number (valid taps * C)

`conv_reference` evaluates exactly this in int64 / float64 and is the executable definition of the layer.

A depthwise 3x3 layer (MobileNet-v1; `pf_dw_i8_fwd`) is the same expansion channel by channel, with the one (alpha_w, beta_w) a depthwise
kernel has and TensorFlow 'SAME' pads: `depthwise_reference`, `pack_depthwise`, `depthwise_supported`.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from pocketflow_amd.tools.conversion.export_quant_int8_model import MODE_CHANNEL, MODE_SPLIT, MODE_TENSOR, unpack_codes

K_STEP = 64          # bytes of the window one matrix instruction consumes: packed rows are padded to a multiple of it


def supported(C: int, N: int, R: int, S: int, stride: int) -> bool:
  """The rule of pf_conv_i8_supported, restated for hosts without the library (the tests compare the two over a grid)."""
  if min(C, N, R, S) <= 0 or stride not in (1, 2):
    return False
  return C % 16 == 0 and N % 8 == 0 and R * S * C * 2 ** 14 < 2 ** 31


def pack_layer(codes: np.ndarray, alpha: np.ndarray, beta: np.ndarray, meta: np.ndarray) -> Dict[str, np.ndarray]:
  """One exported Conv2D kernel (`<name>/codes|alpha|beta|meta` of the artefact; HWIO = [R][S][C][N]) in the form pf_conv_i8_fwd reads:
    w          int8  [N][Kp]   t = d - 128 in KRSC order, Kp = R*S*C rounded up to 64, zeros beyond R*S*C
    scale_beta f32   [N][2]    (alpha_w[n] / k_w, beta_w[n]); one bucket per tensor is repeated for every channel
    tsum       int32 [N]       sum over the window of t
    tapsum     int32 [N][R*S]  sum over the channels of d, per tap
    d          uint8 [N][R][S][C]  the unsigned codes (for conv_reference; not sent to the device)
  plus bits and the shape.  Raises ValueError for what the path does not cover: split buckets, more than 8 bits, a kernel that is
  not 4-D."""
  bits, mode = int(meta[0]), int(meta[1])
  shape = tuple(int(v) for v in meta[3:])
  if len(shape) != 4:
    raise ValueError('pack_layer: a Conv2D kernel is [R][S][C][N], got shape %s' % (shape,))
  if not 1 <= bits <= 8:
    raise ValueError('pack_layer: 1..8 bit codes only (got %d)' % bits)
  if mode == MODE_SPLIT:
    raise ValueError('pack_layer: split buckets cut across output channels and are not eligible')
  if mode not in (MODE_TENSOR, MODE_CHANNEL):
    raise ValueError('pack_layer: unknown bucket mode %d' % mode)
  R, S, C, N = shape
  alpha, beta = np.asarray(alpha, np.float32).reshape(-1), np.asarray(beta, np.float32).reshape(-1)
  nb = 1 if mode == MODE_TENSOR else N
  if alpha.size != nb or beta.size != nb:
    raise ValueError('pack_layer: %d (alpha, beta) pairs for %d buckets' % (alpha.size, nb))
  k = np.float32(2 ** bits - 1)
  d = unpack_codes(np.asarray(codes, np.uint8), bits, R * S * C * N).reshape(R, S, C, N)
  if int(d.max(initial=0)) > int(k):
    raise ValueError('pack_layer: a code exceeds 2^bits - 1')
  d = np.ascontiguousarray(np.transpose(d, (3, 0, 1, 2)))                       # KRSC
  K = R * S * C
  Kp = -(-K // K_STEP) * K_STEP
  w = np.zeros((N, Kp), np.int8)
  w[:, :K] = (d.reshape(N, K).astype(np.int16) - 128).astype(np.int8)
  scale_beta = np.empty((N, 2), np.float32)
  scale_beta[:, 0] = np.broadcast_to((alpha / k).astype(np.float32), (N,))
  scale_beta[:, 1] = np.broadcast_to(beta, (N,))
  return dict(w=w, scale_beta=scale_beta, tsum=w.astype(np.int32).sum(axis=1).astype(np.int32),
              tapsum=d.reshape(N, R * S, C).astype(np.int32).sum(axis=2).astype(np.int32), d=d, bits=bits,
              alpha=np.broadcast_to(alpha, (N,)).copy(), beta=np.broadcast_to(beta, (N,)).copy(), shape=(R, S, C, N))


def unpack_layer(p: Dict[str, np.ndarray]) -> np.ndarray:
  """The unsigned KRSC codes back from the signed padded rows of a packed layer."""
  R, S, C, N = p['shape']
  return (p['w'][:, :R * S * C].astype(np.int16) + 128).astype(np.uint8).reshape(N, R, S, C)


def out_size(H: int, R: int, stride: int, pad: int) -> int:
  return (H + 2 * pad - R) // stride + 1


def conv_reference(c: np.ndarray, alpha_a: float, beta_a: float, bits_a: int, d: np.ndarray, alpha_w: np.ndarray, beta_w: np.ndarray,
                   bits_w: int, stride: int, pad_h: int, pad_w: int, residual: Optional[np.ndarray] = None, terms: bool = False):
  """y[B][Ho][Wo][N] in float64 from activation codes c uint8 [B][H][W][C] and weight codes d uint8 [N][R][S][C], by the formula of the
  module docstring: P, Sc, Dv, V in int64, everything else float64.  alpha_w / beta_w: [N].  With terms=True also returns
  sum |terms| per output (the scale of the float32 rounding error of an implementation)."""
  c = np.asarray(c)
  d = np.asarray(d)
  B, H, W, C = c.shape
  N, R, S, Cd = d.shape
  assert C == Cd
  Ho, Wo = out_size(H, R, stride, pad_h), out_size(W, S, stride, pad_w)
  ka, kw = float(2 ** bits_a - 1), float(2 ** bits_w - 1)
  cp = np.zeros((B, H + 2 * pad_h, W + 2 * pad_w, C), np.int64)               # padding positions hold code 0
  cp[:, pad_h:pad_h + H, pad_w:pad_w + W] = c
  inside = np.zeros((H + 2 * pad_h, W + 2 * pad_w), np.int64)
  inside[pad_h:pad_h + H, pad_w:pad_w + W] = 1
  d64 = d.astype(np.int64)
  df = d.astype(np.float64)                                                    # products of integers below 2^53: a float64 matmul is exact
  dtap = d64.sum(axis=3)                                                       # [N][R][S]
  P = np.zeros((B, Ho, Wo, N), np.int64)
  Sc = np.zeros((B, Ho, Wo), np.int64)
  Dv = np.zeros((Ho, Wo, N), np.int64)
  V = np.zeros((Ho, Wo), np.int64)
  for r in range(R):
    for s in range(S):
      win = cp[:, r:r + (Ho - 1) * stride + 1:stride, s:s + (Wo - 1) * stride + 1:stride]       # [B][Ho][Wo][C]
      P += (win.astype(np.float64) @ df[:, r, s].T).astype(np.int64)
      Sc += win.sum(axis=3)
      ok = inside[r:r + (Ho - 1) * stride + 1:stride, s:s + (Wo - 1) * stride + 1:stride]     # [Ho][Wo]
      Dv += ok[:, :, None] * dtap[None, None, :, r, s]
      V += ok * C
  sa = float(alpha_a) / ka
  sw = np.asarray(alpha_w, np.float64).reshape(-1) / kw
  bw = np.asarray(beta_w, np.float64).reshape(-1)
  t1 = sa * sw * P
  t2 = sa * bw * Sc[..., None]
  t3a, t3b = float(beta_a) * (sw * Dv)[None], float(beta_a) * (bw * V[..., None])[None]
  y = t1 + t2 + (t3a + t3b)
  mag = np.abs(t1) + np.abs(t2) + np.abs(t3a) + np.abs(t3b)
  if residual is not None:
    y = y + np.asarray(residual, np.float64)
    mag = mag + np.abs(np.asarray(residual, np.float64))
  return (y, mag) if terms else y


# ---- depthwise 3x3 (pf_depthwise_i8.hip) ----------------------------------------------------------------------------------------

def depthwise_supported(C: int, k: int, stride: int) -> bool:
  """The rule of pf_dw_i8_supported, restated for hosts without the library (the tests compare the two over a grid)."""
  return C > 0 and C % 16 == 0 and k == 3 and stride in (1, 2)


def same_pads(size: int, k: int, stride: int):
  """TensorFlow 'SAME' (front, back) pads, as graph._same_pads computes them: the odd pixel goes behind."""
  out = -(-size // stride)
  total = max((out - 1) * stride + k - size, 0)
  return total // 2, total - total // 2


def pack_depthwise(codes: np.ndarray, alpha: np.ndarray, beta: np.ndarray, meta: np.ndarray) -> Dict[str, np.ndarray]:
  """One exported depthwise kernel (`<name>/codes|alpha|beta|meta`; reference shape [3][3][C][1]) in the form pf_dw_i8_fwd reads:
    wcol       uint32 [C][3]   column s of channel c: d[c][0][s] | d[c][1][s] << 8 | d[c][2][s] << 16
    scale_beta f32    [2]      (alpha_w / k_w, beta_w)
    d          uint8  [C][3][3]  the unsigned codes (for depthwise_reference; not sent to the device)
  plus bits, alpha, beta and the shape.  Raises ValueError for split buckets, more than 8 bits and a shape that is not (3, 3, C, 1)."""
  bits, mode = int(meta[0]), int(meta[1])
  shape = tuple(int(v) for v in meta[3:])
  if len(shape) != 4 or shape[:2] != (3, 3) or shape[3] != 1 or shape[2] <= 0:
    raise ValueError('pack_depthwise: a depthwise kernel is [3][3][C][1], got shape %s' % (shape,))
  if not 1 <= bits <= 8:
    raise ValueError('pack_depthwise: 1..8 bit codes only (got %d)' % bits)
  if mode == MODE_SPLIT:
    raise ValueError('pack_depthwise: split buckets are not eligible')
  if mode not in (MODE_TENSOR, MODE_CHANNEL):
    raise ValueError('pack_depthwise: unknown bucket mode %d' % mode)
  alpha, beta = np.asarray(alpha, np.float32).reshape(-1), np.asarray(beta, np.float32).reshape(-1)
  if alpha.size != 1 or beta.size != 1:                 # [3][3][C][1] has one output channel: one bucket in either mode
    raise ValueError('pack_depthwise: %d (alpha, beta) pairs for the one bucket of a depthwise kernel' % alpha.size)
  C = shape[2]
  k = np.float32(2 ** bits - 1)
  d = unpack_codes(np.asarray(codes, np.uint8), bits, 9 * C).reshape(3, 3, C)
  if int(d.max(initial=0)) > int(k):
    raise ValueError('pack_depthwise: a code exceeds 2^bits - 1')
  d = np.ascontiguousarray(np.transpose(d, (2, 0, 1)))                          # [C][r][s]
  d32 = d.astype(np.uint32)
  wcol = np.ascontiguousarray(d32[:, 0, :] | (d32[:, 1, :] << 8) | (d32[:, 2, :] << 16))
  return dict(wcol=wcol, scale_beta=np.array([alpha[0] / k, beta[0]], np.float32), d=d, bits=bits, alpha=float(alpha[0]),
              beta=float(beta[0]), shape=shape)


def unpack_depthwise(p: Dict[str, np.ndarray]) -> np.ndarray:
  """The unsigned [C][3][3] codes back from the column table of a packed depthwise kernel."""
  w = p['wcol']
  return np.stack([(w >> (8 * r)) & 0xFF for r in range(3)], axis=1).astype(np.uint8)


def depthwise_reference(c: np.ndarray, alpha_a: float, beta_a: float, bits_a: int, d: np.ndarray, alpha_w: float, beta_w: float,
                        bits_w: int, stride: int, terms: bool = False):
  """y[B][Ho][Wo][C] in float64 from activation codes c uint8 [B][H][W][C] and weight codes d uint8 [C][3][3] under TensorFlow 'SAME'
  pads: P, Sc, Dv, V in int64 over the taps INSIDE the image, everything else float64,
    y = (alpha_a/k_a)(alpha_w/k_w) P + (alpha_a/k_a) beta_w Sc + beta_a ((alpha_w/k_w) Dv + beta_w V).
  With terms=True also returns sum |terms| per output, as conv_reference does."""
  c = np.asarray(c)
  d = np.asarray(d)
  B, H, W, C = c.shape
  assert d.shape == (C, 3, 3)
  (ph, ph1), (pw, pw1) = same_pads(H, 3, stride), same_pads(W, 3, stride)
  Ho, Wo = -(-H // stride), -(-W // stride)
  ka, kw = float(2 ** bits_a - 1), float(2 ** bits_w - 1)
  cp = np.zeros((B, H + ph + ph1, W + pw + pw1, C), np.int64)                   # a tap outside the image adds nothing to any sum
  cp[:, ph:ph + H, pw:pw + W] = c
  inside = np.zeros((H + ph + ph1, W + pw + pw1), np.int64)
  inside[ph:ph + H, pw:pw + W] = 1
  d64 = d.astype(np.int64)
  P = np.zeros((B, Ho, Wo, C), np.int64)
  Sc = np.zeros((B, Ho, Wo, C), np.int64)
  Dv = np.zeros((Ho, Wo, C), np.int64)
  V = np.zeros((Ho, Wo), np.int64)
  for r in range(3):
    for s in range(3):
      win = cp[:, r:r + (Ho - 1) * stride + 1:stride, s:s + (Wo - 1) * stride + 1:stride]       # [B][Ho][Wo][C]
      ok = inside[r:r + (Ho - 1) * stride + 1:stride, s:s + (Wo - 1) * stride + 1:stride]       # [Ho][Wo]
      P += win * d64[:, r, s]
      Sc += win
      Dv += ok[:, :, None] * d64[None, None, :, r, s]
      V += ok
  sa, sw, bw = float(alpha_a) / ka, float(alpha_w) / kw, float(beta_w)
  t1 = sa * sw * P
  t2 = sa * bw * Sc
  t3a, t3b = float(beta_a) * (sw * Dv)[None], float(beta_a) * (bw * V[..., None])[None]
  y = t1 + t2 + (t3a + t3b)
  mag = np.abs(t1) + np.abs(t2) + np.abs(t3a) + np.abs(t3b)
  return (y, mag) if terms else y


# ---- fixed (calibrated) activation ranges: the static, clamping quantiser (pf_act_static.hip) -------------------------------------

def range_alpha_beta(mn, mx):
  """(alpha, beta) float32 as a slot holding (min, max) decodes: alpha = (max - min) + 1e-10f, beta = min (pf_common.h)."""
  mn, mx = np.float32(mn), np.float32(mx)
  return np.float32(np.float32(mx - mn) + np.float32(1e-10)), mn


def static_codes(u, alpha, beta, bits: int) -> np.ndarray:
  """uint8 codes of float32 values u under a FIXED range: the float32 chain of the device's quantiser, every operation rounded to
  float32 (the library is built without contraction, so this is bit for bit what the kernels compute),
    t = ((u - beta) / alpha) * k;  t = min(max(t, 0), k);  code = rint(t)   (half to even).
  It is the per-batch quantiser's chain plus the one clamp: a value outside the calibrated range takes the end code."""
  if not 1 <= int(bits) <= 8:
    raise ValueError('static_codes: 1..8 bits (got %s)' % bits)
  u = np.asarray(u, np.float32)
  alpha, beta, k = np.float32(alpha), np.float32(beta), np.float32(2 ** int(bits) - 1)
  with np.errstate(over='ignore', invalid='ignore'):
    t = ((u - beta).astype(np.float32) / alpha).astype(np.float32)
    t = (t * k).astype(np.float32)
  t = np.minimum(np.maximum(t, np.float32(0)), k)
  return np.rint(t).astype(np.uint8)


def static_value(code, alpha, beta, bits: int) -> np.ndarray:
  """The float32 value of a code: alpha * (code / k) + beta, multiply and then add, one float32 rounding each (the apply pass)."""
  alpha, beta, k = np.float32(alpha), np.float32(beta), np.float32(2 ** int(bits) - 1)
  q = (np.asarray(code).astype(np.float32) / k).astype(np.float32)
  return ((alpha * q).astype(np.float32) + beta).astype(np.float32)


def requant_reference(c: np.ndarray, alpha_a: float, beta_a: float, bits_a: int, d: np.ndarray, alpha_w, beta_w, bits_w: int, stride: int,
                      scale: np.ndarray, shift: np.ndarray, act: Optional[str], out_min: float, out_max: float, out_bits: int,
                      pad_h: Optional[int] = None, pad_w: Optional[int] = None):
  """A layer on codes followed by its consumer's folded BatchNorm, activation and static quantiser, in int64 / float64:
  y = conv_reference(...) for d of shape [N][R][S][C] (pads given) or depthwise_reference(...) for d of shape [C][3][3],
  u = act(scale * y + shift), t = clip((u - out_min) / (out_max - out_min + 1e-10) * k, 0, k), code = rint(t).
  Returns (codes int64, values float64) with value = alpha * code / k + out_min."""
  d = np.asarray(d)
  if d.ndim == 3:
    y = depthwise_reference(c, alpha_a, beta_a, bits_a, d, float(np.asarray(alpha_w).reshape(-1)[0]),
                            float(np.asarray(beta_w).reshape(-1)[0]), bits_w, stride)
  else:
    y = conv_reference(c, alpha_a, beta_a, bits_a, d, alpha_w, beta_w, bits_w, stride, pad_h, pad_w)
  u = np.asarray(scale, np.float64) * y + np.asarray(shift, np.float64)
  if act == 'Relu':
    u = np.maximum(u, 0.0)
  elif act == 'Relu6':
    u = np.clip(u, 0.0, 6.0)
  k = float(2 ** int(out_bits) - 1)
  alpha = (float(out_max) - float(out_min)) + 1e-10
  codes = np.rint(np.clip((u - float(out_min)) / alpha * k, 0.0, k)).astype(np.int64)
  return codes, alpha * (codes / k) + float(out_min)
