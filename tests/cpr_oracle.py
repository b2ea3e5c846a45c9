"""NumPy restatement of the 'chn-pruned-rmt' channel selection (reference learners/channel_pruning_rmt/learner.py), the CPU side of
tests/test_cpr_cpu.py and tests/test_cpr_kernels_gpu.py.  float64 where the reference computes in NumPy float64 (patches, feature
matrix, Gram), float32 per TF op where it runs a TF graph (ISTA, Adam); `dtype=np.float64` runs the same statements in float64 (the
noise floor of the least-squares bar)."""
import math

import numpy as np

BETA1, BETA2, EPS = 0.9, 0.999, 1e-8

try:
  from scipy.linalg import norm as _norm                                 # the reference's norm
except ImportError:                                                      # pragma: no cover
  _norm = np.linalg.norm


def same_pad(size, k, stride):
  """Leading pad of the reference sampler's 'SAME' formula (:666-671)."""
  p = max(k - (stride if size % stride == 0 else size % stride), 0)
  return p // 2


def gather(x, y, positions, kh, kw, stride, pad_t, pad_l):
  """x [B][H][W][C], y [B][OH][OW][Co] -> P [crops * B][kh * kw][C], Y [crops * B][Co] (float32), rows crop-major then batch; taps
  outside the image are zeros (:673-703)."""
  B, H, W, C = x.shape
  Ps, Ys = [], []
  for oh, ow in positions:
    p = np.zeros((B, kh, kw, C), np.float32)
    ih0, iw0 = oh * stride - pad_t, ow * stride - pad_l
    for i in range(kh):
      for j in range(kw):
        if 0 <= ih0 + i < H and 0 <= iw0 + j < W:
          p[:, i, j, :] = x[:, ih0 + i, iw0 + j, :]
    Ps.append(p.reshape(B, kh * kw, C))
    Ys.append(y[:, oh, ow, :].astype(np.float32))
  return np.concatenate(Ps, 0), np.concatenate(Ys, 0)


def gram(P, Y, idx, w_hwio):
  """(X^T X, X^T y) / ||X^T X||_F in float64 and cast to float32 (:741-766), X over the rows idx of P, with the reference's NumPy
  calls in its order (one float64 matmul per input channel, then X^T X, X^T y and the Frobenius norm)."""
  kh, kw, C, Co = w_hwio.shape
  Ps = P[idx].astype(np.float64)                                         # [n][kk][C]
  feat = np.zeros((C, len(idx) * Co))
  for c in range(C):
    feat[c] = np.matmul(Ps[:, :, c], np.reshape(w_hwio[:, :, c, :], [kh * kw, Co])).ravel()
  X = np.transpose(feat)                                                 # row n * Co + o
  y = np.reshape(Y[idx], [-1, 1])
  xtx = np.matmul(X.T, X)
  xty = np.matmul(X.T, y)
  nrm = _norm(xtx)
  return (xtx / nrm).astype(np.float32), (xty / nrm).astype(np.float32).reshape(-1), (xtx / nrm, (xty / nrm).reshape(-1))


def ista(A, b, m0, gamma, lr, iters, dtype=np.float32):
  """`iters` iterations of mask <- prox(mask - lr * (A mask - b), gamma * lr), one rounding per TF op (:449-462)."""
  f = dtype
  A, b, m = np.asarray(A, f), np.asarray(b, f).reshape(-1), np.asarray(m0, f).reshape(-1)
  lr_, thr = f(lr), f(f(gamma) * f(lr))
  for __ in range(iters):
    t = (A @ m).astype(f)
    t = (t - b).astype(f)
    t = (lr_ * t).astype(f)
    g = (m - t).astype(f)
    m = np.where(g > thr, g - thr, np.where(g < -thr, g + thr, f(0))).astype(f)
  return m


def bisect(solve, target):
  """The reference's gamma search (:788-813) over `solve(gamma) -> (mask, nnz)`; returns (mask, [(gamma, nnz), ...])."""
  path = []

  def run(x):
    mask, nnz = solve(x)
    path.append((x, nnz))
    return mask, nnz

  ubnd = 0.1
  while True:
    mask, nnz = run(ubnd)
    if nnz <= target:
      break
    ubnd *= 2.0
  lbnd = 0.0
  while nnz != target and ubnd - lbnd > 1e-8:
    val = (lbnd + ubnd) / 2.0
    mask, nnz = run(val)
    if nnz < target:
      ubnd = val
    elif nnz > target:
      lbnd = val
    else:
      break
  return mask, path


def lstsq(P, Y, w_hwio, keep, iters, lrn_rate, wd, dtype=np.float32):
  """The meta least-squares problem (:470-523, :819-841): Adam on W over X = P * mask; returns (W * mask as HWIO, losses before, after)."""
  f = dtype
  kh, kw, C, Co = w_hwio.shape
  N = P.shape[0]
  X = (P.astype(np.float64) * keep.reshape(1, 1, C)).reshape(N, -1).astype(f)
  Yf = Y.astype(f)
  W = w_hwio.reshape(-1, Co).astype(f)
  m, v = np.zeros_like(W), np.zeros_like(W)
  n = f(N)

  def losses():
    r = (X @ W).astype(f) - Yf
    return float(f(f(np.sum((r * r).astype(f), dtype=np.float64) / 2) / n)), float(f(f(wd) * f(np.sum(W.astype(np.float64) ** 2) / 2)))

  before = losses()
  c1, c2 = f(1.0 - BETA1), f(1.0 - BETA2)
  for step in range(1, iters + 1):
    r = ((X @ W).astype(f) - Yf).astype(f)
    g = ((X.T @ r).astype(f) / n).astype(f)
    g = (g + (f(wd) * W).astype(f)).astype(f)
    m = (f(BETA1) * m + c1 * g).astype(f)
    v = (f(BETA2) * v + c2 * (g * g)).astype(f)
    t = f(step)
    lr_t = f(f(lrn_rate) * np.sqrt(f(1.0) - np.power(f(BETA2), t)) / (f(1.0) - np.power(f(BETA1), t)))
    W = (W + ((-lr_t * m).astype(f) / (np.sqrt(v) + f(EPS))).astype(f)).astype(f)
  after = losses()
  return (W.reshape(kh, kw, C, Co) * keep.reshape(1, 1, C, 1)).astype(f), before, after


def secondary_size(N, Co):
  return int(math.ceil(min(N, N / Co * 10.0)))
