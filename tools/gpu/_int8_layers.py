"""What int8_conv_layers.py and int8_depthwise_layers.py share: a packed layer with random 8-bit codes next to its decoded bf16 twin
(the two routes multiply the same numbers), channels-last buffers, and the alternating-rounds timing loop."""
import numpy as np
import torch
from _timing import gpu_time_us
from pocketflow_amd import int8
from pocketflow_amd.tools.conversion import export_quant_int8_model as ex


def nhwc(shape, dtype):
  return torch.empty(shape, dtype=dtype, device='cuda').contiguous(memory_format=torch.channels_last)


def conv_layer(k: int, C: int, N: int):
  """(decoded kernel bf16 [N][k][k][C], (w, scale_beta, tsum, tapsum) of int8.pack_layer) on the device; channel buckets, seed C + N."""
  rng = np.random.RandomState(C + N)
  d = rng.randint(0, 256, size=(k, k, C, N)).astype(np.uint8)
  alpha, beta = rng.uniform(0.05, 0.6, N).astype(np.float32), -rng.uniform(0.02, 0.3, N).astype(np.float32)
  meta = np.array([8, ex.MODE_CHANNEL, 0, k, k, C, N], np.int64)
  p = int8.pack_layer(ex.pack_codes(d.reshape(-1), 8), alpha, beta, meta)
  wdec = ex.decode_tensor(ex.pack_codes(d.reshape(-1), 8), alpha, beta, meta)
  wfull = torch.from_numpy(np.ascontiguousarray(wdec.transpose(3, 0, 1, 2))).cuda().bfloat16()
  return wfull, tuple(torch.from_numpy(np.ascontiguousarray(p[key])).cuda() for key in ('w', 'scale_beta', 'tsum', 'tapsum'))


def depthwise_layer(C: int, stride: int):
  """(decoded kernel bf16 [C][3][3], wcol, scale_beta of int8.pack_depthwise) on the device; seed C + stride."""
  rng = np.random.RandomState(C + stride)
  d = rng.randint(0, 256, size=(3, 3, C, 1)).astype(np.uint8)
  alpha, beta = rng.uniform(0.05, 0.6, 1).astype(np.float32), -rng.uniform(0.02, 0.3, 1).astype(np.float32)
  meta = np.array([8, ex.MODE_TENSOR, 0, 3, 3, C, 1], np.int64)
  p = int8.pack_depthwise(ex.pack_codes(d.reshape(-1), 8), alpha, beta, meta)
  wdec = ex.decode_tensor(ex.pack_codes(d.reshape(-1), 8), alpha, beta, meta)
  wcrs = torch.from_numpy(np.ascontiguousarray(wdec[..., 0].transpose(2, 0, 1))).cuda().bfloat16()
  return wcrs, torch.from_numpy(p['wcol'].view(np.int32)).cuda(), torch.from_numpy(p['scale_beta']).cuda()


def time_rounds(fns, rounds: int):
  """fns: (key, launch) pairs, timed one after the other in each of `rounds` rounds (so the routes alternate).  Returns
  ({key: best round, us}, {key: max - min over the rounds})."""
  t = {key: [] for key, _ in fns}
  for _ in range(rounds):
    for key, fn in fns:
      t[key].append(gpu_time_us(fn))
  return {key: min(v) for key, v in t.items()}, {key: max(v) - min(v) for key, v in t.items()}
