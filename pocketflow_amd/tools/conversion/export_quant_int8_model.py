"""Export the INTEGER form of a uniformly quantised model (the step AFTER the path).

The reference ships quantised models through TF-Lite (tools/conversion/export_quant_tflite_model.py:196-249: freeze the
graph, hand it to the TF-Lite converter) -- for its `uniform-tf` learner only, whose fake-quant nodes the converter
understands; the UniformQuantLearner of the hot path (learners/uniform_quantization) keeps float32 master weights in its
checkpoints and has no integer artefact at all.  This tool gives it one, defined by the learner's OWN quantiser
(`__uniform_quantize`, learners/uniform_quantization/utils.py:163-245): for every quantised matmul kernel

    alpha = max - min + 1e-10,  beta = min        per tensor / per output channel / per (strided) split bucket
    code  = round((w - beta) / alpha * k)         k = 2^bits - 1, an integer in [0, k]
    w_q   = alpha * (code / k) + beta             float32, mul then add: the reference's __inv_scale, bit for bit

so `decode_tensor` reproduces the fake-quantised weights the training graph multiplied with EXACTLY, and a model restored
from the artefact evaluates identically (re-quantising a quantised tensor is the identity).  Where the numbers come from:
alpha / beta and the fake-quantised weights are taken from the device kernels the learner trains with (`pf_seg_minmax`,
`pf_seg_uq_apply`, float32), the codes are read back from them and every tensor is verified to round-trip bit-exactly
before it is written -- there is no second implementation of the quantiser here.

Artefact: one `.npz` -- per quantised kernel `<name>/codes` (bit-packed, `bits` per weight, HWIO order like the reference's
checkpoints), `<name>/alpha`, `<name>/beta` (float32, one per bucket), `<name>/meta` = [bits, bucket mode, bucket size, *shape];
every other variable as float32 -- plus `export_summary.json` (bytes before / after per tensor, incl. the 2 x 32 bits per
bucket the reference accounts for, uq utils.py:299-306).  With `--calib_batches N` (N > 0) the file also carries one float32
`<activation op name>/act_range` = [min, max] per Relu / Relu6 op: the range of that activation over N evaluation batches
(`calibrate_act_ranges`), which `inference.load_int8(act_ranges='static')` quantises against instead of recalibrating per batch.

    python -m pocketflow_amd.tools.conversion.export_quant_int8_model --model_name resnet --dataset_name ilsvrc_12 \\
        --uql_weight_bits 8 [--uql_use_buckets --uql_bucket_type channel]      # reads uql_save_quant_model_path (needs the GPU)
"""
from __future__ import annotations

import json
import logging
import os
from typing import Dict, Tuple

import numpy as np

log = logging.getLogger('pocketflow_amd')

MODE_TENSOR, MODE_CHANNEL, MODE_SPLIT = 0, 1, 2
ACT_RANGE_SUFFIX = '/act_range'


def _bucket_index(shape, mode: int, bucket_size: int) -> np.ndarray:
  """Bucket of every element of an HWIO-ordered tensor, flattened: whole tensor | output channel (the last axis of
  reshape(w, [-1, cout]), uq utils.py:277-289) | the COLUMN of reshape(padded flat, [bucket_size, multiple]) with multiple =
  ceil(n / bucket_size) buckets (:247-275) -- a 'split' bucket is the strided set {flat[i * multiple + j]}_i."""
  n = int(np.prod(shape))
  if mode == MODE_TENSOR:
    return np.zeros(n, np.int64)
  if mode == MODE_CHANNEL:
    return np.tile(np.arange(shape[-1], dtype=np.int64), n // shape[-1])
  return np.arange(n, dtype=np.int64) % (-(-n // bucket_size))


def pack_codes(codes: np.ndarray, bits: int) -> np.ndarray:
  """`bits` per code, little-endian bit order, padded to a whole byte."""
  b = ((codes.reshape(-1, 1).astype(np.uint8) >> np.arange(bits, dtype=np.uint8)) & 1).astype(np.uint8)
  return np.packbits(b.reshape(-1), bitorder='little')


def unpack_codes(packed: np.ndarray, bits: int, n: int) -> np.ndarray:
  b = np.unpackbits(packed, bitorder='little')[:n * bits].reshape(n, bits).astype(np.uint16)
  return (b << np.arange(bits, dtype=np.uint16)).sum(axis=1).astype(np.uint8)


def decode_tensor(packed: np.ndarray, alpha: np.ndarray, beta: np.ndarray, meta: np.ndarray) -> np.ndarray:
  """The executable definition of the format: float32 HWIO tensor from codes + per-bucket (alpha, beta)."""
  bits, mode, bucket_size = int(meta[0]), int(meta[1]), int(meta[2])
  shape = tuple(int(v) for v in meta[3:])
  n = int(np.prod(shape))
  codes = unpack_codes(packed, bits, n).astype(np.float32)
  k = np.float32(np.int64(2) ** np.int64(bits) - np.int64(1))
  idx = _bucket_index(shape, mode, bucket_size)
  q = (codes / k).astype(np.float32)
  return ((alpha.astype(np.float32)[idx] * q).astype(np.float32) + beta.astype(np.float32)[idx]).astype(np.float32).reshape(shape)


def encode_tensor(wq: np.ndarray, alpha: np.ndarray, beta: np.ndarray, bits: int, mode: int,
                  bucket_size: int) -> Tuple[np.ndarray, np.ndarray]:
  """Codes of an already fake-quantised HWIO tensor `wq` under the quantiser's own (alpha, beta); raises unless
  decode(encode(wq)) == wq bit for bit."""
  if not 1 <= bits <= 8:
    raise ValueError('integer export covers 1..8 bits (got %d)' % bits)
  shape = wq.shape
  idx = _bucket_index(shape, mode, bucket_size)
  k = float(2 ** bits - 1)
  a, b = alpha.astype(np.float64)[idx], beta.astype(np.float64)[idx]
  codes = np.clip(np.rint((wq.reshape(-1).astype(np.float64) - b) / a * k), 0, k).astype(np.uint8)
  meta = np.array([bits, mode, bucket_size] + list(shape), np.int64)
  packed = pack_codes(codes, bits)
  back = decode_tensor(packed, alpha, beta, meta)
  if not np.array_equal(back.view(np.uint32), np.ascontiguousarray(wq, np.float32).view(np.uint32)):
    bad = int((back != wq).sum())
    raise ValueError('%d of %d weights do not round-trip through their integer codes' % (bad, wq.size))
  return packed, meta


def export_from_learner(learner, path: str) -> Dict:
  """Artefact of a UniformQuantLearner in its current state (rank 0).  Returns the summary dict."""
  import torch
  g = learner.graph
  st, plan, uq = g.store, learner.uni_quant.plan, learner.uni_quant
  qw = torch.empty_like(st.w_master)                      # float32 fake-quantised copy, whatever the compute dtype is
  plan.uniform_quantize(st.w_master, qw)
  ab = plan.alpha_beta().cpu().numpy()
  qw = qw.cpu().numpy()
  seg_bits = plan.segs_host['bits']
  out, rows = {}, []
  quantised = set()
  for s, (v, w) in enumerate(zip(uq._all_vars, plan.weights)):
    bits = int(seg_bits[s])
    if bits <= 0 or bits > 8:
      continue
    nb, so = plan.n_buckets[s], plan.slot_offsets[s]
    if not plan.use_buckets or nb == 1 and plan.bucket_type == 'channel':
      mode = MODE_TENSOR
    else:
      mode = MODE_CHANNEL if plan.bucket_type == 'channel' else MODE_SPLIT
    wq = v.to_ref(qw[v.offset:v.offset + v.numel])
    packed, meta = encode_tensor(wq, ab[so:so + nb, 0], ab[so:so + nb, 1], bits, mode, int(plan.bucket_size))
    out[v.name + '/codes'], out[v.name + '/alpha'], out[v.name + '/beta'] = packed, ab[so:so + nb, 0].copy(), ab[so:so + nb, 1].copy()
    out[v.name + '/meta'] = meta
    quantised.add(v.name)
    rows.append(dict(name=v.name, bits=bits, buckets=int(nb), float32_bytes=int(wq.size * 4),
                     int_bytes=int(packed.nbytes + nb * 8)))
  for name, val in st.export_numpy().items():
    if name not in quantised:
      out[name] = np.asarray(val, np.float32)
  os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
  np.savez(path, **out)
  f32 = sum(r['float32_bytes'] for r in rows)
  summ = dict(quantised_tensors=len(rows), float32_bytes=f32, int_bytes=sum(r['int_bytes'] for r in rows),
              other_float32_bytes=int(sum(v.nbytes for k, v in out.items() if k.split('/')[-1] not in ('codes', 'alpha', 'beta', 'meta'))),
              layers=rows)
  with open(os.path.join(os.path.dirname(os.path.abspath(path)), 'export_summary.json'), 'w') as f:
    json.dump(summ, f, indent=1)
  log.info('integer model written to %s: %d tensors, %.2f MB -> %.2f MB', path, len(rows), f32 / 1e6, summ['int_bytes'] / 1e6)
  return summ


def load_exported(path: str) -> Dict[str, np.ndarray]:
  """{variable name: float32 array} with every quantised kernel decoded: what `restore_vars` / `load_numpy` take."""
  z = np.load(path)
  out, done = {}, set()
  for key in z.files:
    if key.endswith('/codes'):
      name = key[:-len('/codes')]
      out[name] = decode_tensor(z[key], z[name + '/alpha'], z[name + '/beta'], z[name + '/meta'])
      done.update({key, name + '/alpha', name + '/beta', name + '/meta'})
  for key in z.files:
    if key not in done and not key.endswith(ACT_RANGE_SUFFIX):      # ranges are no variables: load_act_ranges
      out[key] = z[key]
  return out


def load_act_ranges(path: str) -> Dict[str, Tuple[float, float]]:
  """{activation op name: (min, max)} of the `<op name>/act_range` entries of an artefact; empty for a file without ranges.  An
  entry that is not two numbers is a ValueError that names it."""
  out = {}
  with np.load(path) as z:
    for key in z.files:
      if key.endswith(ACT_RANGE_SUFFIX):
        v = np.asarray(z[key])
        if v.size != 2 or v.dtype.kind not in 'fiu':
          raise ValueError('%s: %s holds %s, expected [min, max]' % (path, key, tuple(v.shape)))
        v = v.astype(np.float32).reshape(-1)
        out[key[:-len(ACT_RANGE_SUFFIX)]] = (float(v[0]), float(v[1]))
  return out


def decode_slots(slots: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
  """(min, max), float32 each, of int32 min / max slots [n][2] as the device keeps them: the order-preserving encoding of the
  minimum and the complement of that of the maximum (pf_common.h enc_f32 / dec_f32, slot_alpha_beta)."""
  e = np.ascontiguousarray(slots).view(np.uint32).reshape(-1, 2)
  dec = lambda v: np.where(v & np.uint32(0x80000000), v & np.uint32(0x7FFFFFFF), ~v).astype(np.uint32).view(np.float32)
  return dec(e[:, 0].copy()), dec(~e[:, 1])


def calibrate_act_ranges(model_helper, path: str, nb_batches: int, activation_bits: int = 8, device='cuda', dtype=None) -> Dict:
  """Run `nb_batches` evaluation batches of the model helper's dataset through the artefact at `path` on the float route
  (load_int8(int8='off'): what the reference's eval graph evaluates, every quantiser recalibrating per batch), keep the minimum of
  the minima and the maximum of the maxima every activation quantiser saw, and rewrite the file with one float32
  `<activation op name>/act_range` = [min, max] per Relu / Relu6 op.  Returns {op name: (min, max)}."""
  import torch
  from pocketflow_amd.inference import load_int8
  if int(nb_batches) < 1:
    raise ValueError('calibrate_act_ranges: nb_batches must be positive (got %s)' % nb_batches)
  graph, forward = load_int8(model_helper, path, device, dtype if dtype is not None else torch.float32, activation_bits, int8='off')
  it = model_helper.build_dataset_eval()
  lo = hi = None
  for _ in range(int(nb_batches)):
    images, _ = it.get_next()
    forward(images)
    mn, mx = decode_slots(graph.act_slots.cpu().numpy())
    lo = mn if lo is None else np.minimum(lo, mn)
    hi = mx if hi is None else np.maximum(hi, mx)
  ranges = {}
  for op in graph.activation_ops:
    if op.type in ('Relu', 'Relu6'):
      ranges[op.name] = (float(lo[op.index]), float(hi[op.index]))
  write_act_ranges(path, ranges)
  return ranges


def write_act_ranges(path: str, ranges: Dict[str, Tuple[float, float]]) -> None:
  """Rewrite the artefact at `path` with exactly these ranges (earlier `*/act_range` entries are dropped; every other entry as is)."""
  with np.load(path) as z:
    out = {k: z[k] for k in z.files if not k.endswith(ACT_RANGE_SUFFIX)}
  for name, (mn, mx) in ranges.items():
    out[name + ACT_RANGE_SUFFIX] = np.array([mn, mx], np.float32)
  np.savez(path, **out)


def load_codes(path: str):
  """(variables, raw): `variables` as load_exported returns them; `raw` = {kernel name: dict(codes, alpha, beta, meta)} exactly as
  stored, for consumers that multiply the integers themselves (pocketflow_amd.int8.pack_layer)."""
  z = np.load(path)
  raw = {}
  for key in z.files:
    if key.endswith('/codes'):
      name = key[:-len('/codes')]
      raw[name] = dict(codes=z[key], alpha=z[name + '/alpha'], beta=z[name + '/beta'], meta=z[name + '/meta'])
  return load_exported(path), raw


def main(argv=None):
  import sys
  from pocketflow_amd.flags import FLAGS, flags
  flags.DEFINE_string('export_file', 'model_int8.npz', 'file name of the exported model (beside uql_save_quant_model_path)')
  flags.DEFINE_string('model_name', 'resnet', 'lenet | resnet | mobilenet')
  flags.DEFINE_string('dataset_name', 'cifar_10', 'cifar_10 | ilsvrc_12')
  flags.DEFINE_integer('calib_batches', 0, '# of evaluation batches to calibrate fixed activation ranges on (0: none, the file as before)')
  import importlib
  import pocketflow_amd.learners.uniform_quantization.learner as UQ
  FLAGS.parse(argv if argv is not None else sys.argv[1:])
  mod = importlib.import_module('pocketflow_amd.nets.%s_at_%s' % (FLAGS.model_name, FLAGS.dataset_name.replace('_', '')))
  learner = UQ.UniformQuantLearner(None, mod.ModelHelper())
  from pocketflow_amd.utils import checkpoint
  learner.restore_vars(checkpoint.latest_checkpoint(os.path.dirname(FLAGS.uql_save_quant_model_path)))
  path = os.path.join(os.path.dirname(FLAGS.uql_save_quant_model_path), FLAGS.export_file)
  summ = {k: v for k, v in export_from_learner(learner, path).items() if k != 'layers'}
  if FLAGS.calib_batches > 0:
    from pocketflow_amd.learners import abstract_learner as AL
    mh = learner.model_helper if hasattr(learner, 'model_helper') else mod.ModelHelper()
    del learner
    summ['act_ranges'] = len(calibrate_act_ranges(mh, path, FLAGS.calib_batches, FLAGS.uql_activation_bits, AL.require_gpu(),
                                                  AL.compute_dtype()))
  print(json.dumps(summ))


if __name__ == '__main__':
  main()
