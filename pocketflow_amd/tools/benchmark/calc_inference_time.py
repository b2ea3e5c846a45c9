"""Measure the inference time of a model on the device (reference tools/benchmark/calc_inference_time.py, which times *.pb /
*.tflite files): here the model is a `model_shrunk.npz` written by tools/conversion/export_chn_pruned_model.py or a checkpoint
directory, loaded with pocketflow_amd.inference.load_shrunk.

    python -m pocketflow_amd.tools.conversion.export_chn_pruned_model --model_dir ./models --enbl_fake_prune --fake_prune_ratio 0.5
    python -m pocketflow_amd.tools.benchmark.calc_inference_time --net resnet_at_ilsvrc12 --resnet_size 50 --batch_size 256 \\
        --compute_dtype bfloat16 --model_file ./models/model_shrunk.npz                      # shrunk layers on the gather kernel
    python -m pocketflow_amd.tools.benchmark.calc_inference_time ... --model_file ./models/model_shrunk.npz --reinflate all
                                                           # the same weights in full shape (zero channels): the baseline

Flags: `--model_file`, `--nb_repts_warmup` (100), `--nb_repts` (100) as in the reference; `--net` names the ModelHelper module under
pocketflow_amd.nets, whose own flags (`--resnet_size`, `--mobilenet_depth_mult`, `--nb_classes`, `--image_size` ...) and
`--compute_dtype` apply.  `--batch_size` is the datasets' flag of that name (the reference tool's own `batch_size` defaults to 1;
here the default is the dataset's training batch, 128 for CIFAR-10 and 64 for ILSVRC-12), because one registry holds both.
`--reinflate auto|none|all`: see load_shrunk.  A `model_int8.npz` written by tools/conversion/export_quant_int8_model.py goes through the same
`--model_file` flag and is loaded with pocketflow_amd.inference.load_int8: `--int8 auto|on|off` chooses which eligible convolutions
multiply integer codes on the i8 matrix cores ('off': every kernel decoded, the float kernels; the baseline), and the learner's own
`--uql_activation_bits` (default 32: no codes, nothing runs on int8) sets the activation quantisers; the result line then carries
`nb_int8_layers`.  `--int8_depthwise off|on|auto` (default off) does the same for the depthwise 3x3 layers of a MobileNet
(pf_dw_i8_fwd; 'auto' = the layers graph.int8_dw_pays accepts); packed depthwise layers count in `nb_int8_layers`.
`--act_ranges batch|static` (default batch): 'static' quantises every activation against the fixed range the file carries (written by
export_quant_int8_model --calib_batches N) instead of recalibrating per batch; `nb_requant_layers` then counts the packed layers that
applied the BatchNorm + activation + quantiser behind them in their own epilogue.

    python -m pocketflow_amd.tools.benchmark.calc_inference_time --net resnet_at_ilsvrc12 --resnet_size 50 --batch_size 256 \\
        --compute_dtype bfloat16 --model_file ./models_uqtf_eval/model_int8.npz --int8 on --uql_activation_bits 8

The input is a batch of zeros, like the reference's; it is put on the device and
converted once, outside the timed window.  The window is a host clock around `nb_repts` forward passes that ends in a device
synchronise.  Prints ms per batch and per image; `--json` prints one JSON line with those, the number of gathered layers and the
kept share of convolution-kernel parameters.
"""
from __future__ import annotations

import importlib
import json
import logging
import os
import sys
from timeit import default_timer as timer

import numpy as np
import torch

from pocketflow_amd.flags import FLAGS, flags

flags.DEFINE_string('model_file', None, 'model file path: a model_shrunk.npz or a checkpoint directory')
flags.DEFINE_integer('nb_repts_warmup', 100, '# of repeated runs for warm-up')
flags.DEFINE_integer('nb_repts', 100, '# of repeated runs for elapsed time measurement')
flags.DEFINE_string('net', 'resnet_at_ilsvrc12', 'ModelHelper module under pocketflow_amd.nets')
flags.DEFINE_string('reinflate', 'auto', "'auto': re-inflate the layers graph.gather_pays rejects | 'none' | 'all' (full-shape baseline)")
flags.DEFINE_string('int8', 'auto', "a model_int8.npz: 'auto' = the layers graph.int8_pays accepts on the int8 kernel | 'on' = every eligible layer | 'off' = none")
flags.DEFINE_string('int8_depthwise', 'off', "a model_int8.npz: depthwise 3x3 layers on the int8 kernel: 'off' = none | 'on' = every eligible layer | 'auto' = the layers graph.int8_dw_pays accepts")
flags.DEFINE_string('act_ranges', 'batch', "a model_int8.npz: 'batch' = every activation quantiser recalibrates per batch | 'static' = the ranges the file carries (export with --calib_batches)")
flags.DEFINE_boolean('json', False, 'print one JSON result line')

log = logging.getLogger('pocketflow_amd')


def _net_of(argv) -> str:
  """The value of --net, read before parsing: the net's module defines flags the parser must know."""
  for i, a in enumerate(argv):
    if a.startswith('--net='):
      return a.split('=', 1)[1]
    if a == '--net' and i + 1 < len(argv):
      return argv[i + 1]
  return 'resnet_at_ilsvrc12'


def measure(forward_eval, graph, x, nb_warmup: int, nb_repts: int) -> float:
  """Seconds per forward pass: host clock around nb_repts passes, closed by a device synchronise."""
  sync = (lambda: torch.cuda.synchronize()) if x.is_cuda else (lambda: None)
  with torch.no_grad(), graph.as_default():
    for _ in range(nb_warmup):
      forward_eval(x)
    sync()
    beg = timer()
    for _ in range(nb_repts):
      forward_eval(x)
    sync()
    return (timer() - beg) / max(nb_repts, 1)


def is_int8_artefact(path: str) -> bool:
  """A file of export_quant_int8_model.py: an .npz that holds `<kernel>/codes` entries."""
  if not (isinstance(path, str) and path.endswith('.npz') and os.path.isfile(path)):
    return False
  with np.load(path) as z:
    return any(k.endswith('/codes') for k in z.files)


def main(argv=None) -> int:
  argv = list(sys.argv[1:] if argv is None else argv)
  from pocketflow_amd.learners import abstract_learner as AL
  from pocketflow_amd.graph import to_device_images
  from pocketflow_amd.inference import load_int8, load_shrunk
  import pocketflow_amd.learners.uniform_quantization.learner  # noqa: F401  (defines --uql_activation_bits)
  mod = importlib.import_module('pocketflow_amd.nets.' + _net_of(argv))
  FLAGS.parse(argv)
  logging.basicConfig(level=logging.INFO)
  if FLAGS.model_file is None:
    raise ValueError('<FLAGS.model_file> must not be None')
  device = AL.require_gpu()
  mh = mod.ModelHelper()
  int8 = is_int8_artefact(FLAGS.model_file)
  if int8:
    graph, _ = load_int8(mh, FLAGS.model_file, device, AL.compute_dtype(), FLAGS.uql_activation_bits, int8=FLAGS.int8,
                         depthwise=FLAGS.int8_depthwise, act_ranges=FLAGS.act_ranges)
  else:
    graph, _ = load_shrunk(mh, FLAGS.model_file, device, AL.compute_dtype(), reinflate=FLAGS.reinflate)
  batch = int(mh.dataset_train.batch_size)
  x = to_device_images(np.zeros((batch,) + tuple(mh.dataset_train.image_shape), dtype=np.float32), graph)

  def forward_eval(images):
    if int8 and graph.act_static is None:
      graph.begin_step()                         # the activation quantisers calibrate on every batch
    return mh.forward_eval(images)
  sec = measure(forward_eval, graph, x, FLAGS.nb_repts_warmup, FLAGS.nb_repts)
  rslt = {'model_file': FLAGS.model_file, 'net': FLAGS.net, 'compute_dtype': FLAGS.compute_dtype, 'batch_size': batch,
          'nb_repts_warmup': FLAGS.nb_repts_warmup, 'nb_repts': FLAGS.nb_repts, 'reinflate': FLAGS.reinflate,
          'ms_per_batch': sec * 1e3, 'ms_per_image': sec * 1e3 / batch, 'nb_gathered_layers': graph.nb_gathered,
          'nb_reinflated_layers': len(graph.reinflated),
          'kernel_params_kept_share': graph.kernel_params_kept / max(graph.kernel_params, 1)}
  if int8:
    rslt.update({'int8': FLAGS.int8, 'int8_depthwise': FLAGS.int8_depthwise, 'nb_int8_layers': graph.nb_int8, 'nb_int8_layers_ran': len(graph.int8_ran),
                 'activation_bits': FLAGS.uql_activation_bits, 'act_ranges': FLAGS.act_ranges,
                 'nb_requant_layers': len(graph.requant_ran)})
  print('time consumption of %s: %.3f ms per batch of %d, %.4f ms per image (%d gathered layers, %d re-inflated)'
        % (FLAGS.model_file, rslt['ms_per_batch'], batch, rslt['ms_per_image'], graph.nb_gathered, len(graph.reinflated)))
  if int8:
    print('int8 = %s, int8_depthwise = %s: nb_int8_layers = %d (%d took the int8 kernel), %d activation bits'
          % (FLAGS.int8, FLAGS.int8_depthwise, graph.nb_int8, len(graph.int8_ran), FLAGS.uql_activation_bits))
  if FLAGS.json:
    print(json.dumps(rslt))
  return 0


if __name__ == '__main__':
  sys.exit(main())
