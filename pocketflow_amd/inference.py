"""Inference on the device from a saved model: a plain checkpoint directory, or the physically shrunk artefact of
tools/conversion/export_chn_pruned_model.py (`model_shrunk.npz`: Conv2D kernels cut to [kh, kw, nnz, cout] plus an int32
`<conv>/kernel/gather` vector per shrunk convolution; reference tools/conversion/export_chn_pruned_tflite_model.py:184-276).

    graph, forward = load_shrunk(model_helper, './models_cpg_eval/model_shrunk.npz', 'cuda', torch.bfloat16)
    logits = forward(images_nhwc)                 # float32 NHWC batch in, logits out; torch.no_grad() inside

A shrunk convolution runs on hip.conv_gather_fwd (pf_conv_gather.hip): its reduction covers the kept input channels only.  Layers for
which `graph.gather_pays` says the gather kernel loses to the dense inference kernel are re-inflated at load time (the kept slices are
scattered back into a zero kernel of full shape) and run exactly as in the fake-pruned checkpoint; `graph.reinflated` lists them.

`load_int8` does the same for the integer artefact of tools/conversion/export_quant_int8_model.py (`model_int8.npz`): the learner's
activation quantisers on, and the eligible convolutions on hip.conv_i8_fwd (depthwise 3x3 layers: hip.dw_i8_fwd), which multiply the
integer codes themselves.
"""
from __future__ import annotations

import os
from typing import Dict, Tuple

import numpy as np
import torch

from pocketflow_amd import graph as G
from pocketflow_amd.flags import FLAGS
from pocketflow_amd.tools.conversion.export_chn_pruned_model import load_exported
from pocketflow_amd.utils import checkpoint

GATHER_SUFFIX = '/gather'


def read_model_file(path: str) -> Dict[str, np.ndarray]:
  """Variables (reference layout) of a `model_shrunk.npz` or of the latest checkpoint in a directory."""
  if os.path.isdir(path):
    prefix = checkpoint.latest_checkpoint(path)
    if prefix is None:
      raise FileNotFoundError('no checkpoint under ' + path)
    return checkpoint.load(prefix)
  if not os.path.exists(path):
    raise FileNotFoundError(path)
  return load_exported(path)


def split_gathers(values: Dict[str, np.ndarray]) -> Tuple[Dict[str, np.ndarray], Dict[str, np.ndarray]]:
  """(variables, {kernel name: gather vector}) of an exported model."""
  gathers = {k[:-len(GATHER_SUFFIX)]: v for k, v in values.items() if k.endswith(GATHER_SUFFIX)}
  return {k: v for k, v in values.items() if not k.endswith(GATHER_SUFFIX)}, gathers


def _scope_of(variables: Dict[str, np.ndarray]) -> str:
  """The model scope the file was written under ('model'; 'pruned_model' for the channel-pruning learners' copies)."""
  scopes = {k.split('/')[0] for k in variables if '/' in k}
  return scopes.pop() if len(scopes) == 1 else 'model'


def load_shrunk(model_helper, path: str, device='cuda', compute_dtype=torch.float32, reinflate: str = 'auto'):
  """Build the `forward_eval` graph of `model_helper`, apply the gathers of the model at `path`, finalise and load.
  Returns (graph, forward); forward(images) takes an NHWC float32 batch (NumPy or torch) and returns the logits.
  `graph.kernel_params` / `graph.kernel_params_kept`: convolution-kernel parameters of the full-shape model / of the graph as loaded;
  `graph.nb_gathered`: layers that run on the gather kernel.  `reinflate`: 'auto' re-inflates the layers `graph.gather_pays` rejects,
  'none' keeps every shrunk layer shrunk, 'all' re-inflates every layer -- the full-shape (fake-)pruned model with its zero
  channels, the baseline a shrunk file is timed against."""
  from pocketflow_amd.learners.abstract_learner import input_spec
  if reinflate not in ('auto', 'none', 'all'):
    raise ValueError("reinflate must be 'auto', 'none' or 'all'")
  variables, gathers = split_gathers(read_model_file(path))
  graph = G.Graph(_scope_of(variables), device, compute_dtype)
  graph.fuse_conv1x1 = bool(FLAGS.fuse_conv1x1)
  with graph.as_default():
    model_helper.forward_eval(input_spec(model_helper))
  graph.kernel_params = sum(v.numel for v in graph.store.vars if v.kind == 'conv')
  for name in sorted(gathers):
    var = graph.store.by_name.get(name)
    if reinflate == 'none' or var is None or var.kind != 'conv' or name not in variables:
      continue                                   # (anything malformed is reported by apply_gathers, with the variable's name)
    kh, kw, cin, cout = var.ref_shape
    g = np.asarray(gathers[name])
    if np.shape(variables[name]) == (kh, kw, g.size, cout) and (
        reinflate == 'all' or not G.gather_pays(kh, cin, int(g.size), cout, compute_dtype)):
      g = G.check_gather(g, cin, int(g.size), what=name)
      full = np.zeros((kh, kw, cin, cout), dtype=np.float32)
      full[:, :, g, :] = variables[name]
      variables[name] = full
      del gathers[name]
      graph.reinflated.append(name)
  graph.apply_gathers(gathers, variables)
  graph.finalize(requires_grad=False)
  graph.store.load_numpy(variables, strict=True)
  graph.training = False
  graph.frozen = True                            # the weights are fixed from here on: the folded BN scale / shift pairs are cached
  graph.kernel_params_kept = sum(v.numel for v in graph.store.vars if v.kind == 'conv')
  graph.nb_gathered = len(gathers)

  def forward(images) -> torch.Tensor:
    with torch.no_grad(), graph.as_default():
      return model_helper.forward_eval(G.to_device_images(images, graph))
  return graph, forward


def load_int8(model_helper, path: str, device='cuda', compute_dtype=torch.float32, activation_bits: int = 8, int8: str = 'auto',
              depthwise: str = 'off', act_ranges: str = 'batch'):
  """The integer artefact of tools/conversion/export_quant_int8_model.py (`model_int8.npz`) as an inference graph with the learner's
  activation quantisers on (`activation_bits` for every Relu / Relu6, as UniformQuantLearner feeds them).  Returns (graph, forward)
  like load_shrunk.  `int8`:
    'off'   every kernel decoded to float and run on the float kernels: what restoring the artefact into the learner evaluates;
    'on'    every eligible Conv2D on hip.conv_i8_fwd: a kernel with at most 8 bits in tensor or channel buckets that
            pf_conv_i8_supported takes.  It multiplies codes only where its input arrives as codes (a quantising BatchNormAct with
            at most 8 activation bits whose consumers are all Conv2D); anywhere else it runs on its decoded kernel;
    'auto'  of those, the layers `graph.int8_pays` accepts.
  `depthwise` (ignored when int8 = 'off') does the same for the depthwise 3x3 layers (MobileNet-v1) and hip.dw_i8_fwd:
    'off'   none, the default: every depthwise layer runs on its decoded kernel (a producer's codes are materialised for it);
    'on'    every eligible one: at most 8 bits, not in split buckets, `int8.depthwise_supported`;
    'auto'  of those, the layers `graph.int8_dw_pays` accepts.
  `graph.nb_int8`: layers packed for the int8 route, Conv2D and depthwise together; `graph.int8_ran`: names of the kernels that
  took it in the forward passes so far.  Everything else -- the stem, Dense, split buckets, wider kernels -- is untouched.  A
  malformed entry is a ValueError that names the variable.
  `act_ranges`:
    'batch'   the default: every activation quantiser recalibrates on every batch, as the learner's eval graph does;
    'static'  the ranges the artefact carries (`<activation op name>/act_range`, written by the export tool's --calib_batches): each is
              written into its slot once, decoded once (`graph.act_static`), and `forward` never resets or writes the slots.  Every
              quantiser then runs on a clamping kernel (pf_act_static.hip), no statistics pass runs, and a packed layer whose one
              consumer is a quantising BatchNormAct applies it in its epilogue and hands on codes or the fake-quantised tensor
              (`graph.requant_ran`).  'auto' then means `graph.int8_pays_static` / `graph.int8_dw_pays_static`.  A file without
              ranges, a missing or surplus entry, a non-finite range or min > max is a ValueError that names the file or the op."""
  from pocketflow_amd import int8 as I8
  from pocketflow_amd.learners.abstract_learner import input_spec
  from pocketflow_amd.tools.conversion.export_quant_int8_model import MODE_SPLIT, load_codes
  if int8 not in ('auto', 'on', 'off'):
    raise ValueError("int8 must be 'auto', 'on' or 'off'")
  if depthwise not in ('auto', 'on', 'off'):
    raise ValueError("depthwise must be 'auto', 'on' or 'off'")
  if not 1 <= int(activation_bits) <= 32:
    raise ValueError('activation_bits must lie in 1..32 (got %s)' % activation_bits)
  if act_ranges not in ('batch', 'static'):
    raise ValueError("act_ranges must be 'batch' or 'static'")
  static = act_ranges == 'static'
  if not os.path.isfile(path):
    raise FileNotFoundError(path)
  variables, raw = load_codes(path)
  ranges = None
  if static:
    from pocketflow_amd.tools.conversion.export_quant_int8_model import load_act_ranges
    ranges = load_act_ranges(path)
    if not ranges:
      raise ValueError("%s: act_ranges='static' needs an artefact with activation ranges (export with --calib_batches)" % path)
  pays = G.int8_pays_static if static else G.int8_pays
  dw_pays = G.int8_dw_pays_static if static else G.int8_dw_pays
  graph = G.Graph(_scope_of(variables), device, compute_dtype)
  graph.fuse_conv1x1 = bool(FLAGS.fuse_conv1x1)
  with graph.as_default():
    model_helper.forward_eval(input_spec(model_helper))
  for join in graph.join_layers:                 # the BN + shortcut + ReLU tails of ResNet-v1 blocks: no codes, no clamping pass
    raise ValueError(join.refusal())
  layers = {conv.kernel.name: conv for conv in graph.conv_layers}
  dw_layers = {dw.kernel.name: dw for dw in graph.depthwise_layers}
  packed, packed_dw = {}, {}
  for name in sorted(raw):
    var = graph.store.by_name.get(name)
    if var is None:
      raise ValueError('%s: codes for a variable this graph does not have' % name)
    meta = np.asarray(raw[name]['meta'])
    if meta.ndim != 1 or meta.size < 4 or tuple(int(v) for v in meta[3:]) != tuple(var.ref_shape):
      raise ValueError('%s: codes of shape %s, the graph has %s' % (name, tuple(int(v) for v in meta[3:]), tuple(var.ref_shape)))
    dw = dw_layers.get(name)
    if dw is not None:
      if (int8 == 'off' or depthwise == 'off' or int(meta[0]) > 8 or int(meta[1]) == MODE_SPLIT
          or not I8.depthwise_supported(dw.channels, dw.k, dw.stride)):
        continue
      if depthwise == 'auto' and not dw_pays(dw.channels, dw.stride, compute_dtype):
        continue
      try:
        packed_dw[name] = I8.pack_depthwise(raw[name]['codes'], raw[name]['alpha'], raw[name]['beta'], meta)
      except ValueError as e:
        raise ValueError('%s: %s' % (name, e))
      continue
    conv = layers.get(name)
    if int8 == 'off' or conv is None or conv.bias is not None or int(meta[0]) > 8 or int(meta[1]) == MODE_SPLIT:
      continue
    kh, kw, cin, cout = var.ref_shape
    if not I8.supported(cin, cout, kh, kw, conv.stride):
      continue
    if int8 == 'auto' and not pays(kh, cin, cout, conv.stride, compute_dtype):
      continue
    try:
      packed[name] = I8.pack_layer(raw[name]['codes'], raw[name]['alpha'], raw[name]['beta'], meta)
    except ValueError as e:
      raise ValueError('%s: %s' % (name, e))
  for op in graph.activation_ops:
    if op.type in ('Relu', 'Relu6'):
      op.bits = int(activation_bits)
  if static:
    _check_act_ranges(path, graph, ranges)
  graph.finalize(requires_grad=False)
  graph.store.load_numpy(variables, strict=True)
  graph.training = False
  graph.frozen = True                            # the weights are fixed from here on
  graph.int8 = bool(packed) or bool(packed_dw)
  graph.nb_int8 = len(packed) + len(packed_dw)

  def upload(table):
    return torch.from_numpy(np.ascontiguousarray(table)).to(graph.device)
  for name, p in packed.items():
    layers[name].int8 = {k: upload(p[k]) for k in ('w', 'scale_beta', 'tsum', 'tapsum')}
  for name, p in packed_dw.items():
    dw_layers[name].int8 = {'wcol': upload(p['wcol'].view(np.int32)), 'scale_beta': upload(p['scale_beta'])}

  if static:
    # each range into its slot, through the kernels a batch with that minimum / maximum would go through: the slot then decodes
    # exactly as it would after such a batch
    from pocketflow_amd import hip
    hip.minmax_slots_init(graph.act_slots)
    for op in graph.activation_ops:
      if op.name in ranges:
        hip.minmax_tensor(torch.tensor(ranges[op.name], dtype=torch.float32, device=graph.device), graph.act_slots[op.index], None)
    graph.act_static = graph.act_alpha_beta()

  def forward(images) -> torch.Tensor:
    with torch.no_grad(), graph.as_default():
      if not static:
        graph.begin_step()                       # the activation quantisers calibrate on every batch; static: the slots stay as loaded
      return model_helper.forward_eval(G.to_device_images(images, graph))
  return graph, forward


def _check_act_ranges(path: str, graph, ranges) -> None:
  """The artefact's ranges against the graph's Relu / Relu6 ops: one finite pair with min <= max for each, and nothing else."""
  ops = {op.name for op in graph.activation_ops if op.type in ('Relu', 'Relu6')}
  for name in sorted(ops - set(ranges)):
    raise ValueError('%s: no activation range for %s' % (path, name))
  for name in sorted(set(ranges) - ops):
    raise ValueError('%s: an activation range for %s, which is no activation op of this graph' % (path, name))
  for name in sorted(ops):
    mn, mx = ranges[name]
    if not (np.isfinite(mn) and np.isfinite(mx)):
      raise ValueError('%s: the activation range of %s is not finite (%r, %r)' % (path, name, mn, mx))
    if mn > mx:
      raise ValueError('%s: the activation range of %s has min %r > max %r' % (path, name, mn, mx))
