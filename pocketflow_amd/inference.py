"""Inference on the device from a saved model: a plain checkpoint directory, or the physically shrunk artefact of
tools/conversion/export_chn_pruned_model.py (`model_shrunk.npz`: Conv2D kernels cut to [kh, kw, nnz, cout] plus an int32
`<conv>/kernel/gather` vector per shrunk convolution; reference tools/conversion/export_chn_pruned_tflite_model.py:184-276).

    graph, forward = load_shrunk(model_helper, './models_cpg_eval/model_shrunk.npz', 'cuda', torch.bfloat16)
    logits = forward(images_nhwc)                 # float32 NHWC batch in, logits out; torch.no_grad() inside

A shrunk convolution runs on hip.conv_gather_fwd (pf_conv_gather.hip): its reduction covers the kept input channels only.  Layers for
which `graph.gather_pays` says the gather kernel loses to the dense inference kernel are re-inflated at load time (the kept slices are
scattered back into a zero kernel of full shape) and run exactly as in the fake-pruned checkpoint; `graph.reinflated` lists them.
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
