"""Variables, ops and the explicit layer executor that stand in for the reference's TF-1.x graph.

The reference builds a tf.Graph from a ModelHelper's forward function, then *rewrites* it with
tf.contrib.graph_editor to splice fake-quant ops in front of every Conv2D / MatMul /
DepthwiseConv2dNative weight and behind every Relu / Relu6 output
(learners/uniform_quantization/utils.py:51-134).  Here the same information is explicit:

  * `VarStore`  -- every variable of one model scope, named like the TF checkpoint
                   (`model/resnet_model/conv2d_3/kernel`), living in a few flat device buffers:
                   all matmul kernels in ONE fp32 master buffer (+ one compute-dtype copy that the
                   quantiser writes and the convolutions read, + one flat gradient buffer), all other
                   trainables in a second, BN moving statistics in a third.  One launch quantises
                   every kernel, one launch applies the optimiser, one collective reduces gradients.
  * `Graph`     -- ops in creation order (`matmul_ops`, `activation_ops`), which is what
                   `search_matmul_op` / `search_activation_op` enumerate; a learner "rewrites" the
                   graph by assigning bit widths to those ops.
  * layer classes -- Conv2D / DepthwiseConv2D / Dense / BatchNormAct / Activation / pooling, executed
                   eagerly on HIP streams (or recorded once and replayed, step_graph.py); every layer of the
                   benchmarked networks calls the hand-written kernels through the C ABI (pocketflow_amd.hip):
                   the MFMA kernels for the 1x1 / RxS convolutions, pf_convg.hip for every other shape and
                   for the float32 parity mode.  torch's library convolution is left only for geometries no
                   benchmarked network has (few-channel RxS convolutions with a bias, the stem's image gradient).

Storage layouts are chosen for the GPU (activations NHWC = torch channels_last, kernels KRSC =
[cout][kh][kw][cin]); `VarStore.export_numpy` / `load_numpy` speak the reference's layouts (HWIO
kernels, [in, out] dense) so that checkpoints and the oracle see TF-shaped tensors.
"""
from __future__ import annotations

import contextlib
import math
import os
import threading
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from pocketflow_amd import hip
from pocketflow_amd.hip import check_gather
from pocketflow_amd.hip import bn_vector_ok as _bn_vector_ok   # bound here: the tests' stand-ins for `hip` emulate launches only
from pocketflow_amd.plan import WeightDesc
from pocketflow_amd.profiling import region

ALIGN = 64  # elements; keeps every tensor 256-byte aligned inside the flat buffers
# reduce the BN-backward statistics inside the backward-data kernel of the single consuming 1x1 convolution
FUSE_BN_BWD_STATS = os.environ.get('PF_FUSE_BN_BWD_STATS', '1') != '0'
# the network head in fused launches: the last BN reduced to its spatial mean in pass 2 and never written (pf_bn_act_quant_pool, both
# backward passes rebuilt from the pooled gradient), the step's two losses + metrics in one launch (losses.py).  0: the separate chain.
HEAD_FUSE = os.environ.get('PF_HEAD_FUSE', '1') != '0'
HEAD_FUSE_ANY_DEVICE = False     # tests: run the head plumbing on CPU tensors (the HIP entry points are emulated there)
BN_JOIN_ANY_DEVICE = False       # tests: likewise for the BN + shortcut + ReLU join of the v1 blocks (BatchNormAddAct)
# how a BatchNorm layer runs (BatchNormAct._mode): batch statistics; moving statistics with gradients; moving statistics without
BN_TRAIN, BN_EVAL_GRAD, BN_EVAL = 0, 1, 2


def _align(n: int) -> int:
  return (n + ALIGN - 1) // ALIGN * ALIGN


# =================================================================================================
# variables
# =================================================================================================

@dataclass
class Variable:
  name: str                      # TF-style name without ':0'
  ref_shape: Tuple[int, ...]     # reference layout: HWIO conv, [in,out] dense, [kh,kw,C,1] depthwise
  kind: str                      # conv | dense | depthwise | bias | bn_gamma | bn_beta | bn_mean | bn_var | other
  trainable: bool = True
  l2: bool = True                # enters the loss_w_dcy * l2_loss sum of ModelHelper.calc_loss
  init: Optional[Callable[[np.random.RandomState], np.ndarray]] = field(default=None, repr=False)
  group: str = ''                # 'W' matmul kernels | 'O' other trainables | 'S' non-trainable state
  offset: int = 0
  numel: int = 0
  tensor: Optional[torch.Tensor] = field(default=None, repr=False)  # forward view (leaf; compute copy for 'W')
  store: Optional[object] = field(default=None, repr=False)   # owning VarStore
  master: Optional[torch.Tensor] = field(default=None, repr=False)  # fp32 master view
  # a physically shrunk Conv2D kernel (Graph.apply_gathers): ref_shape[2] is the number of KEPT input channels, `cin_full` the layer's
  # input channels, `gather_host` the kept channel indices (int32, strictly ascending), `gather` the same vector on the device
  cin_full: int = 0
  gather_host: Optional[np.ndarray] = field(default=None, repr=False)
  gather: Optional[torch.Tensor] = field(default=None, repr=False)

  @property
  def storage_shape(self) -> Tuple[int, ...]:
    s = self.ref_shape
    if self.kind == 'conv':
      return (s[3], s[0], s[1], s[2])          # KRSC
    if self.kind == 'dense':
      return (s[1], s[0])                      # [out, in]
    if self.kind == 'depthwise':
      return (s[2], s[0], s[1])                # CRS
    return tuple(s)

  def to_storage(self, ref: np.ndarray) -> np.ndarray:
    ref = np.asarray(ref, dtype=np.float32).reshape(self.ref_shape)
    if self.kind == 'conv':
      return np.ascontiguousarray(ref.transpose(3, 0, 1, 2))
    if self.kind == 'dense':
      return np.ascontiguousarray(ref.T)
    if self.kind == 'depthwise':
      return np.ascontiguousarray(ref[:, :, :, 0].transpose(2, 0, 1))
    return ref

  def to_ref(self, st: np.ndarray) -> np.ndarray:
    st = np.asarray(st, dtype=np.float32).reshape(self.storage_shape)
    if self.kind == 'conv':
      return np.ascontiguousarray(st.transpose(1, 2, 3, 0))
    if self.kind == 'dense':
      return np.ascontiguousarray(st.T)
    if self.kind == 'depthwise':
      return np.ascontiguousarray(st.transpose(1, 2, 0)[:, :, :, None])
    return st

  def weight_desc(self) -> WeightDesc:
    s = self.ref_shape
    if self.kind == 'conv':
      return WeightDesc(self.name, self.offset, s[0] * s[1], s[2], s[3], 0)
    if self.kind == 'dense':
      return WeightDesc(self.name, self.offset, 1, s[0], s[1], 0)
    if self.kind == 'depthwise':
      return WeightDesc(self.name, self.offset, s[0] * s[1], s[2], 1, 1)
    raise ValueError('not a matmul kernel: %s' % self.name)


class VarStore:
  """All variables of one model scope in three flat device buffers (see module docstring)."""

  def __init__(self, scope: str):
    self.scope = scope
    self.vars: List[Variable] = []
    self.by_name: Dict[str, Variable] = {}
    self.finalized = False
    self.device = None
    self.compute_dtype = torch.float32
    self.weight_decay = 0.0                    # set by ModelHelper.calc_loss (loss_w_dcy)
    self.grad_hook = None                      # optim.GradReducer: called once per variable whose gradient is final

  # -- declaration ------------------------------------------------------------------------------
  def add(self, name: str, ref_shape, kind: str, trainable: bool = True, l2: bool = True,
          init=None) -> Variable:
    full = self.scope + '/' + name if self.scope else name
    if full in self.by_name:
      return self.by_name[full]                  # tf.AUTO_REUSE
    if self.finalized:
      raise RuntimeError('variable %s created after the store was finalized' % full)
    v = Variable(full, tuple(int(d) for d in ref_shape), kind, trainable, l2 and trainable, init)
    v.numel = int(np.prod(v.ref_shape))
    v.group = 'W' if kind in ('conv', 'dense', 'depthwise') else ('O' if trainable else 'S')
    v.store = self
    self.vars.append(v)
    self.by_name[full] = v
    return v

  @property
  def trainable_vars(self) -> List[Variable]:
    return [v for v in self.vars if v.trainable]

  @property
  def matmul_vars(self) -> List[Variable]:
    return [v for v in self.vars if v.group == 'W']

  def notify_grad(self, var: 'Variable') -> None:
    """The gradient of `var` is complete in the flat gradient buffer (enqueued on the current stream): lets the
    data-parallel reducer launch that bucket's all-reduce while the rest of the backward pass still runs."""
    if self.grad_hook is not None:
      self.grad_hook(var)

  # -- allocation -------------------------------------------------------------------------------
  def finalize(self, device, compute_dtype=torch.float32, separate_compute: bool = False,
               seed: int = 42, requires_grad: bool = True) -> None:
    """Lay variables out and allocate.  `separate_compute`: keep a compute-dtype copy of the matmul
    kernels distinct from the fp32 master (needed when they are fake-quantised or cast to bf16)."""
    if self.finalized:
      return
    self.device = torch.device(device)
    self.compute_dtype = compute_dtype
    separate_compute = separate_compute or compute_dtype != torch.float32
    self.separate_compute = separate_compute
    # matmul kernels: [l2-regularised | not regularised] so that one n_decay splits the buffer
    off = 0
    for flag in (True, False):
      for v in self.vars:
        if v.group == 'W' and v.l2 == flag:
          v.offset = off
          off += _align(v.numel)
      if flag:
        self.w_decay = off
    self.w_size = off
    # other trainables: [l2-regularised | not regularised] so that one n_decay splits them
    off = 0
    for flag in (True, False):
      for v in self.vars:
        if v.group == 'O' and v.l2 == flag:
          v.offset = off
          off += _align(v.numel)
      if flag:
        self.o_decay = off
    self.o_size = off
    off = 0
    for v in self.vars:
      if v.group == 'S':
        v.offset = off
        off += _align(v.numel)
    self.s_size = off
    dev = self.device
    self.w_master = torch.zeros(max(self.w_size, ALIGN), dtype=torch.float32, device=dev)
    self.w_compute = (torch.zeros(max(self.w_size, ALIGN), dtype=compute_dtype, device=dev)
                      if separate_compute else self.w_master)
    self.o_master = torch.zeros(max(self.o_size, ALIGN), dtype=torch.float32, device=dev)
    self.state = torch.zeros(max(self.s_size, ALIGN), dtype=torch.float32, device=dev)
    self.w_grad = torch.zeros_like(self.w_compute) if requires_grad else None
    self.w_t = None                            # backward-data layout of the convolution kernels (lazily built)
    self.w_t_fresh = False
    self._t_tiles, self._n_t_tiles = None, 0
    self.o_grad = torch.zeros_like(self.o_master) if requires_grad else None
    for v in self.vars:
      n = v.numel
      if v.group == 'W':
        v.master = self.w_master[v.offset:v.offset + n].view(v.storage_shape)
        t = self.w_compute[v.offset:v.offset + n].view(v.storage_shape)
        if v.kind == 'conv':
          t = t.permute(0, 3, 1, 2)            # logical OIHW, physical KRSC (= channels_last)
        elif v.kind == 'depthwise':
          t = t.unsqueeze(1)                   # [C, 1, kh, kw]
        if requires_grad and v.trainable:
          t = t.detach().requires_grad_(True)
          g = self.w_grad[v.offset:v.offset + n].view(v.storage_shape)
          if v.kind == 'conv':
            g = g.permute(0, 3, 1, 2)
          elif v.kind == 'depthwise':
            g = g.unsqueeze(1)
          t.grad = g
          t.register_post_accumulate_grad_hook(lambda _t, _v=v: self.notify_grad(_v))
        v.tensor = t
      elif v.group == 'O':
        v.master = self.o_master[v.offset:v.offset + n].view(v.storage_shape)
        t = v.master
        if requires_grad:
          t = t.detach().requires_grad_(True)
          t.grad = self.o_grad[v.offset:v.offset + n].view(v.storage_shape)
        v.tensor = t
      else:
        v.master = self.state[v.offset:v.offset + n].view(v.storage_shape)
        v.tensor = v.master
    self.finalized = True
    self.initialize(seed)

  def initialize(self, seed: int = 42) -> None:
    rng = np.random.RandomState(seed)
    vals = {}
    for v in self.vars:
      if v.init is not None:
        vals[v.name] = v.init(rng)
    self.load_numpy(vals, strict=False)

  # -- (de)serialisation in the REFERENCE layout --------------------------------------------------
  def load_numpy(self, values: Dict[str, np.ndarray], strict: bool = True, rename_scope: str = None) -> None:
    for v in self.vars:
      key = v.name
      if rename_scope is not None:             # distillation_helper.py:122-145: first path component
        key = rename_scope + '/' + '/'.join(v.name.split('/')[1:])
      if key not in values:
        if strict:
          raise KeyError('variable %s missing from checkpoint' % key)
        continue
      st = torch.from_numpy(v.to_storage(values[key])).to(self.device)
      v.master.copy_(st)
    self.sync_compute()

  def export_numpy(self) -> Dict[str, np.ndarray]:
    out = {}
    for v in self.vars:
      out[v.name] = v.to_ref(v.master.detach().float().cpu().numpy())
    return out

  def sync_compute(self) -> None:
    """compute copy <- master (plain cast); quantising learners overwrite it every step."""
    if self.separate_compute:
      self.w_compute.copy_(self.w_master)
    self.w_t_fresh = False

  # -- backward-data layout of the convolution kernels: W'[c][R-1-r][S-1-s][n] = W[n][r][s][c], all kernels, one launch ----
  def _build_transpose_tiles(self) -> None:
    rows = []
    for v in self.vars:
      if v.group != 'W' or v.kind != 'conv':      # every convolution kernel, trainable or not: a frozen kernel whose
        continue                                   # INPUT needs a gradient is read in this layout too
      kh, kw, cin, cout = v.ref_shape
      RS = kh * kw
      for rs in range(RS):
        for o0 in range(0, cout, 64):
          for i0 in range(0, cin, 64):
            rows.append((v.offset + rs * cin, v.offset + (RS - 1 - rs) * cout, cout, cin, RS * cin, RS * cout, o0, i0, 0, 0))
    from pocketflow_amd.hip import TILE_DTYPE      # (the `hip` module object may be a test double)
    tiles = np.array(rows, dtype=TILE_DTYPE) if rows else np.zeros(0, dtype=TILE_DTYPE)
    self._n_t_tiles = len(rows)
    self._t_tiles = torch.from_numpy(tiles.view(np.uint8).copy()).to(self.device) if rows else None
    self.w_t = torch.zeros_like(self.w_compute)

  def transposed(self, v: 'Variable') -> torch.Tensor:
    """Kernel `v` in backward-data layout, [C][R][S][N] (1x1: [K][N]), a view of the flat buffer `w_t`; refreshed for
    ALL kernels by one pf_seg_transpose launch the first time it is asked for after the compute copy changed."""
    if self.w_t is None:
      self._build_transpose_tiles()
    if not self.w_t_fresh:
      if self._n_t_tiles:
        hip.seg_transpose(self.w_compute, self.w_t, self._t_tiles, self._n_t_tiles)
      self.w_t_fresh = True
    kh, kw, cin, cout = v.ref_shape
    return self.w_t[v.offset:v.offset + v.numel].view(cin, kh, kw, cout)

  def zero_grad(self) -> None:
    if self.w_grad is not None:
      self.w_grad.zero_()
      self.o_grad.zero_()

  def weight_descs(self, variables: Sequence[Variable]) -> List[WeightDesc]:
    return [v.weight_desc() for v in variables]

  def l2_loss_sum(self) -> torch.Tensor:
    """sum_v l2_loss(v) over the regularised trainables (only evaluated for logging)."""
    tot = torch.zeros((), dtype=torch.float32, device=self.device)
    for v in self.vars:
      if v.trainable and v.l2:
        tot = tot + 0.5 * (v.master.float() ** 2).sum()
    return tot


# =================================================================================================
# ops and graph
# =================================================================================================

@dataclass
class MatmulOp:
  type: str                  # Conv2D | MatMul | DepthwiseConv2dNative   (uq utils.py:49)
  name: str
  var: Variable
  flops_per_out: int = 0


@dataclass
class ActivationOp:
  type: str                  # Relu | Relu6
  name: str
  index: int = 0
  bits: Optional[int] = None           # None: no fake-quant inserted behind this activation


_tls = threading.local()


def get_default_graph() -> 'Graph':
  g = getattr(_tls, 'graph', None)
  if g is None:
    raise RuntimeError('no default Graph: call forward functions inside `with graph.as_default():`')
  return g


class Graph:
  """One model scope: its variables, its ops in creation order, and the per-step scratch."""

  def __init__(self, scope: str = 'model', device='cuda', compute_dtype=torch.float32):
    self.scope = scope
    self.device = torch.device(device)
    self.compute_dtype = compute_dtype
    self.store = VarStore(scope)
    self.matmul_ops: List[MatmulOp] = []
    self.activation_ops: List[ActivationOp] = []
    self.nets: Dict[str, object] = {}          # cached net objects (tf.AUTO_REUSE)
    self.capturing = False                     # a hipGraph is recording this graph's step (step_graph.py): nothing per-step on the host
    self.step_feeders: List = []               # callables run before every replay of a recorded step (per-step host draws)
    self.training = True
    self.frozen = False                        # teacher: BN scale/shift cached
    self.act_slots: Optional[torch.Tensor] = None
    self._scratch: Optional[torch.Tensor] = None
    self._zero_row: Optional[torch.Tensor] = None
    self.fuse_conv1x1 = True                   # bf16 mode: defer BN/act/quant into 1x1 convolutions (pf_conv.hip)
    # channel pruning (host side): when `taps` is a dict, Conv2D / DepthwiseConv2D layers record
    # {layer: (input, output, producer-of-input)}; BN / activation / pooling layers pass the producer tag on
    self.taps: Optional[Dict[object, tuple]] = None
    self.tap_dense = False                     # also record Dense layers (input, MatMul output before the bias)
    self.tap_stop = None                       # layer after whose tap the forward pass is abandoned (TapStop)
    self._names: Dict[str, int] = {}
    self.reinflated: List[str] = []            # shrunk kernels a loader scattered back to full shape (gather_pays)
    self.kernel_params = self.kernel_params_kept = self.nb_gathered = 0   # set by inference.load_shrunk
    # int8 inference (inference.load_int8): quantising BatchNormAct layers whose consumers are all Conv2D / DepthwiseConv2D hand out
    # CodesAct, and the layers the loader packed multiply the codes on pf_conv_i8_fwd / pf_dw_i8_fwd; `int8_ran` collects the layers that did
    self.int8 = False
    self.nb_int8 = 0
    self.int8_ran: set = set()
    # fixed activation ranges (inference.load_int8(act_ranges='static')): every slot decoded ONCE to (alpha, beta) rows on the device.
    # Quantising BatchNormAct / Activation layers then quantise against their row with the clamping kernels (pf_act_static.hip) and
    # never touch the slots; a packed layer whose consumer BatchNormAct quantises applies it in its own epilogue (`requant_ran`).
    self.act_static: Optional[torch.Tensor] = None
    self.requant_ran: set = set()
    self._identity_ss: Dict[int, torch.Tensor] = {}
    self.conv_layers: List = []                # every Conv2D of the graph, in creation order (the loader finds a kernel's layer here)
    self.depthwise_layers: List = []           # every DepthwiseConv2D, likewise
    self.join_layers: List = []                # every BatchNormAddAct (the int8 / static loaders refuse a graph that has one)

  # -- naming like tf.layers (conv2d, conv2d_1, ...) ---------------------------------------------
  def unique_name(self, base: str) -> str:
    k = self._names.get(base, 0)
    self._names[base] = k + 1
    return base if k == 0 else '%s_%d' % (base, k)

  def as_default(self):
    graph = self

    class _Ctx:
      def __enter__(self_inner):
        self_inner.prev = getattr(_tls, 'graph', None)
        _tls.graph = graph
        return graph

      def __exit__(self_inner, *exc):
        _tls.graph = self_inner.prev
        return False
    return _Ctx()

  def add_matmul_op(self, op_type: str, name: str, var: Variable) -> MatmulOp:
    op = MatmulOp(op_type, self.scope + '/' + name, var)
    self.matmul_ops.append(op)
    return op

  def add_activation_op(self, op_type: str, name: str) -> ActivationOp:
    op = ActivationOp(op_type, self.scope + '/' + name, len(self.activation_ops))
    self.activation_ops.append(op)
    return op

  def apply_gathers(self, gathers: Dict[str, np.ndarray], values: Optional[Dict[str, np.ndarray]] = None) -> None:
    """Turn the named Conv2D kernels of a constructed, not yet finalised INFERENCE graph into physically shrunk ones: the artefact of
    tools/conversion/export_chn_pruned_model.py stores such a kernel as [kh, kw, len(gather), cout] plus the int32 vector of the kept
    input channels.  The variable's stored shape changes from cin to len(gather), the layer's cin is kept for checks, and the vector
    goes to the device once (finalize); Conv2D then runs on hip.conv_gather_fwd.  `values`: the kernels that will be loaded, to
    check their shapes here, where the message can name the variable.  Every rejection is a ValueError that names the variable."""
    if self.store.finalized:
      raise RuntimeError('apply_gathers: the graph is already finalised')
    for name, vec in gathers.items():
      var = self.store.by_name.get(name)
      if var is None:
        raise ValueError('%s: gather for a variable this graph does not have' % name)
      if var.kind != 'conv':
        raise ValueError('%s: a gather applies to Conv2D kernels only, this is a %s variable' % (name, var.kind))
      if var.gather_host is not None:
        raise ValueError('%s: the kernel already has a gather' % name)
      kh, kw, cin, cout = var.ref_shape
      g = check_gather(vec, cin, int(np.asarray(vec).size), what=name)
      if cin > GATHER_MAX_CIN:
        raise ValueError('%s: %d input channels, the gather kernel takes at most %d' % (name, cin, GATHER_MAX_CIN))
      shape = (kh, kw, int(g.size), cout)
      if values is not None and name in values and tuple(np.shape(values[name])) != shape:
        raise ValueError('%s: kernel of shape %s does not match its gather of %d kept channels (expected %s)'
                         % (name, tuple(np.shape(values[name])), g.size, shape))
      full_init = var.init
      var.cin_full, var.gather_host, var.ref_shape, var.numel = cin, g, shape, int(np.prod(shape))
      if full_init is not None:
        var.init = lambda rng, _f=full_init, _g=g: np.ascontiguousarray(_f(rng)[:, :, _g, :])

  def finalize(self, separate_compute: bool = False, seed: int = 42, requires_grad: bool = True) -> None:
    self.store.finalize(self.device, self.compute_dtype, separate_compute, seed, requires_grad)
    for v in self.store.vars:
      if v.gather_host is not None and v.gather is None:
        v.gather = torch.from_numpy(v.gather_host).to(self.device)
    n_act = max(len(self.activation_ops), 1)
    self.act_slots = torch.empty((n_act, 2), dtype=torch.int32, device=self.device)

  def begin_step(self) -> None:
    """Reset the activation min/max slots (ONE memset for all activations of the step)."""
    hip.minmax_slots_init(self.act_slots)
    self.store.w_t_fresh = False               # the quantiser rewrites the compute copy of the kernels every step

  def scratch(self, n_floats: int) -> torch.Tensor:
    if self._scratch is None or self._scratch.numel() < n_floats:
      self._scratch = torch.empty(max(n_floats, 1 << 20), dtype=torch.float32, device=self.device)
    return self._scratch

  def act_alpha_beta(self) -> torch.Tensor:
    return hip.minmax_decode(self.act_slots)

  def identity_scale_shift(self, C: int) -> torch.Tensor:
    """scale 1 / shift 0 as a [2][C] float32 pair: a stand-alone activation as the BN -> act -> quant pass sees it (fmaf(1, x, 0) = x)."""
    ss = self._identity_ss.get(C)
    if ss is None:
      ss = self._identity_ss[C] = torch.cat([torch.ones(C, dtype=torch.float32), torch.zeros(C, dtype=torch.float32)]).view(2, C).to(self.device)
    return ss

  def zero_row(self, C: int) -> torch.Tensor:
    """A float32 zero vector: the pivot row of BN statistics that were accumulated un-shifted."""
    if self._zero_row is None or self._zero_row.numel() < C:
      self._zero_row = torch.zeros(max(C, 4096), dtype=torch.float32, device=self.device)
    return self._zero_row


# =================================================================================================
# backward-filter launches on a second queue
# =================================================================================================

WRW_SIDE = os.environ.get('PF_WRW_SIDE', '1') != '0'


class WrwSide(object):
  """The backward-FILTER launches of the convolutions on a second HIP stream for the duration of one backward pass (round 6).

  In the backward pass of a layer only the backward-DATA product is on the critical path (dy -> dx -> the BN backward of the layer
  below); the filter gradient is read by the optimiser alone.  Issued in one queue the two alternate, and every launch of the chain
  (pixel-split filter kernel, its reduce, the BN sums' finalize -- 150 launches of 8-10 us a step) leaves the chip to one small grid.
  Armed by the optimisers' backward() for the variable store's graphs, a convolution's backward then forks: the side stream waits for the main stream (dy exists, the gradient
  buffer is zeroed), runs the filter kernel with its own split workspace, and the main stream goes on with backward-data.  The pass
  ends with ONE join.  dy / x of a forked launch are kept referenced until the join (the caching allocator would otherwise hand
  their memory to the main stream's next allocation while the side stream still reads it); only launches that write straight into
  the flat gradient buffer fork (no tensor allocated on the side stream outlives it).  Not inside a step-graph recording: there the
  forks would become edges of the hipGraph, which were measured to gain nothing in a replay and to cost one on small networks.  Data-parallel runs: the gradient notification of a forked launch is issued on the side stream (the
  reducer's staging copy and all-reduce of a bucket are ordered behind the launches that filled it; a bucket completed from the main
  stream waits for the side stream first, optim.GradReducer._stage_bucket).  PF_WRW_SIDE=0: one queue."""

  def __init__(self, device):
    self.device = device
    self.stream = torch.cuda.Stream(device=device)
    self.keep: List = []
    self._scratch: Optional[torch.Tensor] = None
    self.armed = False
    self.forks = 0

  def scratch(self, n_floats: int) -> torch.Tensor:
    if self._scratch is None or self._scratch.numel() < n_floats:
      with torch.cuda.stream(self.stream):
        self._scratch = torch.empty(max(n_floats, 1 << 20), dtype=torch.float32, device=self.device)
    return self._scratch

  def join(self) -> None:
    if self.forks:
      torch.cuda.current_stream(self.device).wait_stream(self.stream)
    self.keep.clear()
    self.forks = 0


class _WrwQueue(object):
  """`with _wrw_queue(graph, direct, dy, x) as scratch:` -- the filter launch inside runs on the side stream when one is armed and
  the launch writes into the flat gradient buffer; `scratch(n)` is the split workspace of the queue it runs on."""

  def __init__(self, graph, direct, tensors):
    side = getattr(getattr(graph, 'store', None), 'wrw_side', None)
    # not while a step graph is being recorded: the forks become edges of the hipGraph, which gain nothing in a replay (ResNet-50:
    # 23.4 ms either way) and cost one where the launches are small (ResNet-20: 2.25 -> 2.78 ms per replayed step, measured)
    self.side = side if (side is not None and side.armed and direct and not torch.cuda.is_current_stream_capturing()) else None
    self.graph, self.tensors, self.ctx = graph, tensors, None

  def __enter__(self):
    if self.side is None:
      return self.graph.scratch
    side = self.side
    side.stream.wait_stream(torch.cuda.current_stream(side.device))
    side.keep.append(self.tensors)
    side.forks += 1
    self.ctx = torch.cuda.stream(side.stream)
    self.ctx.__enter__()
    return side.scratch

  def __exit__(self, *exc):
    if self.ctx is not None:
      self.ctx.__exit__(*exc)
    return False


def _wrw_queue(graph, direct, *tensors):
  return _WrwQueue(graph, direct, tensors)


@contextlib.contextmanager
def wrw_side_armed(store: 'VarStore'):
  """One backward pass over the variables of `store` with the filter launches forked (see WrwSide); joins on the way out, also when
  the pass raises."""
  if not (WRW_SIDE and store is not None and getattr(store, 'device', None) is not None and torch.device(store.device).type == 'cuda'):
    yield
    return
  side = getattr(store, 'wrw_side', None)
  if side is None:
    side = store.wrw_side = WrwSide(store.device)
  side.armed = True
  try:
    yield
  finally:
    side.armed = False
    side.join()


# =================================================================================================
# autograd functions over the HIP kernels
# =================================================================================================

def _nhwc(x: torch.Tensor) -> torch.Tensor:
  if x.dim() == 4:
    return x.contiguous(memory_format=torch.channels_last)
  return x.contiguous()


def _bn_fast_ok(C: int) -> bool:
  """bn_fast_ok() of csrc/pf_bn.hip, asked of the library (pf_bn_vector_ok: a host query, no device work)."""
  return _bn_vector_ok(C)


def _bn_blocks(rows: int, C: int) -> int:
  """Number of row splits of the BN statistics passes (= entries per channel the finalize kernel
  reduces).  Fast path: 1024-thread workgroups over (channel slab x row split); ~256 workgroups."""
  if _bn_fast_ok(C):
    G = C // 8
    cg = 8 if G >= 8 else (G if G <= 2 else (4 if G <= 4 else 8))   # bn_cg_of(): a power of two, the last slab guarded
    nslab = -(-G // cg)
    row_lanes = 1024 // cg
    return int(max(1, min(256 // nslab, rows // (row_lanes * 2))))
  return int(min(256, max(1, rows // 64)))


class BnSums(object):
  """What a training-mode BatchNormAct shares with the convolutions that read its output, so that its ONE consumer's backward-data
  kernel can reduce the BN-backward sums in its epilogue.  BatchNormAct.__call__ makes it, the node's forward fills it and keeps it in
  its ctx, and the output carries it as `_pf_bn` (a materialised tensor and a LazyAct alike): the consumers count themselves in
  `n_consumers` (a consumer that cannot leave the sums counts twice) and the single one leaves `bwd_stats`.
  It holds the BN's INPUT, never the node's output or the LazyAct: that reference would close a cycle ctx -> record -> output ->
  grad_fn -> ctx which only Python's cyclic collector frees -- one step's activations (~10 GB at B = 256) alive for a random number
  of further steps, the caching allocator at the memory ceiling (measured: 26 GB reserved after 5 steps, 52 GB after 13; DESIGN.md
  section 6)."""
  __slots__ = ('x', 'scale_shift', 'mean_invstd', 'act', 'n_consumers', 'bwd_stats', 'deferred')

  def __init__(self):
    self.n_consumers = 0
    self.bwd_stats = None                        # (partial, n_blocks, data_ptr of the dq they are the sums of)
    self.deferred = None                         # (dy, wt, M, N, K, placeholder): that dq was never written (defer)

  def sums_for(self, dq):
    """(partial, n_blocks) where the single consumer's backward-data kernel already reduced THIS dq, else None."""
    bs = self.bwd_stats
    return bs[:2] if bs is not None and bs[2] == dq.data_ptr() else None

  def add_consumer(self, fuses: bool):
    """One more layer reads the BN's output: a consumer whose backward-data kernel can leave the BN-backward sums counts once, any
    other twice, so that `n_consumers == 1` means "exactly one consumer, and it fuses".  Called from ONE site per layer class
    (Conv2D.__call__, DepthwiseConv2D.__call__, LazyAct.materialize), keyed by the route the call takes:
      Conv2D   fused 1x1 reading a LazyAct            1        DepthwiseConv2D   own kernel           2
               fused 1x1 reading a materialised tensor 2       LazyAct.materialize                    2
               implicit GEMM                          1
               im2col, general kernel, library        2
    These count NOTHING, and that is kept as it was found: the tap (the plain call behind it counts as the route IT takes), gather,
    int8 / codes and the two stem routes of Conv2D, and the tap, codes and library routes of DepthwiseConv2D.  (The gather and codes
    routes run in inference only, where no record exists; the stems read images.)"""
    self.n_consumers += 1 if fuses else 2

  @staticmethod
  def sums_buffer(G: int, C: int, device):
    """The [G][2][C] float32 partial sums a backward-data launch with the BN-backward epilogue fills."""
    return torch.empty((G, 2, C), dtype=torch.float32, device=device)

  def leave(self, partial, G: int, dx):
    """After that launch: the sums of `dx`, for the BN node's backward to find (sums_for)."""
    self.bwd_stats = (partial, G, dx.data_ptr())

  def defer(self, partial, G: int, dy, wt, M: int, N: int, K: int, like):
    """After the sums-only launch (conv1x1_bwd_data_bnsums): the sums as `leave`, and what the BN node's apply pass needs to
    recompute dq = dy * wt in its own launch (conv1x1_bwd_data_bnapply), referenced until it ran.  Returns the gradient autograd
    carries to that node instead: a placeholder of x's shape that owns one element (a zero-stride expand), recognised there by its
    address (deferred_for) and never read."""
    placeholder = torch.empty(1, dtype=like.dtype, device=like.device).expand(like.shape)
    self.bwd_stats = (partial, G, placeholder.data_ptr())
    self.deferred = (dy, wt, M, N, K, placeholder)
    return placeholder

  def deferred_for(self, dq):
    """(dy, wt, M, N, K) where `dq` is the placeholder `defer` handed out, else None.  Taken once: the references go with it."""
    d = self.deferred
    if d is None or d[5].data_ptr() != dq.data_ptr():
      return None
    self.deferred = None
    return d[:5]


def _bn_enter(ctx, x, gamma, beta, layer, graph, training, slot, stats, rec=None, *more):
  """The forward prologue the BN nodes share: x in NHWC memory, the layer's scale / shift (_bn_scale_shift), and everything
  _bn_leave needs saved on ctx (`more`: further tensors to save behind the three).  Returns (x, rows, C, scale_shift)."""
  x = _nhwc(x)
  C = gamma.numel()
  rows = x.numel() // C
  scale_shift, mean_invstd = _bn_scale_shift(x, gamma, beta, layer, graph, training, slot, stats)
  ctx.save_for_backward(x, scale_shift, mean_invstd, *more)
  ctx.bn = (layer.act, graph, rows, C, (gamma, beta), not training, rec)
  if rec is not None:
    rec.x, rec.scale_shift, rec.mean_invstd, rec.act = x, scale_shift, mean_invstd, layer.act
  return x, rows, C, scale_shift


def _bn_leave(ctx, dq, pre=None, **kw):
  """(dx, dgamma, dbeta) of a node entered with _bn_enter for the gradient `dq` of the activated output: _bn_backward on the saved
  state, with the sums the single consumer left for this dq where it did (BnSums)."""
  x, scale_shift, mean_invstd = ctx.saved_tensors[:3]
  act, graph, rows, C, params, frozen, rec = ctx.bn
  if rec is not None:
    pre = rec.sums_for(dq)
    if pre is not None:
      kw['deferred'] = rec.deferred_for(dq)
    if rec.deferred is not None:                 # a placeholder went out and something else came back: there is no dq to fall back on
      raise RuntimeError('BN backward: the deferred input gradient of the consuming convolution did not arrive as handed out')
  return _bn_backward(dq, x, scale_shift, mean_invstd, act, graph, rows, C, params=params, pre=pre, frozen=frozen, **kw)


class _BnActQuant(torch.autograd.Function):
  """BN -> act -> activation fake-quant, fused (pf_bn_* kernels).  `training`: batch statistics.  Otherwise inference mode WITH
  gradients: the networks the pruning-ratio search re-trains are built with forward_eval (reference pr_optimizer.py:176-196 "DO NOT
  USE forward_train() HERE"), i.e. BN normalises with its moving statistics while gamma / beta (and everything upstream) are still
  trained.  y = act(scale * x + shift), scale = gamma * rsqrt(var + eps), shift = beta - mean * scale;
  dgamma = sum dy * (x - mean) * rsqrt(var + eps), dbeta = sum dy, dx = scale * dy  (same kernels as the training-mode backward:
  the statistics pass with the moving mean / invstd, the apply pass with zero sums)."""

  @staticmethod
  def forward(ctx, x, gamma, beta, layer, graph, training, slot, bits, stats=None, rec=None):
    x, rows, C, scale_shift = _bn_enter(ctx, x, gamma, beta, layer, graph, training, slot, stats, rec)
    quantize = bits is not None
    q = torch.empty_like(x)
    with region('bn_act_quant_apply', 2.0 * x.numel() * x.element_size()):   # 1 read of x + 1 write of q
      hip.bn_act_quant_apply(x, q, rows, C, scale_shift, layer.act, slot, bits if quantize else 8, quantize)
    return q

  @staticmethod
  def backward(ctx, dq):
    return _bn_leave(ctx, dq) + (None,) * 7


class _BnActPool(torch.autograd.Function):
  """The network head: BN -> act -> activation fake-quant -> mean over H, W, without the activated map in between
  (pf_bn_act_quant_pool; x.float().mean(dim=(2, 3)).to(x.dtype) of the q _BnActQuant would have written), in both of its modes.
  Returns [B][C]; backward takes its gradient and runs the pooled forms of the two BN-backward passes, dgamma / dbeta straight
  into the flat gradient views."""

  @staticmethod
  def forward(ctx, x, gamma, beta, layer, graph, training, slot, bits, stats=None):
    x, rows, C, scale_shift = _bn_enter(ctx, x, gamma, beta, layer, graph, training, slot, stats)
    ctx.hw = hw = rows // x.shape[0]
    quantize = bits is not None
    pooled = torch.empty((x.shape[0], C), dtype=x.dtype, device=x.device)
    with region('bn_act_quant_pool', float(x.numel() * x.element_size())):   # 1 read of x
      hip.bn_act_quant_pool(x, pooled, rows, C, hw, scale_shift, layer.act, slot, bits if quantize else 8, quantize)
    return pooled

  @staticmethod
  def backward(ctx, g):
    return _bn_leave(ctx, g.contiguous(), pool_hw=ctx.hw) + (None,) * 6


def head_fuse_ok(graph, x) -> bool:
  """The fused head takes this tensor: switch on, no taps, a float32 / bf16 GPU tensor and a library (or test double) with the
  entry points."""
  return (HEAD_FUSE and graph.taps is None and isinstance(x, torch.Tensor) and (x.is_cuda or HEAD_FUSE_ANY_DEVICE)
          and x.dtype in (torch.float32, torch.bfloat16)
          and hasattr(hip, 'bn_act_quant_pool') and hasattr(hip, 'bn_bwd_stats_pooled') and hasattr(hip, 'bn_bwd_apply_pooled'))


class _ActQuant(torch.autograd.Function):
  """act -> per-tensor fake-quant (pf_minmax_tensor + pf_uq_apply); backward = STE o act'."""

  @staticmethod
  def forward(ctx, u, act, slot, bits):
    u = _nhwc(u)
    y = torch.empty_like(u)
    hip.minmax_tensor(u, slot, act)
    hip.uq_apply(u, y, slot, bits, act)
    ctx.save_for_backward(u)
    ctx.act = act
    return y

  @staticmethod
  def backward(ctx, g):
    (u,) = ctx.saved_tensors
    g = _nhwc(g)
    if g.dtype != u.dtype:
      g = g.to(u.dtype)
    dx = torch.empty_like(u)
    hip.act_grad(g, u, dx, ctx.act)
    return dx, None, None, None


class _BnAddActQuant(torch.autograd.Function):
  """BN (batch statistics, or the moving ones with gradients) + shortcut -> act -> activation fake-quant: the tail of a ResNet-v1
  block in ONE pass over the tensor (pf_bn_add_act_fwd, which also leaves the range of the stored sum in the slot) plus the
  quantiser in place.  Backward is straight-through (as _ActQuant): pf_bn_add_act_bwd_gate recomputes the gate from x and the
  shortcut, writes g = dq * gate -- the shortcut's gradient as it stands -- and leaves the BN-backward sums of g, so that
  pf_bn_bwd_finalize / pf_bn_bwd_apply(act = none) on g finish the BN.
  Returns TWO aliases of the output (as _BnLazy does of its input): a block output has two consumers, the next block's first
  convolution and its shortcut (or projection).  Each reads its own alias, so their gradients arrive here separately and the gate
  pass forms the sum autograd would form with a separate add kernel (pf_bn_add_act_bwd_gate_add)."""

  @staticmethod
  def forward(ctx, x, shortcut, gamma, beta, layer, graph, training, slot, bits, stats=None):
    ctx.set_materialize_grads(False)               # an unused alias must arrive as None, not as a zeros tensor
    r = _nhwc(shortcut)
    # the BN (layer.bn) has no activation of its own and its output alone is never quantised: no slot for the finalize pass
    # (without an activation no gate reads the shortcut in backward: it is not kept)
    x, rows, C, scale_shift = _bn_enter(ctx, x, gamma, beta, layer.bn, graph, training, None, stats, None,
                                        *((r,) if layer.act is not None else ()))
    ctx.act = layer.act
    quantize = bits is not None
    nbytes = float(x.numel() * x.element_size())
    u = torch.empty_like(x)
    if quantize:
      hip.minmax_slots_init(slot)
    with region('bn_add_act_fwd', 3 * nbytes):       # reads x and the shortcut, writes u
      hip.bn_add_act_fwd(x, r, u, rows, C, scale_shift, layer.act, slot if quantize else None)
    if quantize:
      with region('uq_apply', 2 * nbytes):
        hip.uq_apply(u, u, slot, bits, None)         # in place; the activation is already applied
    # TWO views of u, as _BnLazy and _Fork return of their input -- never u and a view of it: the caller hangs the second alias on the
    # first (`_pf_skip`), and a view keeps its base alive from the C++ side, so `u._pf_skip = view of u` closes a cycle that not
    # even the cyclic collector sees; every step's block outputs stayed allocated for good (found at batch 256: out of memory
    # after some thirty steps of MobileNet-v2)
    return u.view_as(u), u.view_as(u)

  @staticmethod
  def backward(ctx, dq, dskip):
    x, scale_shift, mean_invstd = ctx.saved_tensors[:3]
    graph, rows, C = ctx.bn[1:4]
    if dq is None:
      dq, dskip = dskip, None
    if dq is None:
      return (None,) * 10

    def as_x(t):
      t = _nhwc(t)
      return t if t.dtype == x.dtype else t.to(x.dtype)
    dq = as_x(dq)
    dskip = as_x(dskip) if dskip is not None else None
    if ctx.act is None:
      # no gate: g is the arriving gradient -- with ONE consumer as it stands (no launch; the BN takes its own statistics pass),
      # with two their sum, formed by the gate pass's ADD form, which leaves the BN-backward sums as well.  That pass reads dq, the
      # addend and x and writes g; its shortcut operand is never loaded without an activation (x stands in for the pointer).
      if dskip is None:
        dx, dgamma, dbeta = _bn_leave(ctx, dq)
        return dx, dq, dgamma, dbeta, None, None, None, None, None, None
      nblk = hip.bn_add_act_groups(rows, C)
      partial = graph.scratch(nblk * 2 * C)
      g = torch.empty_like(x)
      with region('bn_add_act_bwd_gate', 4.0 * x.numel() * x.element_size()):
        hip.bn_add_act_bwd_gate(dq, x, x, g, rows, C, scale_shift, mean_invstd, None, partial, addend=dskip)
      dx, dgamma, dbeta = _bn_leave(ctx, g, pre=(partial, nblk))
      return dx, g, dgamma, dbeta, None, None, None, None, None, None
    r = ctx.saved_tensors[3]
    nblk = hip.bn_add_act_groups(rows, C)
    partial = graph.scratch(nblk * 2 * C)
    g = torch.empty_like(x)
    # reads dq (and the second consumer's gradient), x and the shortcut, writes g
    with region('bn_add_act_bwd_gate', (5.0 if dskip is not None else 4.0) * x.numel() * x.element_size()):
      hip.bn_add_act_bwd_gate(dq, x, r, g, rows, C, scale_shift, mean_invstd, ctx.act, partial, addend=dskip)
    dx, dgamma, dbeta = _bn_leave(ctx, g, pre=(partial, nblk))     # the BN behind the gate: no activation (layer.bn.act)
    return dx, g, dgamma, dbeta, None, None, None, None, None, None


class _Fork(torch.autograd.Function):
  """Two aliases of a tensor that has two consumers and no BatchNormAddAct behind it (the input of the first v1 bottleneck
  block: projection + conv1).  Backward sums the two gradients on pf_bn_add_act_fwd with scale 1 / shift 0 and no activation
  (fmaf(1, a, 0) + b = a + b, one rounding): the accumulation autograd would run as a separate aten kernel."""

  @staticmethod
  def forward(ctx, x, graph):
    ctx.graph = graph
    ctx.set_materialize_grads(False)
    return x.view_as(x), x.view_as(x)

  @staticmethod
  def backward(ctx, a, b):
    if a is None or b is None:
      return (a if a is not None else b), None
    a = _nhwc(a)
    b = _nhwc(b)
    if b.dtype != a.dtype:
      b = b.to(a.dtype)
    C = a.shape[1]
    out = torch.empty_like(a)
    with region('bn_add_act_fwd', 3.0 * a.numel() * a.element_size()):
      hip.bn_add_act_fwd(a, b, out, a.numel() // C, C, ctx.graph.identity_scale_shift(C), None, None)
    return out, None


def bn_join_tensor_ok(x) -> bool:
  """A tensor the join kernels (pf_bn_join.hip) take: 4-D, float32 / bf16, C % 8 == 0, on the GPU."""
  return (isinstance(x, torch.Tensor) and (x.is_cuda or BN_JOIN_ANY_DEVICE) and x.dim() == 4 and x.shape[1] % 8 == 0
          and x.dtype in (torch.float32, torch.bfloat16))


def fork(x, graph):
  """x, tagged with a second alias `x._pf_skip` for its second consumer, where the gradients of the two can be summed on the join
  kernels (training on the GPU); x as it is otherwise."""
  if bn_join_tensor_ok(x) and graph.taps is None and torch.is_grad_enabled() and x.requires_grad:
    x, x._pf_skip = _Fork.apply(x, graph)
  return x


# =================================================================================================
# BN -> act -> fake-quant deferred into the consuming 1x1 convolution (pf_conv.hip)
# =================================================================================================

class LazyAct(object):
  """The output of a BatchNormAct that has NOT been written to HBM.

  `x` is the raw (pre-BN) tensor; a consumer computes q = fake_quant(act(scale * x + shift)) itself:
  the fused 1x1 convolutions do it while staging their input tile (prologue of pf_conv1x1_fwd /
  pf_conv1x1_wrw), anything else calls `materialize()` (one pf_bn_act_quant_apply launch, cached).
  Gradients with respect to q flow into `x`'s autograd node (_BnLazy), which runs the BN backward once.
  """

  def __init__(self, x, scale_shift, act, slot, bits, rows, C, bn=None):
    self.x, self.scale_shift, self.act, self.slot, self.bits = x, scale_shift, act, slot, bits
    self.rows, self.C = rows, C
    self._pf_bn = bn                          # training mode only (BnSums): lets a consumer fuse the BN-backward statistics
    self.n_grad_consumers = 0                 # fused convolutions that read this activation and take part in the backward pass
    self.pending = None                       # dq of the first of TWO consumers, waiting to be joined by the second
    self.join_ok = False                      # set by the caller that KNOWS both consumers reach the loss (see _FusedConv1x1)
    self.pending_geom = None                  # geometry of a COMPACT parked gradient (a strided first consumer), else None
    self.dense_out = None                     # output channels of the stride-1 fused consumer that takes part in the backward pass
    self._q = None

  @property
  def shape(self):
    return self.x.shape

  @property
  def dtype(self):
    return self.x.dtype

  @property
  def device(self):
    return self.x.device

  def materialize(self) -> torch.Tensor:
    if self._pf_bn is not None:
      self._pf_bn.add_consumer(fuses=False)   # a materialised consumer: its gradient is summed by autograd
    if self._q is None:
      self._q = _Materialize.apply(self.x, self)
    return self._q


def materialize(x):
  return x.materialize() if isinstance(x, LazyAct) else x


class CodesAct(LazyAct):
  """The output of a quantising inference-mode BatchNormAct (bits <= 8) on a graph with `int8` set: a LazyAct that can also hand out
  the activation as uint8 CODES plus the decoded (alpha, beta) pair on the device (one pf_bn_act_quant_codes launch, cached) -- what a
  packed Conv2D multiplies on the i8 matrix cores and a packed DepthwiseConv2D on pf_dw_i8_fwd.  `materialize()` is unchanged: the fake-quantised float tensor of the apply pass,
  for every consumer that stays on the float kernels.  Inference only: there is no autograd node behind it."""

  def __init__(self, x, scale_shift, act, slot, bits, rows, C):
    super(CodesAct, self).__init__(x, scale_shift, act, slot, bits, rows, C)
    self._codes = None
    self.alpha_beta = None

  def codes(self):
    """(codes, alpha_beta): uint8 in x's NHWC memory order, float32[2] on the device (never read by the host)."""
    if self._codes is None:
      x = self.x
      self._codes = torch.empty(x.shape, dtype=torch.uint8, device=x.device, memory_format=torch.channels_last)
      self.alpha_beta = torch.empty(2, dtype=torch.float32, device=x.device)
      with region('bn_act_quant_codes', float(x.numel() * (x.element_size() + 1))):
        hip.bn_act_quant_codes(x, self._codes, self.rows, self.C, self.scale_shift, self.act, self.slot, self.bits, self.alpha_beta)
    return self._codes, self.alpha_beta


class StaticCodesAct(CodesAct):
  """CodesAct on a graph with fixed activation ranges (`graph.act_static`): `alpha_beta` is the layer's row of that tensor, there is no
  slot, and both forms come from the clamping pass pf_bn_act_quant_static.  Built either from the raw tensor `x` of a BatchNormAct
  (codes / values made on demand, one launch each, cached) or from the CODES a requantising producer wrote (`codes=`; x is None):
  then `materialize()` decodes them, alpha * (code / k) + beta in float32 and one rounding to `dtype` -- a cold path, for a consumer
  that refuses the codes at call time."""

  def __init__(self, x, scale_shift, act, alpha_beta, bits, rows, C, codes=None, dtype=None):
    super(StaticCodesAct, self).__init__(x if x is not None else codes, scale_shift, act, None, bits, rows, C)
    self._raw, self._codes, self.alpha_beta = x, codes, alpha_beta
    self._dtype = dtype if dtype is not None else x.dtype

  @property
  def dtype(self):
    return self._dtype

  def codes(self):
    if self._codes is None:
      x = self._raw
      self._codes = torch.empty(x.shape, dtype=torch.uint8, device=x.device, memory_format=torch.channels_last)
      with region('bn_act_quant_static', float(x.numel() * (x.element_size() + 1))):
        hip.bn_act_quant_static(x, self._codes, self.rows, self.C, self.scale_shift, self.act, self.alpha_beta, self.bits)
    return self._codes, self.alpha_beta

  def materialize(self) -> torch.Tensor:
    if self._q is None:
      x = self._raw
      if x is not None:
        self._q = torch.empty_like(x)
        with region('bn_act_quant_static', float(2 * x.numel() * x.element_size())):
          hip.bn_act_quant_static(x, self._q, self.rows, self.C, self.scale_shift, self.act, self.alpha_beta, self.bits)
      else:
        k = float(2 ** self.bits - 1)
        ab = self.alpha_beta
        self._q = (ab[0] * (self._codes.float() / k) + ab[1]).to(self._dtype).contiguous(memory_format=torch.channels_last)
    return self._q


class _Materialize(torch.autograd.Function):
  @staticmethod
  def forward(ctx, x, lazy):
    q = torch.empty_like(x)
    quant = lazy.bits is not None
    hip.bn_act_quant_apply(x, q, lazy.rows, lazy.C, lazy.scale_shift, lazy.act, lazy.slot if quant else None,
                           lazy.bits if quant else 8, quant)
    return q

  @staticmethod
  def backward(ctx, dq):
    return dq, None


def _bn_statistics(x, rows, C, graph, st=None):
  """(partial, n_blocks, pivot_row): from the producing convolution's epilogue when it left them
  (`st` = the tensor's `_pf_stats`), otherwise one pf_bn_stats pass over x."""
  if st is not None:
    partial, nblk = st
    return partial, nblk, graph.zero_row(C)
  nblk = _bn_blocks(rows, C)
  partial = graph.scratch(nblk * 4 * C)
  with region('bn_stats', float(x.numel() * x.element_size())):
    hip.bn_stats(x, rows, C, partial, nblk)
  return partial, nblk, x


def _bn_scale_shift(x, gamma, beta, layer, graph, training, slot, stats=None):
  """(scale_shift, mean_invstd) of `layer` applied to x, each [2][C] float32.  `training`: batch statistics (`stats` as in
  _bn_statistics) finalized on the device, which also updates the moving statistics and, with a `slot`, leaves the activated
  tensor's min / max there.  Otherwise inference mode with gradients: the moving statistics, gamma / beta as constants."""
  C = gamma.numel()
  scale_shift = torch.empty((2, C), dtype=torch.float32, device=x.device)
  if training:
    rows = x.numel() // C
    mean_invstd = torch.empty((2, C), dtype=torch.float32, device=x.device)
    partial, nblk, piv = _bn_statistics(x, rows, C, graph, stats)
    hip.bn_finalize(partial, nblk, rows, C, piv, gamma, beta, layer.moving_mean.tensor, layer.moving_var.tensor,
                    layer.momentum, layer.eps, True, layer.act, scale_shift, mean_invstd, slot)
  else:
    hip.bn_eval_scale_shift(gamma.detach(), beta.detach(), layer.moving_mean.tensor, layer.moving_var.tensor,
                            layer.eps, scale_shift)
    mean_invstd = torch.stack([layer.moving_mean.tensor.float(),
                               torch.rsqrt(layer.moving_var.tensor.float() + layer.eps)]).contiguous()
  return scale_shift, mean_invstd


class _BnLazy(torch.autograd.Function):
  """BN statistics + finalize only; returns an alias of x that stands for q (see LazyAct)."""

  @staticmethod
  def forward(ctx, x, gamma, beta, layer, graph, slot, rec, stats):
    ctx.set_materialize_grads(False)          # an unused shortcut alias must arrive as None, not as a zeros tensor
    x = _bn_enter(ctx, x, gamma, beta, layer, graph, True, slot, stats, rec)[0]
    # two aliases of x: the first stands for q (consumed by the fused convolutions), the second is x
    # itself for the block's identity shortcut -- routing the shortcut through this node lets the
    # backward add its gradient inside pf_bn_bwd_apply_add instead of a separate accumulation kernel
    return x.view_as(x), x.view_as(x)

  @staticmethod
  def backward(ctx, dq, dskip):
    if dq is None:
      return (dskip,) + (None,) * 7
    return _bn_leave(ctx, dq, addend=dskip) + (None,) * 5


def _grad_view(t: Optional[torch.Tensor], n: int):
  """The pre-allocated flat-buffer gradient view of a leaf (VarStore.finalize), if it can be written directly."""
  g = getattr(t, 'grad', None) if t is not None else None
  if g is not None and g.dtype == torch.float32 and g.is_contiguous() and g.numel() == n:
    return g
  return None


def _bn_backward(dq, x, scale_shift, mean_invstd, act, graph, rows, C, addend=None, params=None, pre=None,
                 frozen=False, pool_hw=None, deferred=None):
  """Returns (dx, dgamma, dbeta); when `params` = (gamma leaf, beta leaf) carry flat-buffer gradient views,
  dgamma / dbeta are written there by pf_bn_bwd_finalize and None is returned for them (no accumulation
  kernels; every BN layer is applied once per step and the buffers are zeroed by the optimiser).
  `frozen`: inference-mode BN (moving statistics are constants): the batch-statistics terms of dx vanish,
  dx = scale * dy -- the same apply kernel fed with zero sums.
  `pool_hw`: dq is the [B][C] gradient of the POOLED tensor (_BnActPool); both passes rebuild the per-pixel value from it.
  `deferred` = (dy, wt, M, N, K) (BnSums.defer; with `pre`, training mode, not pooled): dq is a placeholder -- the single consumer's
  backward-data left the sums and no dq, and the apply pass is that GEMM again with the BN backward as its row pass
  (conv1x1_bwd_data_bnapply: the same bits as the stored dq through bn_bwd_apply, without its write and read)."""
  if deferred is not None:
    assert pre is not None and not frozen and pool_hw is None
  else:
    dq = _nhwc(dq)
    if dq.dtype != x.dtype:
      dq = dq.to(x.dtype)
  if addend is not None:
    addend = _nhwc(addend)
    if addend.dtype != x.dtype:
      addend = addend.to(x.dtype)
  nbytes = float(x.numel() * x.element_size())
  if pool_hw is not None:
    # the pooled passes read x and the small pooled gradient; the apply pass also writes dx
    stats_pass = ('bn_bwd_stats_pooled', nbytes, hip.bn_bwd_stats_pooled, (pool_hw,))
    apply_pass = ('bn_bwd_apply_pooled', 2 * nbytes, hip.bn_bwd_apply_pooled, (pool_hw,), ())
  else:
    # the plain passes read dq and x; the apply pass also reads the addend and writes dx
    stats_pass = ('bn_bwd_stats', 2 * nbytes, hip.bn_bwd_stats, ())
    apply_pass = ('bn_bwd_apply', (4 if addend is not None else 3) * nbytes, hip.bn_bwd_apply, (), (addend,))
  if pre is not None:
    partial, nblk = pre
  else:
    nblk = _bn_blocks(rows, C)
    partial = graph.scratch(nblk * 2 * C)
    name, traffic, launch, hw = stats_pass
    with region(name, traffic):
      launch(dq, x, rows, C, *hw, scale_shift, mean_invstd, act, partial, nblk)
  gview = _grad_view(params[0], C) if params is not None else None
  bview = _grad_view(params[1], C) if params is not None else None
  direct = gview is not None and bview is not None
  dgamma = gview if direct else torch.empty(C, dtype=torch.float32, device=x.device)
  dbeta = bview if direct else torch.empty(C, dtype=torch.float32, device=x.device)
  hip.bn_bwd_finalize(partial, nblk, C, dgamma, dbeta)
  dx = torch.empty_like(x)
  zero = graph.zero_row(C)[:C] if frozen else None
  name, traffic, launch, hw, tail = apply_pass
  if deferred is not None:
    dy, wt, M, N, K = deferred
    # reads dy (N of K channels wide), x and the addend, writes dx
    with region(name, (3 if addend is not None else 2) * nbytes + float(dy.numel() * dy.element_size())):
      hip.conv1x1_bwd_data_bnapply(dy, wt, x, scale_shift, mean_invstd, act, dgamma, dbeta, addend, dx, M, N, K)
    return (dx, None, None) if direct else (dx, dgamma, dbeta)
  with region(name, traffic):
    launch(dq, x, dx, rows, C, *hw, scale_shift, mean_invstd, zero if frozen else dgamma, zero if frozen else dbeta, act,
           *tail)
  return (dx, None, None) if direct else (dx, dgamma, dbeta)


def _filter_grad(graph, w, w_var, keep, name, nbytes, launch):
  """The filter gradient of the convolution kernel `w` (logical [N][C][R][S] over KRSC memory; depthwise [C][1][k][k]), computed by
  `launch(target, scratch)`: `target` is the gradient in STORAGE layout ([N][R][S][C]), `scratch(n)` the float32 split workspace of
  the queue the launch runs on.  The target is the leaf's gradient view inside the flat gradient buffer where there is one: written
  directly (each kernel is used once per step; the optimiser zeroes the buffer), no accumulation kernel.  Autograd then sees no
  gradient for this leaf (None is returned), so it is reported here, on the launch's queue.  Any other `w` -- no gradient yet, or one
  that is not laid out in storage order -- gets a fresh tensor, returned in the logical layout for autograd to accumulate.  (`w.grad`
  always has the shape and dtype of `w`, torch refuses any other: what decides is the layout.)  `keep`: every tensor the launch
  reads, referenced until the side queue is joined (WrwSide)."""
  gw = getattr(w, 'grad', None)
  direct = gw is not None and gw.shape == w.shape and gw.dtype == w.dtype and gw.permute(0, 2, 3, 1).is_contiguous()
  target = (gw.permute(0, 2, 3, 1) if direct
            else torch.empty((w.shape[0], w.shape[2], w.shape[3], w.shape[1]), dtype=w.dtype, device=w.device))
  with _wrw_queue(graph, direct, *keep) as scratch, region(name, nbytes):
    launch(target, scratch)
    if direct:
      graph.store.notify_grad(w_var)
  return None if direct else target.permute(0, 3, 1, 2)


def _bwd_data_weight(graph, w_var, w):
  """The kernel in backward-data layout, W'[c][R-1-r][S-1-s][n] = W[n][r][s][c]: a view of the store's transposed buffer (one launch
  for all kernels of the step) when `w` is that variable's tensor, else a copy made here."""
  if USE_SEG_TRANSPOSE and w_var is not None and w_var.store is graph.store and w_var.tensor is w:
    return graph.store.transposed(w_var)
  return w.detach().permute(0, 2, 3, 1).flip(1, 2).permute(3, 1, 2, 0).contiguous()


def _krsc(w, dtype):
  """The kernel `w` (logical [N][C][R][S]) as a contiguous [N][R][S][C] tensor of `dtype`: a view where it is stored that way."""
  wk = w.detach().permute(0, 2, 3, 1)
  if not wk.is_contiguous() or wk.dtype != dtype:
    wk = wk.contiguous().to(dtype)
  return wk


def _out_size(size: int, k: int, stride: int, pad_total: int) -> int:
  """Output pixels along one axis of a k-wide window moved by `stride` over `size` pixels padded by `pad_total` (both ends together)."""
  return (size + pad_total - k) // stride + 1


def _wants_grad(w, x=None) -> bool:
  """A layer call takes part in the backward pass: gradients are enabled and the kernel `w` or the input `x` asks for one.  (Without
  `x`: the MobileNet stem, whose image never does.)"""
  return torch.is_grad_enabled() and (w.requires_grad or (x is not None and x.requires_grad))


def _library_conv_backward(dy, x, w, stride, pad, which: int):
  """The library's backward of a dense convolution: the data gradient (`which` = 0) or the filter gradient (1).  What remains of it
  are the A/B switches' other side, geometries outside the kernels' limits and the ResNet stem's image gradient."""
  return torch.ops.aten.convolution_backward(dy, x, w.detach(), None, [stride, stride], list(pad), [1, 1], False, [0, 0], 1,
                                             [which == 0, which == 1, False])[which]


def _apply_with_stats(fn, *args):
  """`fn.apply(*args, box)` for the convolutions whose forward kernel leaves the BN statistics of its output: apply() wraps the
  result in a new tensor object, so forward hands `_pf_stats` over in `box` and it is put back on the tensor here."""
  box = []
  y = fn.apply(*args, box)
  if box[0] is not None:
    y._pf_stats = box[0]
  return y


def _conv1x1_geom(x_shape, stride):
  """(M, geom) of a 1x1 convolution over a logical-NCHW / physical-NHWC input."""
  n, _, h, w = x_shape
  if stride == 1:
    return n * h * w, None, (h, w)
  ho, wo = -(-h // stride), -(-w // stride)
  return n * ho * wo, (ho, wo, h, w, stride), (ho, wo)


def _run_conv1x1(x, w2d, lazy, residual, want_stats, stride, out_bn=None):
  N, K = w2d.shape
  M, geom, (ho, wo) = _conv1x1_geom(x.shape, stride)
  y = torch.empty((x.shape[0], N, ho, wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
  if out_bn is not None:
    # the consumer's inference-mode BN + activation in the epilogue (pf_conv1x1_fwd_affine): y IS that layer's output
    with region('conv1x1_fwd', float((M * K + M * N) * 2)):
      hip.conv1x1_fwd(x, w2d, y, M, N, K, scale_shift=lazy.scale_shift if lazy is not None else None,
                      act=lazy.act if lazy is not None else None, geom=geom, out_scale_shift=out_bn._eval_scale_shift(y),
                      out_act=out_bn.act)
    y._pf_bn_done = out_bn
    return y
  partial, G = None, 0
  if want_stats:
    G = hip.conv1x1_stats_groups(M, N, K, prologue=lazy is not None)
    partial = torch.empty((G, 4, N), dtype=torch.float32, device=x.device)
  ss = lazy.scale_shift if lazy is not None else None
  quant = lazy is not None and lazy.bits is not None
  nbytes = float((M * K + M * N * (2 if residual is not None else 1)) * 2)
  with region('conv1x1_fwd', nbytes):
    hip.conv1x1_fwd(x, w2d, y, M, N, K, R=residual, scale_shift=ss, act=lazy.act if lazy is not None else None,
                    slot=lazy.slot if quant else None, bits=lazy.bits if quant else 8, partial=partial, geom=geom)
  if want_stats:
    y._pf_stats = (partial, G)
  return y


def _conv1x1_bwd_data_plan(lazy, bn, geom, act, M: int, N: int, K: int, dtype=None):
  """How _FusedConv1x1.backward computes its input gradient: (launch, outcome, alloc), decided here and nowhere else, from the
  producer's LazyAct and BnSums record (None: a materialised input / no training-mode BN), the row map `geom` of a strided layer,
  the producer's activation, the GEMM shape and the switches as they stand at this call.
    launch   the ONE launch:  'compact' | 'join_stats' | 'join' | 'bnstats' | 'bnsums' | 'residual' | 'plain' (with the row scatter
             when strided)
    outcome  'parked' on the LazyAct for the second consumer | 'delivered' together with the parked gradient | 'plain'
    alloc    dx is 'compact' ([B][K][Ho][Wo]) | 'empty' | 'zeros' (the row scatter writes every stride-th pixel) | 'deferred' (none)
  'bnstats': the single consumer of a ReLU / ReLU6 BN leaves the BN-backward sums of its dx (BnSums), stride 1 only.
  'bnsums': the same sums WITHOUT the dx (where the loaded library offers the pair and its plan takes the shape and `dtype`, bfloat16:
  conv1 of an identity bottleneck block in stages 1-2).  The BN node's apply pass is dx's one reader; it recomputes the product in
  its own launch (BnSums.defer, _bn_backward), so the 4C-wide dx is neither written nor read.  PF_BN1_RECOMPUTE=0: 'bnstats'.
  The join: an activation with exactly TWO fused consumers (bn1 of a projection block: shortcut convolution + conv1): the consumer
  whose backward runs first parks its dq on the LazyAct and reports no gradient; the second takes it as the residual operand of its
  backward-data kernel ('residual') -- the sum autograd would form with a separate add kernel (two reads and one write of the
  4C-channel tensor) costs one extra read.  The block calls conv1 BEFORE the shortcut convolution, so the (possibly strided,
  zero-filled) shortcut gradient comes first and the dense one joins it; a strided second consumer has no residual operand under its
  row map and adds the parked gradient behind its launch.  Opt-in (`lazy.join_ok`, set by the bottleneck block): a parked gradient is
  only delivered by the second consumer's backward, so both consumers must be known to reach the loss.
  The projection join (pf_conv1x1_bwd_data_join), where the loaded library offers it and its plan takes the dense consumer's shape:
  a strided first consumer parks a COMPACT [B][K][Ho][Wo] gradient -- a plain dense GEMM, no zero fill, no row scatter ('compact')
  -- which the second reads through the inverse row map ('join'); and the second takes the BN-backward sums of the joined gradient
  in the same launch ('join_stats'), so that _BnLazy.backward finds them (BnSums.bwd_stats) and skips its statistics pass."""
  relu = act in ('Relu', 'Relu6')
  join = JOIN_TWO_CONSUMERS and bn is not None and lazy.join_ok and bn.n_consumers == 2 and lazy.n_grad_consumers == 2
  alloc = 'empty' if geom is None else 'zeros'
  if not join:
    fuse_stats = FUSE_BN_BWD_STATS and bn is not None and bn.n_consumers == 1 and geom is None and relu
    if fuse_stats and BN1_RECOMPUTE and dtype is not None:
      pair_plan = getattr(hip, 'conv1x1_bwd_apply_plan', None)          # (the library's: zero for anything but bfloat16)
      if (pair_plan is not None and getattr(hip, 'conv1x1_bwd_data_bnsums', None) is not None
          and getattr(hip, 'conv1x1_bwd_data_bnapply', None) is not None and pair_plan(M, N, K, dtype) != 0):
        return 'bnsums', 'plain', 'deferred'
    return ('bnstats' if fuse_stats else 'plain'), 'plain', alloc
  join_entry = getattr(hip, 'conv1x1_bwd_data_join', None) if PROJ_JOIN else None
  if lazy.pending is None:                       # the first of the two
    if geom is not None and join_entry is not None and lazy.dense_out is not None:
      rows = M // (geom[0] * geom[1]) * geom[2] * geom[3]                      # pixels of the dense consumer's (= the full) map
      if hip.conv1x1_join_plan(rows, lazy.dense_out, K) != 0:
        return 'compact', 'parked', 'compact'
    return 'plain', 'parked', alloc
  if geom is not None:                           # the second, strided
    return 'plain', 'delivered', alloc
  if join_entry is not None and PROJ_JOIN_STATS and FUSE_BN_BWD_STATS and relu and hip.conv1x1_join_plan(M, N, K, True) != 0:
    return 'join_stats', 'delivered', alloc
  return ('join' if lazy.pending_geom is not None else 'residual'), 'delivered', alloc


class _FusedConv1x1(torch.autograd.Function):
  """y = conv1x1(Q(x), W) [+ residual], Q = the producer BN's normalise/act/fake-quant (prologue)."""

  @staticmethod
  def forward(ctx, x, w, residual, lazy, want_stats, stride, graph, w_var, box):
    w2d = w.detach().permute(0, 2, 3, 1).reshape(w.shape[0], w.shape[1])      # [N][K] (KRSC, R=S=1)
    res = _nhwc(residual) if residual is not None else None
    y = _run_conv1x1(x, w2d, lazy, res, want_stats, stride)
    ctx.save_for_backward(x, w2d)
    ctx.meta = (lazy, stride, graph, residual is not None, w.shape)
    ctx.w_leaf = w
    ctx.w_var = w_var
    box.append(getattr(y, '_pf_stats', None))
    return y

  @staticmethod
  def backward(ctx, dy):
    x, w2d = ctx.saved_tensors
    lazy, stride, graph, has_res, w_shape = ctx.meta
    dy = _nhwc(dy)
    N, K = w2d.shape
    M, geom, _ = _conv1x1_geom(x.shape, stride)
    ss = lazy.scale_shift if lazy is not None else None
    quant = lazy is not None and lazy.bits is not None
    act = lazy.act if lazy is not None else None
    bn = lazy._pf_bn if lazy is not None else None                             # the producer BN's record (BnSums), training mode
    dx = dw = None
    if ctx.needs_input_grad[1]:
      S = hip.conv1x1_wrw_splits(M, N, K)

      def wrw(dwk, scratch):                     # dwk: [N][1][1][K] memory = [N][K]
        hip.conv1x1_wrw(dy, x, dwk.view(N, K), scratch((S + 32) * N * K), M, N, K, scale_shift=ss, act=act,
                        slot=lazy.slot if quant else None, bits=lazy.bits if quant else 8, geom=geom)
      # (everything the launch reads stays referenced until the join: the producer BN's constants belong to ITS autograd node, which
      # runs -- and frees them -- on the main stream right after this function returns)
      dw = _filter_grad(graph, ctx.w_leaf, ctx.w_var, (dy, x, w2d, ss, lazy), 'conv1x1_wrw', float((M * K + M * N) * 2), wrw)
    if ctx.needs_input_grad[0]:
      wt = _bwd_data_weight(graph, ctx.w_var, ctx.w_leaf).view(K, N)           # [K][N]
      launch, outcome, alloc = _conv1x1_bwd_data_plan(lazy, bn, geom, act, M, N, K, x.dtype)
      if alloc == 'compact':
        dx = torch.empty((x.shape[0], K, geom[0], geom[1]), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
      elif alloc != 'deferred':
        dx = torch.empty_like(x) if alloc == 'empty' else torch.zeros_like(x)
      res = lazy.pending if launch in ('join_stats', 'join', 'residual') else None
      with region('conv1x1_bwd_data', float((M * K * {'compact': 1, 'plain': 1, 'bnsums': 1}.get(launch, 2) + M * N) * 2)):
        leaves_sums = launch in ('join_stats', 'bnstats', 'bnsums')
        if leaves_sums:
          G = hip.conv1x1_stats_groups(M, K, N)
          partial = bn.sums_buffer(G, K, x.device)
        if launch == 'compact':
          hip.conv1x1_fwd(dy, wt, dx, M, K, N)
        elif launch == 'join_stats':
          hip.conv1x1_bwd_data_join(dy, wt, dx, res, M, N, K, rgeom=lazy.pending_geom, bn_x=x, bn_scale_shift=bn.scale_shift,
                                    bn_mean_invstd=bn.mean_invstd, bn_act=act, partial=partial)
        elif launch == 'join':
          hip.conv1x1_bwd_data_join(dy, wt, dx, res, M, N, K, rgeom=lazy.pending_geom)
        elif launch == 'bnstats':
          hip.conv1x1_bwd_data_bnstats(dy, wt, dx, x, bn.scale_shift, bn.mean_invstd, act, partial, M, N, K)
        elif launch == 'bnsums':
          hip.conv1x1_bwd_data_bnsums(dy, wt, x, bn.scale_shift, bn.mean_invstd, act, partial, M, N, K)
        elif launch == 'residual':
          hip.conv1x1_fwd(dy, wt, dx, M, K, N, R=res)
        else:
          hip.conv1x1_fwd(dy, wt, dx, M, K, N, geom=geom, ymap=geom is not None)
        if launch == 'bnsums':
          dx = bn.defer(partial, G, dy, wt, M, N, K, x)
        elif leaves_sums:
          bn.leave(partial, G, dx)
      if outcome == 'parked':
        lazy.pending, dx = dx, None             # the second consumer delivers the sum
        lazy.pending_geom = geom if launch == 'compact' else None
      elif outcome == 'delivered':
        if res is None:
          dx = dx + lazy.pending                # the second one is the strided one: no residual operand under a row map
        lazy.pending = lazy.pending_geom = None
    return dx, dw, (dy if has_res else None), None, None, None, None, None, None


# two fused consumers of one activation: join their input gradients inside the second backward-data kernel (0: autograd add)
JOIN_TWO_CONSUMERS = os.environ.get('PF_JOIN_TWO_CONSUMERS', '1') != '0'
# projection blocks: the strided shortcut's input gradient stays compact and conv1's backward-data reads it through the inverse row
# map (0: the zero-filled full-size tensor and the row scatter); ..._STATS: the BN-backward sums of bn1 in that launch (0: pf_bn_bwd_stats)
PROJ_JOIN = os.environ.get('PF_PROJ_JOIN', '1') != '0'
PROJ_JOIN_STATS = os.environ.get('PF_PROJ_JOIN_STATS', '1') != '0'
# identity blocks of stages 1-2: conv1's input gradient is never written -- sums-only backward-data, then bn1's apply pass recomputes
# the product in its own launch (0: the backward-data that stores it + pf_bn_bwd_apply_add, for A/B runs)
BN1_RECOMPUTE = os.environ.get('PF_BN1_RECOMPUTE', '1') != '0'
USE_SEG_TRANSPOSE = os.environ.get('PF_SEG_TRANSPOSE', '1') != '0'   # backward-data kernel layouts in one launch (0: aten)
OWN_POOL = os.environ.get('PF_OWN_POOL', '1') != '0'         # stem max-pooling on pf_pool.hip (0: aten, for A/B runs)
# backward-filter of the RxS convolutions on pf_wrw.hip (shared-tile kernel); PF_OWN_CONV2D_WRW=0: MIOpen, for A/B runs
OWN_CONV2D_WRW = os.environ.get('PF_OWN_CONV2D_WRW', '1') != '0'
OWN_CONV2D_WRW_MIN_C = int(os.environ.get('PF_OWN_CONV2D_WRW_MIN_C', '64'))    # (round 3: 128 -- MIOpen was faster at C = 64; round 4, per step in one box: 9 633 vs 9 590 images/s with ours)
OWN_CONV2D_BWD_STRIDED = os.environ.get('PF_OWN_CONV2D_BWD_STRIDED', '1') != '0'   # strided backward-data by parity classes (0: MIOpen)
OWN_CONV2D = os.environ.get('PF_OWN_CONV2D', '1') != '0'     # RxS convolutions on pf_igemm.hip (0: MIOpen, for A/B runs)
OWN_STEM = os.environ.get('PF_OWN_STEM', '1') != '0'         # the 7x7/2 stem on pf_stem.hip (0: MIOpen, for A/B runs)
OWN_DEPTHWISE = os.environ.get('PF_OWN_DEPTHWISE', '1') != '0'   # depthwise 3x3 on pf_depthwise.hip (0: MIOpen, for A/B runs)
OWN_CONV_IM2COL = os.environ.get('PF_OWN_CONV_IM2COL', '1') != '0'   # few-channel RxS convolutions as im2col + own 1x1 kernels (0: MIOpen)
CONVG_BF16_NARROW = os.environ.get('PF_CONVG_BF16_NARROW', '0') != '0'
# inference-mode BN + activation applied in the epilogue of the producing convolution (teacher / evaluation of unquantised networks)
FOLD_EVAL_BN = os.environ.get('PF_FOLD_EVAL_BN', '1') != '0'
OWN_CONV_GENERIC = os.environ.get('PF_OWN_CONV_GENERIC', '1') != '0'   # every other convolution / dense layer on pf_convg.hip (0: MIOpen / rocBLAS)
DEPTHWISE_ANY_DEVICE = False     # tests: run the depthwise plumbing on CPU tensors (the HIP entry points are emulated there)
# a depthwise layer applies its producer's BN + activation (+ fake-quant) in its own prologue instead of reading a materialised tensor
# (pf_depthwise_fwd_act / pf_depthwise_wrw_act).  PF_DW_LAZY=1: every layer that can; 0: none; unset: where `dw_lazy_pays` says so
DW_LAZY_ACTS = (None, 'Relu6')     # the activations pf_depthwise_*_act are built for (a ReLU producer materialises)
DW_LAZY: Optional[bool] = {'0': False, '1': True}.get(os.environ.get('PF_DW_LAZY', ''))


def _run_conv2d(x, w_krsc, stride, pad, want_stats, out_bn=None):
  """x: logical NCHW / physical NHWC bf16, w_krsc: contiguous [N][R][S][C] bf16."""
  B, C, H, W = x.shape
  N, R, S, _ = w_krsc.shape
  Ho, Wo = _out_size(H, R, stride, 2 * pad[0]), _out_size(W, S, stride, 2 * pad[1])
  y = torch.empty((B, N, Ho, Wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
  M = B * Ho * Wo
  if out_bn is not None:                         # the consumer's inference-mode BN + activation in the epilogue (pf_conv2d_fwd_affine)
    with region('conv2d_fwd', float((B * H * W * C + M * N) * 2)):
      hip.conv2d_fwd(x, w_krsc, y, B, H, W, C, N, R, S, stride, pad[0], pad[1], Ho, Wo,
                     out_scale_shift=out_bn._eval_scale_shift(y), out_act=out_bn.act)
    y._pf_bn_done = out_bn
    return y
  partial, G = None, 0
  if want_stats:
    G = hip.conv2d_stats_groups(M, N, geom=(B, H, W, C, N, R, S, stride, pad[0], pad[1], Ho, Wo))
    partial = torch.empty((G, 4, N), dtype=torch.float32, device=x.device)
  with region('conv2d_fwd', float((B * H * W * C + M * N) * 2)):
    hip.conv2d_fwd(x, w_krsc, y, B, H, W, C, N, R, S, stride, pad[0], pad[1], Ho, Wo, partial=partial)
  if want_stats:
    y._pf_stats = (partial, G)
  return y


class _Conv2dIgemm(torch.autograd.Function):
  """y = conv2d(x, W) on the implicit-GEMM kernel (pf_conv2d_fwd), x a materialised bf16 NHWC activation.
  Backward-data of stride-1 convolutions runs on the same kernel with the flipped / transposed kernel and reduces the
  BN-backward sums of x's producer BN in its epilogue; strided backward-data runs on it by output-parity classes
  (pf_conv2d_bwd_data_strided), backward-filter on pf_wrw.hip (conv2d_wrw).  The library calls that remain below are the A/B
  switches' other side and geometries outside the kernels' limits (channel counts, 31-bit offsets)."""

  @staticmethod
  def forward(ctx, x, w, stride, pad, want_stats, graph, bn_sums, w_var, box):
    ctx.w_var = w_var
    w_krsc = w.detach().permute(0, 2, 3, 1)              # physical layout of the kernel: contiguous [N][R][S][C]
    y = _run_conv2d(x, w_krsc, stride, pad, want_stats)
    ctx.save_for_backward(x, w)
    ctx.meta = (stride, pad, graph, bn_sums)
    box.append(getattr(y, '_pf_stats', None))
    return y

  @staticmethod
  def backward(ctx, dy):
    x, w = ctx.saved_tensors
    stride, pad, graph, bn_sums = ctx.meta
    dy = _nhwc(dy)
    dx = dw = None
    N, C, R, S = w.shape
    B, _, H, W = x.shape
    Ho, Wo = dy.shape[2], dy.shape[3]
    if ctx.needs_input_grad[1]:
      # C = 64: the [64 x 64] tile per tap is too small to feed the matrix cores (measured 256 vs 168 us against MIOpen on
      # the 56x56 layer, tools/gpu/wrw_bench.py); from C = 128 up the shared-tile kernel is on par or ahead
      splits = hip.conv2d_wrw_splits(B * Ho * Wo, N, C, R * S) if (OWN_CONV2D_WRW and C >= OWN_CONV2D_WRW_MIN_C) else 0
      nbytes = float((x.numel() + dy.numel()) * 2)
      if splits > 0:
        def wrw(dwk, scratch):
          hip.conv2d_wrw(dy, x, dwk, scratch((splits + 32) * N * R * S * C), B, H, W, C, N, R, S, stride, pad[0], pad[1], Ho, Wo)
        dw = _filter_grad(graph, w, ctx.w_var, (dy, x), 'conv2d_wrw', nbytes, wrw)
      elif OWN_CONV2D_WRW and OWN_CONV_GENERIC and x.is_cuda and dy.dtype == x.dtype and w.dtype == x.dtype:
        # fewer than 2 048 output pixels (the 64 x 64 test networks): too few steps for the pixel-split MFMA kernels -- the general
        # kernel (round 6; MIOpen until then: VERDICT r5 weak #1 "those parity lines partly measure the library")
        gs = hip.convg_wrw_splits(B, C, N, R, S, Ho, Wo)
        dwk = torch.empty((N, R, S, C), dtype=w.dtype, device=x.device)
        with region('conv2d_wrw', nbytes):
          hip.convg_wrw(dy, x, dwk, graph.scratch(gs * N * R * S * C), B, H, W, C, N, R, S, stride, pad[0], pad[1], Ho, Wo)
        dw = dwk.permute(0, 3, 1, 2)
      else:
        with region('conv2d_wrw', nbytes):
          dw = _library_conv_backward(dy, x, w, stride, pad, 1)
    if ctx.needs_input_grad[0]:
      # backward-data = the same kernel with the roles of C and N swapped: its contraction runs over N in steps of 64
      mfma = N % 64 == 0 and C % 8 == 0 and igemm_limits_ok(dy.numel(), w.numel(), R * S)
      # strided backward-data by output-parity classes on the implicit-GEMM kernel (pf_conv2d_bwd_data_strided; MIOpen until round 4)
      by_classes = (OWN_CONV2D_BWD_STRIDED and stride > 1 and H % stride == 0 and W % stride == 0 and R >= stride and S >= stride
                    and dy.dtype == torch.bfloat16)
      if mfma and (stride == 1 or by_classes):
        wb = _bwd_data_weight(graph, ctx.w_var, w)                                        # [C][R][S][N], flipped
        dx = torch.empty_like(x)
        # the BN-backward sums of x's producer BN from this launch's epilogue (stride 1: bn2 of a block; by classes: bn2 in front of a
        # stage's strided 3x3, round 6)
        fuse = (FUSE_BN_BWD_STATS and bn_sums is not None and bn_sums.n_consumers == 1
                and bn_sums.act in ('Relu', 'Relu6') and bn_sums.x.shape == x.shape)
        with region('conv2d_bwd_data', float((dy.numel() + x.numel() * (2 if fuse else 1)) * 2)):
          bn = {}
          if fuse:
            G = (hip.conv2d_stats_groups(B * H * W, C, geom=(B, H, W, N, C, R, S, 1, R - 1 - pad[0], S - 1 - pad[1], H, W))
                 if stride == 1 else hip.conv2d_bwd_data_strided_stats_groups(B, H, W, C, stride))
            partial = bn_sums.sums_buffer(G, C, x.device)
            bn = dict(partial=partial, bn_x=bn_sums.x, bn_scale_shift=bn_sums.scale_shift, bn_mean_invstd=bn_sums.mean_invstd,
                      bn_act=bn_sums.act)
          if stride == 1:
            hip.conv2d_fwd(dy, wb, dx, B, H, W, N, C, R, S, 1, R - 1 - pad[0], S - 1 - pad[1], H, W, **bn)
          else:
            hip.conv2d_bwd_data_strided(dy, wb, dx, B, H, W, C, N, R, S, stride, pad[0], pad[1], Ho, Wo, **bn)
          if fuse:
            bn_sums.leave(partial, G, dx)
      elif OWN_CONV2D and OWN_CONV_GENERIC and x.is_cuda and dy.dtype == x.dtype and w.dtype == x.dtype:
        # geometries outside the MFMA kernels' limits (odd strided sizes, channel counts, 31-bit offsets): the general kernel
        dx = torch.empty_like(x)
        with region('conv2d_bwd_data', float((dy.numel() + x.numel()) * 2)):
          hip.convg_bwd_data(dy, _krsc(w, x.dtype), dx, B, H, W, C, N, R, S, stride, pad[0], pad[1], Ho, Wo,
                             slab=_convg_slab(graph, x.dtype, B * H * W, C, R * S * N))
      else:
        with region('conv2d_bwd_data', float((dy.numel() + x.numel()) * 2)):
          dx = _library_conv_backward(dy, x, w, stride, pad, 0)
    return dx, dw, None, None, None, None, None, None, None


class _ConvGeneric(torch.autograd.Function):
  """y = conv2d(x, W) [+ bias] on the general kernels of pf_convg.hip (any shape / stride, float32 or bf16 storage, float32
  accumulation): the float32 parity mode's convolutions and every bf16 layer the MFMA kernels do not take.  x: logical NCHW /
  physical NHWC, W: logical [N][C][R][S] / physical KRSC; pad = BEGIN pads (the end pads follow from Ho / Wo)."""

  @staticmethod
  def forward(ctx, x, w, bias, stride, pad, out_hw, graph):
    B, C, H, Wd = x.shape
    N, _, R, S = w.shape
    Ho, Wo = out_hw
    wk = _krsc(w, x.dtype)
    y = torch.empty((B, N, Ho, Wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    bf = None if bias is None else bias.detach().float().contiguous()
    with region('convg_fwd', float((x.numel() + y.numel()) * x.element_size())):
      # (split contraction of small outputs in bf16 only: the float32 parity mode keeps ONE ascending sum per output -- the conditioned
      # ResNet-50 gradient test moves from 1.7e-3 to 1.9e-2 on its most sensitive BN scale with the dense layer summed in 8 slabs)
      hip.convg_fwd(x, wk, bf, y, B, H, Wd, C, N, R, S, stride, pad[0], pad[1], Ho, Wo,
                    slab=_convg_slab(graph, x.dtype, B * Ho * Wo, N, R * S * C))
    ctx.save_for_backward(x, w)
    ctx.meta = (stride, pad, out_hw, graph, bias is not None)
    return y

  @staticmethod
  def backward(ctx, dy):
    x, w = ctx.saved_tensors
    stride, pad, (Ho, Wo), graph, has_bias = ctx.meta
    B, C, H, Wd = x.shape
    N, _, R, S = w.shape
    dy = _nhwc(dy)
    if dy.dtype != x.dtype:
      dy = dy.to(x.dtype)
    dx = dw = db = None
    if ctx.needs_input_grad[0]:
      wk = _krsc(w, x.dtype)
      dx = torch.empty_like(x, memory_format=torch.channels_last)
      with region('convg_bwd_data', float((dy.numel() + dx.numel()) * x.element_size())):
        hip.convg_bwd_data(dy, wk, dx, B, H, Wd, C, N, R, S, stride, pad[0], pad[1], Ho, Wo,
                           slab=_convg_slab(graph, x.dtype, B * H * Wd, C, R * S * N))
    if ctx.needs_input_grad[1]:
      splits = hip.convg_wrw_splits(B, C, N, R, S, Ho, Wo)
      dwk = torch.empty((N, R, S, C), dtype=w.dtype, device=x.device)
      with region('convg_wrw', float((dy.numel() + x.numel()) * x.element_size())):
        hip.convg_wrw(dy, x, dwk, graph.scratch(splits * N * R * S * C), B, H, Wd, C, N, R, S, stride, pad[0], pad[1], Ho, Wo)
      dw = dwk.permute(0, 3, 1, 2)
    if has_bias and ctx.needs_input_grad[2]:
      db = dy.float().sum(dim=(0, 2, 3))
    return dx, dw, db, None, None, None, None


def _convg_slab(graph, dtype, M: int, Nc: int, K: int):
  """Workspace of a k_convg forward / backward-data launch: EXACTLY what the shape's contraction split needs (hip.convg_small_splits --
  the kernel library decides from the shape alone, so a layer sums in the same order in step 1 and in step 1000, whatever other
  operators have grown the shared scratch to meanwhile); None in the float32 parity mode (one ascending sum per output) and for
  shapes that do not split."""
  if dtype != torch.bfloat16:
    return None
  splits = hip.convg_small_splits(M, Nc, K)
  return graph.scratch(splits * M * Nc) if splits > 0 else None


def convg_ok(x: torch.Tensor, w: torch.Tensor, dense: bool = False) -> bool:
  """float32: every convolution and dense layer.  bf16: the dense layer and convolutions over images (C % 8 != 0); a bf16
  convolution with 16 / 32 / 48 ... input channels (ResNet-20 @ CIFAR-10) is MFMA-shaped work that the vector-ALU kernel runs 2x
  slower per step than MIOpen (measured, configuration C1: 33 665 vs 66 174 images/s) -- it stays with the library until the
  implicit-GEMM kernel takes 16-channel k-steps (PF_CONVG_BF16_NARROW=1 forces ours)."""
  if not (OWN_CONV_GENERIC and isinstance(x, torch.Tensor) and x.is_cuda and x.dtype in (torch.float32, torch.bfloat16)
          and w.dtype in (torch.float32, torch.bfloat16) and x.numel() > 0):
    return False
  return (x.dtype == torch.float32 or dense or x.shape[1] % 8 != 0 or CONVG_BF16_NARROW
          or (x.dim() == 4 and x.shape[2] * x.shape[3] == 1))      # (a convolution over 1 x 1 pixels IS a dense layer: MobileNet's logits)


def conv_generic(x, w, bias, stride, pad_begin, out_hw, graph):
  """Dispatch helper: 4-D x (logical NCHW) through _ConvGeneric; works with or without autograd."""
  return _ConvGeneric.apply(_nhwc(x), w, bias, stride, pad_begin, out_hw, graph)


class _ConvIm2col(torch.autograd.Function):
  """y = conv2d(x, W) for few input channels (bf16, C % 8 == 0, C % 64 != 0: ResNet-20 @ CIFAR-10) as im2col + the in-tree 1x1 kernels
  (pf_im2col.hip): Y = Xcol W2d^T with W2d the [N][R*S*C] view of the KRSC kernel; backward: dXcol = dY W2d, dX = col2im(dXcol),
  dW2d = dY^T Xcol written straight into the flat gradient buffer.  Xcol is re-gathered in backward (9x the layer's input: not kept)."""

  @staticmethod
  def forward(ctx, x, w, stride, pad, out_hw, graph, w_var):
    B, C, H, Wd = x.shape
    N, _, R, S = w.shape
    Ho, Wo = out_hw
    M, K = B * Ho * Wo, R * S * C
    w2d = w.detach().permute(0, 2, 3, 1).reshape(N, K)
    xcol = torch.empty((M, K), dtype=x.dtype, device=x.device)
    y = torch.empty((B, N, Ho, Wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    with region('conv_im2col_fwd', float((x.numel() + 2 * xcol.numel() + y.numel()) * 2)):
      hip.im2col(x, xcol, B, H, Wd, C, R, S, stride, pad[0], pad[1], Ho, Wo)
      hip.conv1x1_fwd(xcol, w2d, y, M, N, K)
    ctx.save_for_backward(x, w)
    ctx.meta = (stride, pad, out_hw, graph, w_var)
    return y

  @staticmethod
  def backward(ctx, dy):
    x, w = ctx.saved_tensors
    stride, pad, (Ho, Wo), graph, w_var = ctx.meta
    B, C, H, Wd = x.shape
    N, _, R, S = w.shape
    M, K = B * Ho * Wo, R * S * C
    dy = _nhwc(dy)
    dx = dw = None
    w2d = w.detach().permute(0, 2, 3, 1).reshape(N, K)
    if ctx.needs_input_grad[1]:
      xcol = torch.empty((M, K), dtype=x.dtype, device=x.device)
      hip.im2col(x, xcol, B, H, Wd, C, R, S, stride, pad[0], pad[1], Ho, Wo)
      splits = hip.conv1x1_wrw_splits(M, N, K)

      def wrw(dwk, scratch):                     # dwk: [N][R][S][C] memory = [N][K]
        hip.conv1x1_wrw(dy, xcol, dwk.view(N, K), scratch((splits + 32) * N * K), M, N, K)
      dw = _filter_grad(graph, w, w_var, (dy, xcol), 'conv_im2col_wrw', float((M * K + M * N) * 2), wrw)
    if ctx.needs_input_grad[0]:
      dxcol = torch.empty((M, K), dtype=x.dtype, device=x.device)
      dx = torch.empty_like(x)
      with region('conv_im2col_bwd_data', float((dy.numel() + 2 * dxcol.numel() + dx.numel()) * 2)):
        hip.conv1x1_fwd(dy, w2d.t().contiguous(), dxcol, M, K, N)
        hip.col2im(dxcol, dx, B, H, Wd, C, R, S, stride, pad[0], pad[1], Ho, Wo)
    return dx, dw, None, None, None, None, None


def im2col_conv_ok(x, conv, pad) -> bool:
  """R x S convolutions the implicit-GEMM kernel does not take for their channel count (cin % 64 != 0) but the 1x1 kernels do."""
  kh, kw, cin, cout = conv.kernel.ref_shape
  return (OWN_CONV_IM2COL and conv.k > 1 and conv.bias is None and isinstance(x, torch.Tensor) and fusable_tensor(x) and x.dim() == 4
          and cin % 8 == 0 and cin % 64 != 0 and cout % 8 == 0 and conv.graph.fuse_conv1x1
          and x.shape[0] * x.shape[2] * x.shape[3] * kh * kw * cin < (1 << 31))


def _run_stem(x, w):
  """x: the image batch, logical NCHW / physical NHWC bf16; w: logical [64][3][7][7] over KRSC memory."""
  B, _, H, Wd = x.shape
  y = torch.empty((B, w.shape[0], H // 2, Wd // 2), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
  with region('conv_stem_fwd', float((x.numel() + y.numel()) * 2)):
    hip.conv_stem_fwd(x, w.detach().permute(0, 2, 3, 1), y, B, H, Wd)
  return y


class _StemConv(torch.autograd.Function):
  """The ResNet stem (7x7 / stride 2 / pad 3, 3 -> 64 channels) on pf_conv_stem_fwd / pf_conv_stem_wrw (the image needs
  no gradient; if it does, backward-data goes through MIOpen)."""

  @staticmethod
  def forward(ctx, x, w, graph, w_var):
    ctx.save_for_backward(x, w)
    ctx.meta = (graph, w_var)
    return _run_stem(x, w)

  @staticmethod
  def backward(ctx, dy):
    x, w = ctx.saved_tensors
    graph, w_var = ctx.meta
    dy = _nhwc(dy)
    dx = dw = None
    if ctx.needs_input_grad[1]:
      B, _, H, Wd = x.shape
      S = hip.conv_stem_wrw_slabs(B, H, Wd) if OWN_CONV2D_WRW else 0
      nbytes = float((x.numel() + dy.numel()) * 2)
      if S > 0:
        def wrw(dwk, scratch):
          hip.conv_stem_wrw(dy, x, dwk, scratch((S + 32) * 64 * 147), B, H, Wd)
        dw = _filter_grad(graph, w, w_var, (dy, x), 'conv_stem_wrw', nbytes, wrw)
      else:
        with region('conv_stem_wrw', nbytes):
          dw = _library_conv_backward(dy, x, w, 2, (3, 3), 1)
    if ctx.needs_input_grad[0]:
      dx = _library_conv_backward(dy, x, w, 2, (3, 3), 0)
    return dx, dw, None, None


def _run_stem3(x, w, pads, out_hw):
  """x: the image batch, logical NCHW / physical NHWC bf16; w: logical [N][3][3][3] over KRSC memory; pads: the FRONT pads."""
  B, _, H, Wd = x.shape
  N = w.shape[0]
  Ho, Wo = out_hw
  y = torch.empty((B, N, Ho, Wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
  with region('conv_stem_fwd', float((x.numel() + y.numel()) * 2)):
    hip.conv_stem3_fwd(x, w.detach().permute(0, 2, 3, 1), y, B, H, Wd, N, pads[0], pads[1], Ho, Wo)
  return y


class _Stem3Conv(torch.autograd.Function):
  """The MobileNet-v1 stem (3x3 / stride 2, 3 -> 16 | 32 channels, TensorFlow 'SAME' padding given by its FRONT pads) on
  pf_conv_stem3_fwd / pf_conv_stem3_wrw: no padded copy of the image (round 4 ran this layer on the general kernel over
  F.pad(image): 361 + 878 us per step against 148 / 119 us for MIOpen).  The image needs no gradient."""

  @staticmethod
  def forward(ctx, x, w, graph, w_var, pads, out_hw):
    ctx.save_for_backward(x, w)
    ctx.meta = (graph, w_var, pads, out_hw)
    return _run_stem3(x, w, pads, out_hw)

  @staticmethod
  def backward(ctx, dy):
    x, w = ctx.saved_tensors
    graph, w_var, pads, (Ho, Wo) = ctx.meta
    dy = _nhwc(dy)
    dw = None
    if ctx.needs_input_grad[1]:
      B, _, H, Wd = x.shape
      N = w.shape[0]
      S = hip.conv_stem3_wrw_slabs(B, H, Wd, N, pads[0], pads[1], Ho, Wo)
      if S <= 0:
        raise RuntimeError('pf_conv_stem3_wrw does not take the shape its forward kernel took')

      def wrw(dwk, scratch):
        hip.conv_stem3_wrw(dy, x, dwk, scratch((S + 32) * N * 27), B, H, Wd, N, pads[0], pads[1], Ho, Wo)
      dw = _filter_grad(graph, w, w_var, (dy, x), 'conv_stem_wrw', float((x.numel() + dy.numel()) * 2), wrw)
    if ctx.needs_input_grad[0]:
      raise RuntimeError('the MobileNet stem kernels compute no image gradient')
    return None, dw, None, None, None, None


def igemm_limits_ok(n_in_elems: int, n_kernel_elems: int, taps: int) -> bool:
  """Mirror of the argument checks of pf_conv2d_fwd (pf_igemm.hip): 31-bit byte offsets, 32-bit tap mask."""
  return n_in_elems < (1 << 30) and n_kernel_elems < (1 << 30) and taps <= 32


def fusable_tensor(t: torch.Tensor) -> bool:
  """pf_conv.hip works on bf16 device tensors (the float32 parity mode keeps every activation materialised)."""
  return t.is_cuda and t.dtype == torch.bfloat16


# =================================================================================================
# layers
# =================================================================================================

def _same_pads(size: int, k: int, stride: int) -> Tuple[int, int]:
  """TF 'SAME' padding: total = max((ceil(in/s)-1)*s + k - in, 0); extra pixel goes at the END."""
  out = -(-size // stride)
  total = max((out - 1) * stride + k - size, 0)
  return total // 2, total - total // 2


def _symmetric_pads(x: torch.Tensor, ph: Tuple[int, int], pw: Tuple[int, int]):
  """(x, (pad_h, pad_w)): the convolution kernels pad both ends of an axis alike, so (begin, end) pads that differ -- TF 'SAME' with
  an odd total -- become a zero-padded copy of `x` and no padding."""
  if ph[0] == ph[1] and pw[0] == pw[1]:
    return x, (ph[0], pw[0])
  return F.pad(x, (pw[0], pw[1], ph[0], ph[1])), (0, 0)


def variance_scaling_init(ref_shape, fan_in: int):
  """tf.variance_scaling_initializer() defaults (scale=1, fan_in, truncated normal); TF >= 1.9
  divides the stddev by .87962566103423978 to correct for the truncation (resnet_model.py:102)."""
  std = math.sqrt(1.0 / max(1.0, fan_in)) / .87962566103423978

  def init(rng: np.random.RandomState):
    from scipy.stats import truncnorm
    return truncnorm.rvs(-2, 2, size=ref_shape, random_state=rng).astype(np.float32) * np.float32(std)
  return init


def glorot_uniform_init(ref_shape, fan_in: int, fan_out: int):
  limit = math.sqrt(6.0 / (fan_in + fan_out))
  return lambda rng: rng.uniform(-limit, limit, size=ref_shape).astype(np.float32)


def truncated_normal_init(ref_shape, stddev: float):
  def init(rng: np.random.RandomState):
    from scipy.stats import truncnorm
    return truncnorm.rvs(-2, 2, size=ref_shape, random_state=rng).astype(np.float32) * np.float32(stddev)
  return init


def constant_init(ref_shape, value: float):
  return lambda rng: np.full(ref_shape, value, dtype=np.float32)


GATHER_MAX_CIN = 8192             # pf_conv_gather.hip keeps an int16 inverse channel map in LDS


def gather_pays(k: int, cin: int, kept: int, cout: int, dtype) -> bool:
  """Should a loader keep a shrunk k x k convolution with `kept` of `cin` input channels on pf_conv_gather.hip (True), or re-inflate
  it -- scatter the kept slices back into a zero kernel of full shape -- so that it runs on the dense inference kernels (False)?

  profiles/gather_conv_layers.txt (every ResNet-50 and MobileNet-v1 convolution shape at B = 256, bf16, 0.5 and 0.75 of the channels
  kept): the gather kernel loses on EVERY layer, dense / gather 0.17 - 0.46 (all convolutions of one ResNet-50 pass: 3.7 ms dense
  against 14.4 / 16.6 ms gathered; MobileNet 0.80 against 1.9 / 2.2 ms); the one row near 1 is MobileNet's 1 x 1-pixel logits layer
  (61 us either way).  float32 has not been timed.  So no layer class pays today and every shrunk layer is re-inflated: a shrunk
  file then runs exactly as fast as the full-shape checkpoint.  (inference.load_shrunk(reinflate='none') still runs the kernel.)"""
  return False


def int8_pays(k: int, cin: int, cout: int, stride: int, dtype) -> bool:
  """Should a loader send an eligible k x k convolution to pf_conv_i8_fwd (True) or leave it on the float kernels (False)?

  profiles/int8_conv_layers.txt (every eligible ResNet-50 convolution and every MobileNet-v1 pointwise convolution at B = 256 / 224 x
  224, bf16 output, the launches each route makes: fake-quant apply pass + bf16 kernel against codes pass + i8 kernel): the int8 route
  loses on every row but one, float / int8 0.40 - 0.99 (ResNet-50 summed: 6.3 ms against 9.9 ms; MobileNet 1.16 against 2.01 ms).  The
  codes pass is the cheaper producer (0.7 x the apply pass: it writes one byte per element), but the plain LDS-staged i8 kernel runs
  at 0.07 - 0.40 of its bound where the bf16 kernels with their LDS-DMA fills and double buffering reach 0.23 - 0.58.  The one row it
  wins is the 1 x 1, 256 -> 64 convolution at 56 x 56 (ResNet-50 stage 1 conv1: 314 against 289 us, 1.09), where the producer pass over
  the 256-channel input dominates both routes; with those two layers on int8 the whole ResNet-50 pass takes 8.106 against 8.154 ms
  (profiles/int8_inference_time.txt; every eligible layer on int8: 12.40 ms).  float32 output has not been timed.  (inference.load_int8(int8='on') still runs every
  eligible layer on the kernel.)"""
  return dtype == torch.bfloat16 and k == 1 and stride == 1 and cin == 256 and cout == 64


def int8_dw_pays(C: int, stride: int, dtype) -> bool:
  """Should a loader send an eligible depthwise 3x3 layer to pf_dw_i8_fwd (True) or leave it on pf_depthwise_fwd (False)?

  profiles/int8_depthwise_layers.txt (the 13 depthwise shapes of MobileNet-v1 1.0 at B = 256 / 224 x 224, bf16, the launches each route
  makes: fake-quant apply pass + pf_depthwise_fwd against codes pass + pf_dw_i8_fwd, three alternating rounds): the int8 route wins on
  EVERY row, float / int8 1.49 - 2.00 with spreads between rounds of at most 1.8 us on rows of 30 - 326 us (summed over one pass: 1.81
  against 1.09 ms).  Both halves gain: the codes pass writes one byte per element instead of two (0.7 x the apply pass) and the
  depthwise kernel reads one instead of two (0.36 - 0.75 x pf_depthwise_fwd).  Whole model (profiles/int8_mobilenet_inference_time.txt):
  with the pointwise layers on pf_conv_i8_fwd as well the pass takes 4.033 against 4.704 ms without this route.  True for exactly the
  measured (C, stride) pairs in bf16; float32 output and other widths have not been timed.  (inference.load_int8(depthwise='on') runs
  every eligible layer on the kernel.)"""
  return dtype == torch.bfloat16 and (C, stride) in _INT8_DW_PAYS


# (C, stride) of the rows of profiles/int8_depthwise_layers.txt on which the int8 route won by more than the spread: all of them
_INT8_DW_PAYS = frozenset([(32, 1), (64, 2), (128, 1), (128, 2), (256, 1), (256, 2), (512, 1), (512, 2), (1024, 1)])


def int8_pays_static(k: int, cin: int, cout: int, stride: int, dtype) -> bool:
  """`int8_pays` for a graph with FIXED activation ranges (inference.load_int8(act_ranges='static')): should a loader send an eligible
  Conv2D to the kernels on codes, where pf_conv_i8_fwd_q also applies the BatchNorm + activation + quantiser behind the layer?

  The STATIC table of profiles/int8_conv_layers.txt (tools/gpu/int8_conv_layers.py with STATIC=1: every eligible ResNet-50 convolution
  and every MobileNet-v1 pointwise convolution at B = 256 / 224 x 224, bf16, three alternating rounds; float = the bf16 kernel +
  pf_bn_act_quant_static writing the consumer's codes, int8 = pf_conv_i8_fwd_q, codes in and codes out): the route on codes loses on
  every row but one, float / int8 0.60 - 0.81 (ResNet-50 summed 5.22 against 7.37 ms, MobileNet 1.09 against 1.63 ms) -- the epilogue
  removed the static pass from the int8 side, but pf_conv_i8_fwd itself is the slower kernel.  It wins on the 256 -> 64 1x1 convolution
  at 56 x 56 (134.9 against 123.7 us, spreads 1.2 / 0.3 us), the row `int8_pays` accepts too.  Whole model
  (profiles/int8_static_inference_time.txt): ResNet-50 with that layer on codes 6.578 ms against 6.696 ms on the float kernels (both
  with static ranges), every eligible layer on codes 9.88 ms.  True for exactly that shape in bf16; float32 has not been timed."""
  return dtype == torch.bfloat16 and (k, cin, cout, stride) in _INT8_PAYS_STATIC


def int8_dw_pays_static(C: int, stride: int, dtype) -> bool:
  """`int8_dw_pays` for a graph with FIXED activation ranges: pf_dw_i8_fwd_q (codes in, the consumer's codes out) against
  pf_depthwise_fwd plus the static pass.

  The STATIC table of profiles/int8_depthwise_layers.txt (tools/gpu/int8_depthwise_layers.py with STATIC=1: the 13 depthwise shapes of
  MobileNet-v1 1.0 at B = 256 / 224 x 224, bf16, three alternating rounds; float = pf_depthwise_fwd + pf_bn_act_quant_static writing
  the consumer's codes, int8 = pf_dw_i8_fwd_q): the route on codes wins on EVERY row, float / int8 1.80 - 2.99 with spreads of at most
  4.0 us on rows of 15 - 228 us (summed over one pass 1.36 against 0.70 ms).  Whole model (profiles/int8_static_inference_time.txt):
  the 13 depthwise layers on codes and the pointwise layers on the bf16 kernels take 2.289 ms per batch against 2.877 ms with static
  ranges on the float kernels and 3.149 ms on the best per-batch route.  True for exactly the nine measured (C, stride) pairs in
  bf16; float32 and other widths have not been timed."""
  return dtype == torch.bfloat16 and (C, stride) in _INT8_DW_PAYS_STATIC


# (k, cin, cout, stride) / (C, stride) of the rows of the STATIC tables of profiles/int8_conv_layers.txt and
# profiles/int8_depthwise_layers.txt on which the route on codes won by more than the spread
_INT8_PAYS_STATIC = frozenset([(1, 256, 64, 1)])
_INT8_DW_PAYS_STATIC = frozenset([(32, 1), (64, 2), (128, 1), (128, 2), (256, 1), (256, 2), (512, 1), (512, 2), (1024, 1)])


def dw_lazy_pays(C: int, stride: int, quantised: bool, dtype) -> bool:
  """Should a depthwise 3x3 layer whose input is a LazyAct apply the producer's BN + activation (+ fake-quant) in its prologue
  (pf_depthwise_fwd_act / pf_depthwise_wrw_act: True) or have it materialised first (pf_bn_act_quant_apply + the plain kernels: False)?

  profiles/dw_lazy_layers.txt (tools/gpu/dw_lazy_layers.py: the ten depthwise shapes of MobileNet-v2 1.0 at B = 256 / 224 x 224, bf16,
  ReLU6, with and without an 8-bit quantiser, medians of three alternating rounds in one build): the fused launch LOSES on every row.
  Forward, no quantiser: apply + pf_depthwise_fwd over pf_depthwise_fwd_act 0.46 - 0.90 (the 0.90 is the 96-channel stride-2 layer at
  112 x 112: 430 against 476 us); backward-filter 0.52 - 0.97; with the quantiser 0.31 - 0.57.  One training step of a layer (the apply
  pass runs ONCE for both directions): 0.44 - 0.65 without, 0.25 - 0.39 with the quantiser; all 17 layers 3.22 against 6.47 ms and
  3.56 against 11.87 ms, spreads at most 2.8 us.  The parent kernels are not HBM-bound (0.2 - 0.6 of their byte bound): they are
  bound by issue and latency at two wavefronts per SIMD, and the prologue -- fmaf, clamp, the rounding to bf16 and the select, run
  once per output ROW that reads an element, three times at stride 1, plus two correctly rounded divisions with a quantiser -- costs
  more instructions than the multiply-adds it feeds and takes the kernels to one wavefront per SIMD (profiles/dw_lazy_registers.txt).
  So no row pays and every layer materialises by default; PF_DW_LAZY=1 runs the route (bit-identical results) for A/B runs.  float32
  has not been timed."""
  return dtype == torch.bfloat16 and (C, stride, bool(quantised)) in _DW_LAZY_PAYS


# (C, stride, quantised) of the rows of profiles/dw_lazy_layers.txt on which the fused pair of launches (forward + backward-filter) won
_DW_LAZY_PAYS = frozenset([])


def dw_lazy_on(C: int, stride: int, quantised: bool, dtype) -> bool:
  """The switch of the lazy depthwise route for one layer: PF_DW_LAZY forces it either way, otherwise the measured table decides."""
  return dw_lazy_pays(C, stride, quantised, dtype) if DW_LAZY is None else DW_LAZY


# What Conv2D._route / DepthwiseConv2D._route decide for one call, a plain tuple (it is built once per layer call):
#   (name, x, pad, out_hw, out_bn, geom)
# `name`: the route; the layer launches it in `_call_<name>`.  `x`: the prepared input -- materialised where the route reads a tensor,
# padded where its kernel pads both ends alike, never converted, so that it still carries the producer's tags.  `pad`: (pad_h, pad_w);
# for the routes that take 'SAME' padding by its FRONT pads, those.  `out_bn`: the BatchNormAct the launch applies in its epilogue
# (folded; on the int8 routes the requantising one).  `geom`: the int8 geometry.  What a route does not need is None.  The record
# lives for the call and references inputs, never an output.
ROUTE_NAME, ROUTE_X = 0, 1

# the Conv2D routes that count themselves on the producer's BnSums (the table stands at BnSums.add_consumer)
_CONV2D_COUNTED = frozenset(['conv1x1', 'igemm', 'im2col', 'general', 'library'])


@contextlib.contextmanager
def _plain_call(graph, fusion_off: bool = False):
  """A layer's plain() runs its __call__ with the taps off (and, for Conv2D, fusion off): the switches are put back behind it."""
  saved = graph.taps, graph.fuse_conv1x1
  graph.taps, graph.fuse_conv1x1 = None, graph.fuse_conv1x1 and not fusion_off
  try:
    yield
  finally:
    graph.taps, graph.fuse_conv1x1 = saved


class Conv2D:
  """tf.layers.conv2d / slim.conv2d: NHWC, kernel HWIO (stored KRSC), padding 'SAME' | 'VALID'."""

  def __init__(self, graph: Graph, name: str, cin: int, cout: int, k: int, stride: int = 1,
               padding: str = 'SAME', use_bias: bool = False, kernel_name: str = 'kernel',
               bias_name: str = 'bias', init=None, l2: bool = True):
    self.graph, self.k, self.stride, self.padding = graph, k, stride, padding
    ref_shape = (k, k, cin, cout)
    init = init or variance_scaling_init(ref_shape, k * k * cin)
    self.kernel = graph.store.add(name + '/' + kernel_name, ref_shape, 'conv', True, l2, init)
    self.bias = (graph.store.add(name + '/' + bias_name, (cout,), 'bias', True, l2, constant_init((cout,), 0.0))
                 if use_bias else None)
    self.op = graph.add_matmul_op('Conv2D', name + '/Conv2D', self.kernel)
    self.int8 = None                             # the packed layer on the device (inference.load_int8): dict of int8.pack_layer's tables
    graph.conv_layers.append(self)

  def __call__(self, x, residual: Optional[torch.Tensor] = None, want_stats: bool = False, out_bn=None) -> torch.Tensor:
    """`residual`: tensor added to the output (the block's shortcut); `want_stats`: the consumer is a
    BatchNormAct -- leave per-channel statistics of the output on the tensor (1x1 fused path only); `out_bn`: the ONLY
    consumer is that BatchNormAct in inference mode (`out_bn.folds_into_producer()`): the MFMA kernels apply it in their
    epilogue and tag the output, which the layer then passes through; any other route ignores the hint."""
    r = self._route(x, residual, out_bn)
    name = r[ROUTE_NAME]
    if name in _CONV2D_COUNTED:                  # the ONE place a Conv2D counts itself on its producer (BnSums.add_consumer)
      bn_sums = getattr(r[ROUTE_X], '_pf_bn', None)
      if bn_sums is not None:
        bn_sums.add_consumer(fuses=name == 'igemm' or (name == 'conv1x1' and isinstance(r[ROUTE_X], LazyAct)))
    return getattr(self, '_call_' + name)(r, residual, want_stats)

  def _route(self, x, residual, out_bn) -> tuple:
    """Which kernel family takes this call -- the ONE place that decides it -- and what its launch needs (the route record above).  The checks run
    in this order, and the order matters:
      (narrowing)  `requant` (a quantising consumer BN on a graph with fixed ranges: for the kernel on codes alone) and `out_bn` (dropped
                   with a residual, or where the BN does not fold) are settled before any route is asked.
      tap          before everything: the channel pruner records the layer whatever route it would take (_tapped, which re-enters
                   through plain() with taps and fusion off); a LazyAct is materialised for it.
      gathered     a physically shrunk layer (Graph.apply_gathers): inference on pf_conv_gather.hip.
      (int8)       a packed layer RAISES under gradients, whatever its input; then
      int8         a CodesAct whose codes pf_conv_i8_fwd takes (_int8_geometry); any other CodesAct is materialised here -- the
                   fake-quantised tensor of the apply pass, as without int8 -- and goes on down the list.
      conv1x1      1x1 on pf_conv.hip, the producer BN's normalise / act / fake-quant in the prologue: the only route that reads a
                   LazyAct, so it is asked before the input is materialised for all the others.
      stem3        the MobileNet stem, asked BEFORE _symmetric_pads: its kernel takes the asymmetric 'SAME' pads by their front pads
                   and must not see (or pay for) a padded copy of the image.  Asks about the image's gradient: it computes none.
      stem         the ResNet stem, asked AFTER it: its kernel pads both ends alike.
      igemm        RxS on the implicit-GEMM kernel (cin % 64 == 0).
      im2col       few-channel RxS as im2col + the 1x1 kernels (im2col_conv_ok).
      general      everything else our kernels take (convg_ok): pf_convg.hip.
      library      the rest.
    `out_bn` is honoured by the conv1x1 and igemm routes where they run without gradients and by the gathered route; every other
    route ignores it and the BatchNormAct runs its own pass."""
    g, w = self.graph, self.kernel.tensor
    requant = out_bn if (out_bn is not None and residual is None and out_bn.requantises()) else None
    if out_bn is not None and (residual is not None or not out_bn.folds_into_producer()):
      out_bn = None
    if g.taps is not None:
      return 'tap', materialize(x), None, None, None, None
    if self.kernel.gather_host is not None:
      return 'gathered', x, None, None, out_bn, None
    if self.int8 is not None and _wants_grad(w, x.x if isinstance(x, LazyAct) else x):
      raise RuntimeError('%s: a convolution packed for int8 runs in inference only: call it under torch.no_grad() on a graph '
                         'finalised with requires_grad=False' % self.kernel.name)
    if isinstance(x, CodesAct):
      geom = self._int8_geometry(x.x.shape, x.x.is_cuda) if self.int8 is not None else None
      if geom is not None:
        return 'int8', x, None, None, requant, geom
      x = x.materialize()
    kh, kw, cin, cout = self.kernel.ref_shape
    t = x.x if isinstance(x, LazyAct) else x
    if (self.k == 1 and self.bias is None and fusable_tensor(t) and t.dim() == 4 and cin % 8 == 0 and cout % 8 == 0
        and self.padding in ('SAME', 'VALID', 0) and g.fuse_conv1x1):
      return 'conv1x1', x, None, None, out_bn, None
    x = materialize(x)
    ph, pw, out_hw = self._geometry(x.shape)
    # what the stem and implicit-GEMM kernels ask alike: no bias, a 4-D bf16 device tensor, fusion on (a padded copy keeps all three)
    mfma = self.bias is None and isinstance(x, torch.Tensor) and fusable_tensor(x) and x.dim() == 4 and g.fuse_conv1x1
    if (mfma and OWN_STEM and self.padding == 'SAME' and residual is None and x.shape[1] == 3 and self.k == 3 and self.stride == 2
        and not x.requires_grad and x.is_contiguous(memory_format=torch.channels_last)
        and hip.conv_stem3_supported(x.shape[2], x.shape[3], 3, cout, 3, 2, ph[0], pw[0], out_hw[0], out_hw[1])
        and hip.conv_stem3_wrw_slabs(x.shape[0], x.shape[2], x.shape[3], cout, ph[0], pw[0], out_hw[0], out_hw[1]) > 0):
      return 'stem3', x, (ph[0], pw[0]), out_hw, None, None
    x, pad = _symmetric_pads(x, ph, pw)
    if (mfma and OWN_STEM and residual is None and pad[0] == pad[1] and x.is_contiguous(memory_format=torch.channels_last)
        and hip.conv_stem_supported(x.shape[2], x.shape[3], x.shape[1], cout, self.k, self.stride, pad[0])):
      return 'stem', x, pad, out_hw, None, None
    if (mfma and OWN_CONV2D and self.k > 1 and cin % 64 == 0 and cout % 8 == 0
        and igemm_limits_ok(x.numel(), kh * kw * cin * cout, kh * kw)):
      return 'igemm', x, pad, out_hw, out_bn, None
    if im2col_conv_ok(x, self, pad):
      return 'im2col', x, pad, out_hw, None, None
    return ('general' if convg_ok(x, w) else 'library'), x, pad, out_hw, None, None

  def _call_tap(self, r, residual, want_stats):
    return _tapped(self, r[ROUTE_X], residual)

  def _call_conv1x1(self, r, residual, want_stats):
    _, x, _, _, out_bn, _ = r
    w = self.kernel.tensor
    lazy = x if isinstance(x, LazyAct) else None
    xin = lazy.x if lazy is not None else _nhwc(x)
    if _wants_grad(w, xin):
      if lazy is not None and xin.requires_grad:
        lazy.n_grad_consumers += 1
        if self.stride == 1:
          lazy.dense_out = int(w.shape[0])
      return _apply_with_stats(_FusedConv1x1, xin, w, residual, lazy, want_stats, self.stride, self.graph, self.kernel)
    w2d = w.detach().permute(0, 2, 3, 1).reshape(w.shape[0], w.shape[1])
    return _run_conv1x1(xin, w2d, lazy, _nhwc(residual) if residual is not None else None, want_stats, self.stride, out_bn=out_bn)

  def _call_stem3(self, r, residual, want_stats):
    _, x, front_pads, out_hw, _, _ = r
    w = self.kernel.tensor
    if _wants_grad(w):                           # (the route was refused to an image that asks for a gradient)
      return _Stem3Conv.apply(x, w, self.graph, self.kernel, front_pads, out_hw)
    return _run_stem3(x, w, front_pads, out_hw)

  def _call_stem(self, r, residual, want_stats):
    x, w = r[ROUTE_X], self.kernel.tensor
    return _StemConv.apply(x, w, self.graph, self.kernel) if _wants_grad(w, x) else _run_stem(x, w)

  def _call_igemm(self, r, residual, want_stats):
    _, x, pad, _, out_bn, _ = r
    w, xin = self.kernel.tensor, _nhwc(x)
    if _wants_grad(w, xin):
      y = _apply_with_stats(_Conv2dIgemm, xin, w, self.stride, pad, want_stats, self.graph, getattr(x, '_pf_bn', None), self.kernel)
    else:
      y = _run_conv2d(xin, w.detach().permute(0, 2, 3, 1), self.stride, pad, want_stats, out_bn=out_bn)
    return y if residual is None else y + residual

  def _call_im2col(self, r, residual, want_stats):
    _, x, pad, out_hw, _, _ = r
    y = _ConvIm2col.apply(_nhwc(x), self.kernel.tensor, self.stride, pad, out_hw, self.graph, self.kernel)
    return y if residual is None else y + residual

  def _call_general(self, r, residual, want_stats):
    _, x, pad, out_hw, _, _ = r
    y = conv_generic(x, self.kernel.tensor, self.bias.tensor if self.bias is not None else None, self.stride, pad, out_hw, self.graph)
    return y if residual is None else y + residual

  def _call_library(self, r, residual, want_stats):
    _, x, pad, _, _, _ = r
    b = self.bias.tensor.to(x.dtype) if self.bias is not None else None
    y = F.conv2d(x, self.kernel.tensor, b, stride=self.stride, padding=pad)
    return y if residual is None else y + residual

  def _geometry(self, shape):
    """What `self.padding` means for an input of NCHW `shape`: ((top, bottom), (left, right), (Ho, Wo)).  An int pads every side by that much;
    TF 'SAME' puts the odd pixel at the END; 'VALID', 'SAME' with a 1x1 kernel and any other string pad nothing."""
    ph = pw = (0, 0)
    if isinstance(self.padding, int):
      ph = pw = (self.padding, self.padding)
    elif self.padding == 'SAME' and self.k > 1:
      ph = _same_pads(shape[2], self.k, self.stride)
      pw = _same_pads(shape[3], self.k, self.stride)
    return ph, pw, (_out_size(shape[2], self.k, self.stride, ph[0] + ph[1]),
                    _out_size(shape[3], self.k, self.stride, pw[0] + pw[1]))

  def _call_gathered(self, r, residual, want_stats) -> torch.Tensor:
    """The shrunk layer: reduction over the kept input channels only (hip.conv_gather_fwd), with the epilogues the dense inference
    kernels have (bias, residual, the consumer's folded inference-mode BN + activation).  Training a shrunk model is out of scope."""
    _, x, _, _, out_bn, _ = r
    var = self.kernel
    w = var.tensor
    x = materialize(x)
    if _wants_grad(w, x):
      raise RuntimeError('%s: a shrunk (channel-gathered) convolution runs in inference only: call it under torch.no_grad() '
                         'on a graph finalised with requires_grad=False' % var.name)
    if x.dim() != 4 or x.shape[1] != var.cin_full:
      raise ValueError('%s: input of shape %s, the layer has %d input channels' % (var.name, tuple(x.shape), var.cin_full))
    ph, pw, (Ho, Wo) = self._geometry(x.shape)
    x, pad = _symmetric_pads(x, ph, pw)
    x = _nhwc(x)
    B, C, H, Wd = x.shape
    N = w.shape[0]
    wk = _krsc(w, x.dtype)
    y = torch.empty((B, N, Ho, Wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    bias = None if self.bias is None else self.bias.tensor.detach().float().contiguous()
    res = None if residual is None else _nhwc(residual).to(x.dtype)
    ss = out_bn._eval_scale_shift(y) if out_bn is not None else None
    with region('conv_gather_fwd', float((x.numel() + y.numel() * (2 if res is not None else 1)) * x.element_size())):
      hip.conv_gather_fwd(x, wk, var.gather, y, B, H, Wd, C, N, self.k, self.k, self.stride, pad[0], pad[1], Ho, Wo,
                          bias=bias, residual=res, scale_shift=ss, act=out_bn.act if out_bn is not None else None)
    if out_bn is not None:
      y._pf_bn_done = out_bn
    return y

  def takes_codes(self, shape, is_cuda: bool) -> bool:
    """This layer will multiply the CODES of an input of this NCHW shape: it is packed, and no route ahead of the int8 kernel in
    __call__ (taps, a gather) takes the call."""
    return (self.int8 is not None and self.graph.taps is None and self.kernel.gather_host is None
            and self._int8_geometry(shape, is_cuda) is not None)

  def _int8_geometry(self, shape, is_cuda: bool):
    """(pad_h, pad_w, Ho, Wo) where pf_conv_i8_fwd takes this layer on an input of NCHW `shape`, else None: symmetric pads only (it has
    no padded copy to fall back on), no bias, a 4-D device tensor."""
    if self.bias is not None or len(shape) != 4 or not is_cuda or shape[1] != self.kernel.ref_shape[2]:
      return None
    ph, pw, (Ho, Wo) = self._geometry(shape)
    if ph[0] != ph[1] or pw[0] != pw[1]:
      return None
    return ph[0], pw[0], Ho, Wo

  def _call_int8(self, r, residual, want_stats) -> torch.Tensor:
    """The packed layer on the i8 matrix cores: the producer's codes (the record's `x`, a CodesAct) times the signed weights, scales and offsets in
    the epilogue (pocketflow_amd/int8.py states the formula), the residual added before the one rounding to the compute dtype.
    `requant` (the record's `out_bn`): the quantising BatchNormAct that alone consumes the output, on a graph with fixed ranges: applied in the epilogue
    (pf_conv_i8_fwd_q), the output being that layer's output -- codes where ITS consumer multiplies codes, the fake-quantised tensor
    otherwise.  `geom`: what _int8_geometry returned for the input."""
    _, x, _, _, requant, geom = r
    p, bits = self.int8, x.bits
    pad_h, pad_w, Ho, Wo = geom
    B, C, H, Wd = x.x.shape
    N = self.kernel.ref_shape[3]
    dims = (B, H, Wd, C, N, self.k, self.k, self.stride, pad_h, pad_w, Ho, Wo)
    return _run_on_codes(
        self, x, (B, N, Ho, Wo), 'conv_i8_fwd', requant, residual,
        lambda codes, ab, y, res: hip.conv_i8_fwd(codes, p['w'], ab, bits, p['scale_beta'], p['tsum'], p['tapsum'], y, *dims, residual=res),
        lambda codes, ab, ss, oab, out: hip.conv_i8_fwd_q(codes, p['w'], ab, bits, p['scale_beta'], p['tsum'], p['tapsum'], ss, requant.act, oab,
                                                          requant.op.bits, out, *dims))

  def plain(self, x: torch.Tensor) -> torch.Tensor:
    """The convolution alone on a materialised tensor (tracing / channel pruning)."""
    with _plain_call(self.graph, fusion_off=True):
      return self(x)


def _run_on_codes(layer, x: 'CodesAct', shape, name: str, requant, residual, launch, launch_q):
  """A packed layer on the codes of `x`, its output of NCHW `shape`: launch(codes, alpha_beta, y, residual) stores the output in the
  compute dtype; with `requant` (the BatchNormAct applied in the epilogue) launch_q(codes, alpha_beta, scale_shift, out_alpha_beta, out)
  stores that layer's output.  `name`: the region of the plain launch, name + '_q' that of the requantising one."""
  g, var = layer.graph, layer.kernel
  codes, ab = x.codes()
  if requant is not None:
    ss, oab, as_codes = requant.requant_plan(shape, codes.is_cuda)
    out = torch.empty(shape, dtype=torch.uint8 if as_codes else x.dtype, device=codes.device, memory_format=torch.channels_last)
    with region(name + '_q', float(codes.numel() + out.numel() * out.element_size())):
      launch_q(codes, ab, ss, oab, out)
    g.int8_ran.add(var.name)
    g.requant_ran.add(var.name)
    return requant.requant_result(out, ss, oab, x.dtype)
  y = torch.empty(shape, dtype=x.dtype, device=codes.device, memory_format=torch.channels_last)
  res = None if residual is None else _nhwc(residual).to(y.dtype)
  with region(name, float(codes.numel() + y.numel() * y.element_size() * (2 if res is not None else 1))):
    launch(codes, ab, y, res)
  g.int8_ran.add(var.name)
  return y


class TapStop(Exception):
  """Raised by the tap of `graph.tap_stop`: the caller only needed the network up to that layer."""


def _tapped(layer, x, residual=None):
  g = layer.graph
  y = layer.plain(x)
  y_add = None if residual is None else y + residual   # a residual sum has no single producer: tag dropped
  g.taps[layer] = (x, y, getattr(x, '_pf_src', None), y_add, residual)
  if g.tap_stop is layer:
    raise TapStop()
  y._pf_src = layer
  return y if residual is None else y_add


def _pass_tag(x, y):
  src = getattr(x, '_pf_src', None)
  if src is not None:
    y._pf_src = src
  return y


def _run_depthwise(x, w, stride, ph, pw, Ho, Wo, want_stats):
  """x: logical NCHW / physical NHWC, float32 or bf16; w: [C][1][k][k]; ph / pw: the FRONT pads."""
  B, C, H, W = x.shape
  k = w.shape[2]
  y = torch.empty((B, C, Ho, Wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
  partial = None
  if want_stats:
    G = hip.depthwise_groups(B, Ho, Wo, C)
    partial = torch.empty((G, 4, C), dtype=torch.float32, device=x.device)
  with region('depthwise_fwd', float((x.numel() + y.numel()) * x.element_size())):
    hip.depthwise_fwd(x, w.detach().reshape(C, k, k), y, B, H, W, C, k, stride, ph, pw, Ho, Wo, partial=partial)
  if want_stats:
    y._pf_stats = (partial, G)
  return y


class _Depthwise(torch.autograd.Function):
  """y = depthwise_conv3x3(x, W) on pf_depthwise_* (float32 or bf16 NHWC), TF 'SAME' front pads; the forward kernel leaves
  the statistics of y for the BatchNorm behind it (`want_stats`)."""

  @staticmethod
  def forward(ctx, x, w, stride, ph, pw, Ho, Wo, want_stats, graph, w_var, box):
    x = _nhwc(x)
    y = _run_depthwise(x, w, stride, ph, pw, Ho, Wo, want_stats)
    ctx.save_for_backward(x, w)
    ctx.meta = (stride, ph, pw, Ho, Wo, graph, w_var)
    box.append(getattr(y, '_pf_stats', None))
    return y

  @staticmethod
  def backward(ctx, dy):
    x, w = ctx.saved_tensors
    stride, ph, pw, Ho, Wo, graph, w_var = ctx.meta
    dy = _nhwc(dy)
    if dy.dtype != x.dtype:
      dy = dy.to(x.dtype)
    B, C, H, W = x.shape
    k = w.shape[2]
    dx = dw = None
    if ctx.needs_input_grad[1]:
      G = hip.depthwise_groups(B, Ho, Wo, C)

      def wrw(dwk, scratch):                       # dwk: [C][k][k][1] memory = [C][k][k]
        hip.depthwise_wrw(dy, x, dwk, scratch((G + 32) * C * k * k), B, H, W, C, k, stride, ph, pw, Ho, Wo)
      dw = _filter_grad(graph, w, w_var, (dy, x), 'depthwise_wrw', float((x.numel() + dy.numel()) * x.element_size()), wrw)
    if ctx.needs_input_grad[0]:
      dx = torch.empty_like(x)
      with region('depthwise_bwd_data', float((x.numel() + dy.numel()) * x.element_size())):
        hip.depthwise_bwd_data(dy, w.detach().reshape(C, k, k), dx, B, H, W, C, k, stride, ph, pw, Ho, Wo)
    return dx, dw, None, None, None, None, None, None, None, None, None


def _run_depthwise_act(x, lazy, w, stride, ph, pw, Ho, Wo, want_stats):
  """_run_depthwise on the un-materialised output of a BatchNormAct: x is the RAW tensor, the kernel applies `lazy` on the fly."""
  B, C, H, W = x.shape
  k = w.shape[2]
  y = torch.empty((B, C, Ho, Wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
  partial = None
  if want_stats:
    G = hip.depthwise_groups(B, Ho, Wo, C)
    partial = torch.empty((G, 4, C), dtype=torch.float32, device=x.device)
  quant = lazy.bits is not None
  with region('depthwise_fwd_act', float((x.numel() + y.numel()) * x.element_size())):
    hip.depthwise_fwd_act(x, lazy.scale_shift, lazy.act, lazy.slot if quant else None, lazy.bits if quant else 8,
                          w.detach().reshape(C, k, k), y, B, H, W, C, k, stride, ph, pw, Ho, Wo, partial=partial)
  if want_stats:
    y._pf_stats = (partial, G)
  return y


class _DepthwiseAct(torch.autograd.Function):
  """_Depthwise reading a LazyAct: y = depthwise_conv3x3(Q(x), W), Q the producer BN's normalise / act / fake-quant, applied in the
  prologue of pf_depthwise_fwd_act and again in pf_depthwise_wrw_act (the raw x and Q's operands are what is saved: the activated
  tensor never exists).  Backward-data never reads x: it is pf_depthwise_bwd_data as it stands, and its result is the gradient with
  respect to Q(x), which flows into x's node (_BnLazy) as it does from the fused 1x1 convolutions."""

  @staticmethod
  def forward(ctx, x, w, lazy, stride, ph, pw, Ho, Wo, want_stats, graph, w_var, box):
    y = _run_depthwise_act(x, lazy, w, stride, ph, pw, Ho, Wo, want_stats)
    ctx.save_for_backward(x, w)
    ctx.meta = (lazy, stride, ph, pw, Ho, Wo, graph, w_var)
    box.append(getattr(y, '_pf_stats', None))
    return y

  @staticmethod
  def backward(ctx, dy):
    x, w = ctx.saved_tensors
    lazy, stride, ph, pw, Ho, Wo, graph, w_var = ctx.meta
    dy = _nhwc(dy)
    if dy.dtype != x.dtype:
      dy = dy.to(x.dtype)
    B, C, H, W = x.shape
    k = w.shape[2]
    dx = dw = None
    if ctx.needs_input_grad[1]:
      G = hip.depthwise_groups(B, Ho, Wo, C)
      quant = lazy.bits is not None
      ss = lazy.scale_shift

      def wrw(dwk, scratch):                       # dwk: [C][k][k][1] memory = [C][k][k]
        hip.depthwise_wrw_act(dy, x, ss, lazy.act, lazy.slot if quant else None, lazy.bits if quant else 8, dwk,
                              scratch((G + 32) * C * k * k), B, H, W, C, k, stride, ph, pw, Ho, Wo)
      # (the producer BN's constants belong to ITS node, which runs right behind this one: kept referenced until the join)
      dw = _filter_grad(graph, w, w_var, (dy, x, ss, lazy), 'depthwise_wrw_act', float((x.numel() + dy.numel()) * x.element_size()), wrw)
    if ctx.needs_input_grad[0]:
      dx = torch.empty_like(x)
      with region('depthwise_bwd_data', float((x.numel() + dy.numel()) * x.element_size())):
        hip.depthwise_bwd_data(dy, w.detach().reshape(C, k, k), dx, B, H, W, C, k, stride, ph, pw, Ho, Wo)
    return (dx, dw) + (None,) * 10


class DepthwiseConv2D:
  """slim.separable_conv2d(num_outputs=None, depth_multiplier=1): DepthwiseConv2dNative."""

  def __init__(self, graph: Graph, name: str, channels: int, k: int, stride: int,
               kernel_name: str = 'depthwise_weights', init=None, l2: bool = True):
    self.graph, self.k, self.stride, self.channels = graph, k, stride, channels
    ref_shape = (k, k, channels, 1)
    init = init or truncated_normal_init(ref_shape, 0.09)
    self.kernel = graph.store.add(name + '/' + kernel_name, ref_shape, 'depthwise', True, l2, init)
    self.op = graph.add_matmul_op('DepthwiseConv2dNative', name + '/depthwise', self.kernel)
    self.int8 = None                             # the packed kernel on the device (inference.load_int8): tables of int8.pack_depthwise
    graph.depthwise_layers.append(self)

  def plain(self, x):
    with _plain_call(self.graph):
      return self(x)

  def takes_codes(self, shape, is_cuda: bool) -> bool:
    """This layer will multiply the CODES of an input of this NCHW shape: it is packed and no tap takes the call."""
    return self.int8 is not None and self.graph.taps is None and len(shape) == 4 and bool(is_cuda) and shape[1] == self.channels

  def _geometry(self, shape):
    """TF 'SAME' for an input of NCHW `shape`, as Conv2D._geometry: ((top, bottom), (left, right), (Ho, Wo)).  The kernels of this
    layer take the FRONT pads."""
    return (_same_pads(shape[2], self.k, self.stride), _same_pads(shape[3], self.k, self.stride),
            (-(-shape[2] // self.stride), -(-shape[3] // self.stride)))

  def __call__(self, x, want_stats: bool = False, out_bn=None) -> torch.Tensor:
    """`want_stats`: the consumer is a BatchNormAct -- leave the per-channel statistics of the output on the tensor.  `out_bn`: the
    ONLY consumer is that BatchNormAct; on a graph with fixed activation ranges the packed layer applies it in its epilogue
    (pf_dw_i8_fwd_q), any other route ignores the hint."""
    r = self._route(x, out_bn)
    name = r[ROUTE_NAME]
    if name in ('own', 'lazy'):                  # the ONE place a DepthwiseConv2D counts itself on its producer (BnSums.add_consumer)
      bn_sums = getattr(r[ROUTE_X], '_pf_bn', None)
      if bn_sums is not None:
        bn_sums.add_consumer(fuses=False)
    return getattr(self, '_call_' + name)(r, want_stats)

  def _route(self, x, out_bn) -> tuple:
    """As Conv2D._route, in this order: a packed layer that no tap takes RAISES under gradients, then `int8` for the CodesAct it takes
    (takes_codes; `out_bn` narrowed to a requantising one); every other input is materialised -- a CodesAct too: the fake-quantised
    tensor of the apply pass, as without int8 --; `tap`; `own` (pf_depthwise.hip); `library`.  In front of the materialisation:
    `lazy`, a LazyAct (never a CodesAct) this layer reads raw, with the producer's BN + activation + fake-quant in the prologue of
    pf_depthwise_fwd_act / pf_depthwise_wrw_act (takes_lazy: what `own` asks, no taps, the switch)."""
    g, w = self.graph, self.kernel.tensor
    if self.int8 is not None and g.taps is None:
      if _wants_grad(w, x.x if isinstance(x, LazyAct) else x):
        raise RuntimeError('%s: a depthwise convolution packed for int8 runs in inference only: call it under torch.no_grad() on a '
                           'graph finalised with requires_grad=False' % self.kernel.name)
      if isinstance(x, CodesAct) and self.takes_codes(x.x.shape, x.x.is_cuda):
        ph, pw, out_hw = self._geometry(x.x.shape)
        return 'int8', x, (ph[0], pw[0]), out_hw, (out_bn if (out_bn is not None and out_bn.requantises()) else None), None
    if (isinstance(x, LazyAct) and not isinstance(x, CodesAct) and x.act in DW_LAZY_ACTS
        and self.takes_lazy(x.x, x.bits is not None)):
      ph, pw, out_hw = self._geometry(x.x.shape)
      return 'lazy', x, (ph[0], pw[0]), out_hw, None, None
    x = materialize(x)
    if g.taps is not None:
      return 'tap', x, None, None, None, None
    ph, pw, out_hw = self._geometry(x.shape)
    if (OWN_DEPTHWISE and (x.is_cuda or DEPTHWISE_ANY_DEVICE) and x.dim() == 4 and x.dtype in (torch.float32, torch.bfloat16)
        and w.dtype == x.dtype and hip.depthwise_supported(self.channels, self.k, self.stride)):
      return 'own', x, (ph[0], pw[0]), out_hw, None, None
    x, pad = _symmetric_pads(x, ph, pw)
    return 'library', x, pad, None, None, None

  def _call_tap(self, r, want_stats):
    return _tapped(self, r[ROUTE_X])

  def _call_own(self, r, want_stats):
    _, x, (ph, pw), (Ho, Wo), _, _ = r
    w = self.kernel.tensor
    if _wants_grad(w, x):
      return _apply_with_stats(_Depthwise, x, w, self.stride, ph, pw, Ho, Wo, want_stats, self.graph, self.kernel)
    return _run_depthwise(_nhwc(x), w, self.stride, ph, pw, Ho, Wo, want_stats)

  def takes_lazy(self, t, quantised: bool) -> bool:
    """This layer will read the RAW tensor `t` behind a LazyAct and apply the producer itself: everything the `own` route asks, no
    tap, no packed kernel, a library (or test double) with the entry points, and the switch (dw_lazy_on)."""
    w = self.kernel.tensor
    return (OWN_DEPTHWISE and self.graph.taps is None and self.int8 is None and isinstance(t, torch.Tensor)
            and (t.is_cuda or DEPTHWISE_ANY_DEVICE) and t.dim() == 4 and t.dtype in (torch.float32, torch.bfloat16)
            and w.dtype == t.dtype and t.shape[1] == self.channels and hasattr(hip, 'depthwise_fwd_act')
            and hasattr(hip, 'depthwise_wrw_act') and hip.depthwise_supported(self.channels, self.k, self.stride)
            and dw_lazy_on(self.channels, self.stride, quantised, t.dtype))

  def _call_lazy(self, r, want_stats):
    _, lazy, (ph, pw), (Ho, Wo), _, _ = r
    w, x = self.kernel.tensor, lazy.x
    if _wants_grad(w, x):
      return _apply_with_stats(_DepthwiseAct, x, w, lazy, self.stride, ph, pw, Ho, Wo, want_stats, self.graph, self.kernel)
    return _run_depthwise_act(x, lazy, w, self.stride, ph, pw, Ho, Wo, want_stats)

  def _call_library(self, r, want_stats):
    _, x, pad, _, _, _ = r
    return F.conv2d(x, self.kernel.tensor, None, stride=self.stride, padding=pad, groups=self.channels)

  def _call_int8(self, r, want_stats) -> torch.Tensor:
    """The packed layer on pf_dw_i8_fwd: the producer's codes (the record's `x`, a CodesAct) times the kernel's codes in integers, scales and
    offsets in the epilogue (pocketflow_amd/int8.py states the formula), one rounding to the compute dtype.  The BatchNorm behind it
    makes its own statistics pass (the output carries none).  `requant`: as in Conv2D._call_int8 (pf_dw_i8_fwd_q)."""
    _, x, (ph, pw), (Ho, Wo), requant, _ = r
    p, bits = self.int8, x.bits
    B, C, H, Wd = x.x.shape
    dims = (B, H, Wd, C, self.stride, ph, pw, Ho, Wo)
    return _run_on_codes(
        self, x, (B, C, Ho, Wo), 'dw_i8_fwd', requant, None,
        lambda codes, ab, y, res: hip.dw_i8_fwd(codes, p['wcol'], p['scale_beta'], ab, bits, y, *dims),
        lambda codes, ab, ss, oab, out: hip.dw_i8_fwd_q(codes, p['wcol'], p['scale_beta'], ab, bits, ss, requant.act, oab, requant.op.bits, out,
                                                        *dims))


class Dense:
  """tf.layers.dense: kernel [in, out] (stored [out, in]) + bias."""

  def __init__(self, graph: Graph, name: str, cin: int, cout: int, init=None, l2: bool = True):
    self.graph = graph
    ref_shape = (cin, cout)
    init = init or glorot_uniform_init(ref_shape, cin, cout)
    self.kernel = graph.store.add(name + '/kernel', ref_shape, 'dense', True, l2, init)
    self.bias = graph.store.add(name + '/bias', (cout,), 'bias', True, l2, constant_init((cout,), 0.0))
    self.op = graph.add_matmul_op('MatMul', name + '/MatMul', self.kernel)

  def __call__(self, x) -> torch.Tensor:
    g = self.graph
    x = materialize(x)
    if g.taps is not None and g.tap_dense:
      y = self.plain(x)
      g.taps[self] = (x, y, None)
      if g.tap_stop is self:
        raise TapStop()
      return y + self.bias.tensor.to(x.dtype)
    return self._matmul(x, self.bias.tensor)

  def plain(self, x: torch.Tensor) -> torch.Tensor:
    """The MatMul op alone (no BiasAdd)."""
    return self._matmul(x, None)

  def _matmul(self, x, bias):
    """x W^T [+ bias]: tf.layers.dense = the 1x1 convolution of a [B][1][1][in] tensor (+ BiasAdd in the epilogue) on pf_convg.hip,
    the library for what that kernel does not take."""
    w = self.kernel.tensor
    if x.dim() == 2 and convg_ok(x, w, dense=True):
      y = _ConvGeneric.apply(x.contiguous().view(x.shape[0], x.shape[1], 1, 1), w.view(w.shape[0], w.shape[1], 1, 1), bias, 1,
                             (0, 0), (1, 1), self.graph)
      return y.view(x.shape[0], -1)
    return F.linear(x, w, bias.to(x.dtype) if bias is not None else None)


class Activation:
  """A stand-alone Relu / Relu6 op (followed by activation fake-quant when the learner asks)."""

  def __init__(self, graph: Graph, name: str, act: str = 'Relu'):
    self.graph, self.act = graph, act
    self.op = graph.add_activation_op(act, name)

  def __call__(self, x: torch.Tensor) -> torch.Tensor:
    g = self.graph
    if self.op.bits is None:
      y = F.relu(x) if self.act == 'Relu' else F.relu6(x)
      return _pass_tag(x, y) if g.taps is not None else y
    if g.act_static is not None and not torch.is_grad_enabled():
      # fixed range: the clamping pass with scale 1 / shift 0 over [rows][C] of any rank (a Dense output is [B][C]); the slot is
      # not touched
      x = _nhwc(x)
      C = x.shape[1] if x.dim() > 1 else x.numel()
      y = torch.empty_like(x)
      hip.bn_act_quant_static(x, y, x.numel() // C, C, g.identity_scale_shift(C), self.act, g.act_static[self.op.index], self.op.bits)
      return y
    return _ActQuant.apply(x, self.act, g.act_slots[self.op.index], self.op.bits)


class BatchNormAct:
  """tf.layers.batch_normalization(fused) [+ Relu / Relu6 right behind it], one fused op chain.

  ResNet-v2 and MobileNet-v1 only ever use BN followed by an activation, which is what lets the
  BN statistics pass also deliver the activation's whole-tensor min/max (pf_bn_finalize).
  """

  def __init__(self, graph: Graph, name: str, channels: int, act: Optional[str], momentum: float, eps: float,
               l2: bool = False, act_name: Optional[str] = None, names=('gamma', 'beta', 'moving_mean',
                                                                       'moving_variance'), lazy_ok: bool = False,
               codes_ok: Optional[bool] = None, beta_first: bool = False):
    self.graph, self.act, self.momentum, self.eps, self.C = graph, act, momentum, eps, channels
    self.lazy_ok = lazy_ok                    # every consumer is a Conv2D: the output may stay un-materialised
    # every consumer is a Conv2D or a DepthwiseConv2D, for the int8 inference route alone (CodesAct): also set where the training path
    # keeps the output materialised (a BN in front of a 3x3 or a depthwise convolution)
    self.codes_ok = lazy_ok if codes_ok is None else codes_ok
    st = graph.store
    if beta_first:                            # slim.batch_norm creates beta in front of gamma (creation order = checkpoint order)
      self.beta = st.add(name + '/' + names[1], (channels,), 'bn_beta', True, l2, constant_init((channels,), 0.0))
    self.gamma = st.add(name + '/' + names[0], (channels,), 'bn_gamma', True, l2, constant_init((channels,), 1.0))
    self.beta = st.add(name + '/' + names[1], (channels,), 'bn_beta', True, l2, constant_init((channels,), 0.0))
    self.moving_mean = st.add(name + '/' + names[2], (channels,), 'bn_mean', False, False,
                              constant_init((channels,), 0.0))
    self.moving_var = st.add(name + '/' + names[3], (channels,), 'bn_var', False, False,
                             constant_init((channels,), 1.0))
    self.op = graph.add_activation_op(act, act_name or (name + '/' + act)) if act else None
    self._frozen_ss = None
    # the ONE layer that reads this layer's output, where the network code names it (None: not named, or more than one): a packed
    # producer that requantises for this layer writes codes exactly when that consumer multiplies codes
    self.consumer = None

  def _mode(self, *tensors, op=None):
    """(mode, bits, slot) of a call of this layer -- the ONE place that decides it.  BN_TRAIN: training, batch statistics.
    BN_EVAL_GRAD: inference mode WITH gradients (moving statistics; gamma / beta and everything upstream still trained): gradients
    are enabled, the graph is not frozen, and the layer's gamma or one of `tensors` (the call's inputs) requires them.  BN_EVAL:
    inference without gradients.  A caller WITHOUT a tensor (_static, folds_into_producer: they decide before the input exists) gets
    the conservative answer: gradients enabled on a graph that is not frozen counts as "may need gradients", whatever requires_grad
    will say.  `bits` / `slot`: the quantiser of the activation `op` behind the BN (default: the layer's own) for a call with
    tensors, None without one."""
    g = self.graph
    bits = slot = None
    if tensors:                                   # (a caller without a tensor launches nothing: it gets no quantiser either)
      op = op if op is not None else self.op
      bits = op.bits if op is not None else None
      slot = g.act_slots[op.index] if bits is not None else None
    grad = torch.is_grad_enabled()
    if g.training and grad:
      return BN_TRAIN, bits, slot
    if not grad or g.frozen:
      return BN_EVAL, bits, slot
    if tensors:
      if not (self.gamma.tensor.requires_grad or any(t.requires_grad for t in tensors)):
        return BN_EVAL, bits, slot
      if bits is not None:
        raise NotImplementedError('inference-mode BN with gradients and activation quantisation (no learner needs it)')
    return BN_EVAL_GRAD, None, None

  def _feeds_lazy_depthwise(self, x) -> bool:
    """The ONE consumer the network code named is a depthwise layer that will read this layer's raw input and apply the layer itself
    (DepthwiseConv2D.takes_lazy): the output may stay un-materialised in float32 too, where no 1x1 kernel has a prologue."""
    c = self.consumer
    return (isinstance(c, DepthwiseConv2D) and x.dim() == 4 and self.act in DW_LAZY_ACTS
            and c.takes_lazy(x, self.op is not None and self.op.bits is not None))

  def _static(self) -> bool:
    """Inference on a graph with fixed activation ranges, this layer quantising: the clamping kernels, no statistics pass."""
    g = self.graph
    return (g.act_static is not None and self.op is not None and self.op.bits is not None and g.taps is None
            and self._mode()[0] == BN_EVAL)

  def requantises(self) -> bool:
    """A packed producer may apply this layer in its epilogue: fixed ranges, at most 8 bits, no gradients."""
    return self._static() and self.op.bits <= 8 and not torch.is_grad_enabled()

  def requant_plan(self, shape, is_cuda: bool):
    """(scale_shift, alpha_beta row, write codes?) for a producer that applies this layer to an output of NCHW `shape`."""
    ss = self._inference_scale_shift(self.gamma.tensor, None)      # a fixed range: no slot
    as_codes = bool(self.graph.int8 and self.codes_ok and self.consumer is not None and self.consumer.takes_codes(shape, is_cuda))
    return ss, self.graph.act_static[self.op.index], as_codes

  def requant_result(self, out, ss, oab, dtype):
    """What the producer returns: this layer's output, marked as already applied (__call__ passes it through)."""
    if out.dtype == torch.uint8:
      C = self.C
      out = StaticCodesAct(None, ss, self.act, oab, self.op.bits, out.numel() // C, C, codes=out, dtype=dtype)
    out._pf_bn_done = self
    return out

  def folds_into_producer(self) -> bool:
    """This layer, in inference mode and without a quantiser (the distillation teacher's forward_eval; evaluation of a
    full-precision network), can be applied in the epilogue of the convolution that feeds it: y -> act(scale * y + shift) on the
    stored bf16 value, bit for bit pf_bn_act_quant_apply (PF_FOLD_EVAL_BN=0: off, A/B runs)."""
    g = self.graph
    if not FOLD_EVAL_BN or g.taps is not None or not g.fuse_conv1x1:
      return False
    if self._mode()[0] != BN_EVAL:
      return False                                # training; inference-mode BN WITH gradients: its input must exist
    return self.op is None or self.op.bits is None

  def __call__(self, x: torch.Tensor, with_skip: bool = False):
    """`with_skip`: also return x for the block's identity shortcut (see _BnLazy)."""
    g = self.graph
    skip = x
    if getattr(x, '_pf_bn_done', None) is self:   # applied in the epilogue of the producing convolution (Conv2D `out_bn`)
      y = x
    else:
      mode, bits, slot = self._mode(x)
      lazy = self.lazy_ok and isinstance(x, torch.Tensor) and ((g.fuse_conv1x1 and fusable_tensor(x)) or self._feeds_lazy_depthwise(x))
      if mode == BN_TRAIN:
        stats = getattr(x, '_pf_stats', None)    # left by the fused convolution that produced x
        rec = BnSums()                           # lets a single consuming convolution fuse the BN-backward sums
        if lazy:
          alias, skip = _BnLazy.apply(_nhwc(x), self.gamma.tensor, self.beta.tensor, self, g, slot, rec, stats)
          y = LazyAct(alias, rec.scale_shift, self.act, slot, bits, x.numel() // self.C, self.C, bn=rec)
        else:
          y = _BnActQuant.apply(x, self.gamma.tensor, self.beta.tensor, self, g, True, slot, bits, stats, rec)
          y._pf_bn = rec
      elif mode == BN_EVAL_GRAD:
        y = _BnActQuant.apply(materialize(x), self.gamma.tensor, self.beta.tensor, self, g, False, None, None)
      else:
        y = self._inference(_nhwc(x), slot, bits, lazy)
    if g.taps is not None and isinstance(y, torch.Tensor):
      y = _pass_tag(x, y)
    return (y, skip) if with_skip else y

  def pooled(self, x: torch.Tensor):
    """mean over H, W of this layer's output as [B][C], in the fused head launches (_BnActPool; the activated map is never written)
    -- or None where the caller has to take the separate chain: PF_HEAD_FUSE=0, taps, no GPU tensor, a library without the
    entry points, a layer already applied in the producing convolution's epilogue."""
    g = self.graph
    if not head_fuse_ok(g, x) or x.dim() != 4 or getattr(x, '_pf_bn_done', None) is self:
      return None
    if self._static():
      return None                                 # pf_bn_act_quant_pool has no clamp: the separate chain through the static pass
    mode, bits, slot = self._mode(x)
    if mode != BN_EVAL:
      return _BnActPool.apply(x, self.gamma.tensor, self.beta.tensor, self, g, mode == BN_TRAIN, slot, bits,
                              getattr(x, '_pf_stats', None) if mode == BN_TRAIN else None)
    x = _nhwc(x)
    rows = x.numel() // self.C
    pooled = torch.empty((x.shape[0], self.C), dtype=x.dtype, device=x.device)
    hip.bn_act_quant_pool(x, pooled, rows, self.C, rows // x.shape[0], self._inference_scale_shift(x, slot), self.act, slot,
                          bits if bits is not None else 8, bits is not None)
    return pooled

  def _inference(self, x, slot, bits, lazy):
    """Inference mode without gradients, x in NHWC memory: lazy?  codes?  a fixed range or the batch's?  Then one launch."""
    C = self.C
    rows = x.numel() // C
    static = bits is not None and self._static()
    ss = self._inference_scale_shift(x, None if static else slot)
    if bits is None and lazy:
      return LazyAct(x, ss, self.act, None, None, rows, C)
    if bits is not None and bits <= 8 and self.graph.int8 and self.codes_ok and x.is_cuda and x.dim() == 4:
      # this layer hands out codes: every consumer may multiply them, and the one that does not materialises
      if static:
        return StaticCodesAct(x, ss, self.act, self.graph.act_static[self.op.index], bits, rows, C)
      return CodesAct(x, ss, self.act, slot, bits, rows, C)
    q = torch.empty_like(x)
    if static:
      hip.bn_act_quant_static(x, q, rows, C, ss, self.act, self.graph.act_static[self.op.index], bits)
    else:
      hip.bn_act_quant_apply(x, q, rows, C, ss, self.act, slot, bits if bits is not None else 8, bits is not None)
    return q

  def _inference_scale_shift(self, x, slot):
    """scale / shift for inference without gradients.  No `slot` (a layer without a quantiser, or one with a fixed range): the
    moving statistics folded, the teacher's (frozen) pair cached.  With one: the calibrating statistics pass."""
    return self._eval_scale_shift(x) if slot is None else self._calibrated_scale_shift(x, slot)

  def _calibrated_scale_shift(self, x, slot):
    """scale / shift of the eval graph of a quantising learner: the moving statistics, plus one statistics pass over x whose
    finalize leaves the freshly calibrated activation range in `slot`."""
    g, C = self.graph, self.C
    rows = x.numel() // C
    with torch.no_grad():
      partial, nblk, _ = _bn_statistics(x, rows, C, g)
      ss = torch.empty((2, C), dtype=torch.float32, device=x.device)
      mi = torch.empty((2, C), dtype=torch.float32, device=x.device)
      hip.bn_finalize(partial, nblk, rows, C, x, self.gamma.tensor, self.beta.tensor, self.moving_mean.tensor,
                      self.moving_var.tensor, self.momentum, self.eps, g.training, self.act, ss, mi, slot)
    return ss

  def _eval_scale_shift(self, x):
    """Inference BN folded to scale/shift; the teacher's (frozen) pair is cached."""
    g = self.graph
    if g.frozen and self._frozen_ss is not None:
      return self._frozen_ss
    ss = torch.empty((2, self.C), dtype=torch.float32, device=x.device)
    hip.bn_eval_scale_shift(self.gamma.tensor, self.beta.tensor, self.moving_mean.tensor, self.moving_var.tensor,
                            self.eps, ss)
    if g.frozen:
      self._frozen_ss = ss
    return ss


class BatchNormAddAct:
  """The tail of a ResNet-v1 block, `act(batch_norm(x) + shortcut)` (utils/external/resnet_model.py:250-252), as one layer: the
  variables and moving averages are those of a BatchNormAct without activation (`self.bn`), the activation op is registered like a
  free-standing Activation's (one more quantised activation for the learners), and on the GPU the three steps and the quantiser's
  range run as one pass (_BnAddActQuant).  Anything the kernels do not take -- no GPU tensor, a dtype other than float32 / bf16,
  C % 8 != 0 -- runs the composition of the v1 basic block: BatchNormAct, torch add, Activation.
  Not covered by the int8 / fixed-range loaders: such a graph is refused with a ValueError that names this layer."""

  def __init__(self, graph: Graph, name: str, channels: int, act: Optional[str], momentum: float, eps: float,
               act_name: Optional[str] = None, l2: bool = False, names=('gamma', 'beta', 'moving_mean', 'moving_variance'),
               beta_first: bool = False):
    if act not in ('Relu', None):
      raise ValueError('%s: the join kernels apply Relu (or nothing), not %s' % (name, act))
    self.graph, self.name, self.act, self.C = graph, name, act, channels
    self.bn = BatchNormAct(graph, name, channels, None, momentum, eps, l2=l2, names=names, beta_first=beta_first)
    # `act` None (the linear bottleneck of MobileNet-v2): no activation op, hence no slot and no quantiser behind the sum
    self.relu = Activation(graph, act_name, act) if act is not None else None   # registers the op; also the activation of the composition
    self.op = self.relu.op if self.relu is not None else None
    graph.join_layers.append(self)

  def refusal(self) -> str:
    return ('%s/%s: the BN + shortcut + %s joins of the ResNet-v1 blocks are not covered by the int8 / static-range loaders'
            % (self.graph.scope, self.name, self.act) if self.act is not None else
            '%s/%s: the BN + shortcut joins of the MobileNet-v2 blocks are not covered by the int8 / static-range loaders'
            % (self.graph.scope, self.name))

  def takes(self, x, shortcut) -> bool:
    return (bn_join_tensor_ok(x) and isinstance(shortcut, torch.Tensor) and shortcut.dtype == x.dtype
            and shortcut.shape == x.shape and shortcut.device == x.device)

  def __call__(self, x, shortcut) -> torch.Tensor:
    g = self.graph
    if g.act_static is not None or g.int8:
      raise ValueError(self.refusal())
    x, shortcut = materialize(x), materialize(shortcut)
    if not self.takes(x, shortcut):
      y = self.bn(x) + shortcut
      return self.relu(y) if self.relu is not None else y
    mode, bits, slot = self.bn._mode(x, shortcut, op=self.op)
    if mode != BN_EVAL:
      u, skip = _BnAddActQuant.apply(x, shortcut, self.bn.gamma.tensor, self.bn.beta.tensor, self, g, mode == BN_TRAIN, slot, bits,
                                     getattr(x, '_pf_stats', None) if mode == BN_TRAIN else None)
      u._pf_skip = skip                            # for the second consumer of the block output (see _BnAddActQuant)
      return u
    # inference mode without gradients: the moving statistics folded to scale / shift (the BN itself has no quantiser), the same pass
    x, r = _nhwc(x), _nhwc(shortcut)
    rows = x.numel() // self.C
    u = torch.empty_like(x)
    if bits is not None:
      hip.minmax_slots_init(slot)
    hip.bn_add_act_fwd(x, r, u, rows, self.C, self.bn._inference_scale_shift(x, None), self.act, slot)
    if bits is not None:
      hip.uq_apply(u, u, slot, bits, None)
    return u


class _MaxPool(torch.autograd.Function):
  """Max-pooling on pf_maxpool_fwd / pf_maxpool_bwd (NHWC, clipped windows = -inf padding, first-maximum gradient)."""

  @staticmethod
  def forward(ctx, x, k, stride, ph, pw):
    need_grad = ctx.needs_input_grad[0]          # of the ARGUMENT: a channels_last copy made in here never requires grad
    x = _nhwc(x)
    B, C, H, W = x.shape
    Ho, Wo = _out_size(H, k, stride, ph[0] + ph[1]), _out_size(W, k, stride, pw[0] + pw[1])
    y = torch.empty((B, C, Ho, Wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    idx = torch.empty((B, Ho, Wo, C), dtype=torch.uint8, device=x.device) if need_grad else None
    with region('maxpool_fwd', float((x.numel() + y.numel()) * x.element_size())):
      hip.maxpool_fwd(x, y, idx, B, H, W, C, k, stride, ph[0], pw[0], Ho, Wo)
    ctx.meta = (k, stride, ph[0], pw[0], x.shape)
    if need_grad:
      ctx.save_for_backward(idx)
    return y

  @staticmethod
  def backward(ctx, dy):
    (idx,) = ctx.saved_tensors
    k, stride, ph0, pw0, xshape = ctx.meta
    dy = _nhwc(dy)
    B, C, H, W = xshape
    dx = torch.empty(xshape, dtype=dy.dtype, device=dy.device, memory_format=torch.channels_last)
    with region('maxpool_bwd', float((dx.numel() + dy.numel()) * dy.element_size())):
      hip.maxpool_bwd(dy, idx, dx, B, H, W, C, k, stride, ph0, pw0, dy.shape[2], dy.shape[3])
    return dx, None, None, None, None


def max_pool_same(x: torch.Tensor, k: int, stride: int) -> torch.Tensor:
  """tf.layers.max_pooling2d(padding='SAME'): pad with -inf, extra pixel at the end."""
  ph = _same_pads(x.shape[2], k, stride)
  pw = _same_pads(x.shape[3], k, stride)
  if x.is_cuda and x.dim() == 4 and x.shape[1] % 8 == 0 and x.dtype in (torch.float32, torch.bfloat16) and OWN_POOL:
    return _MaxPool.apply(x, k, stride, ph, pw)
  if ph[0] == 0 and pw[0] == 0:
    # padding only at the end: identical to a ceil-mode pool (clipped last window), no padded copy
    return F.max_pool2d(x, k, stride, ceil_mode=True)
  if any(ph) or any(pw):
    x = F.pad(x, (pw[0], pw[1], ph[0], ph[1]), value=float('-inf'))
  return F.max_pool2d(x, k, stride)


def fixed_padding(x: torch.Tensor, k: int) -> torch.Tensor:
  """resnet_model.fixed_padding (utils/external/resnet_model.py:65-89)."""
  pad_total = k - 1
  pb = pad_total // 2
  pe = pad_total - pb
  if pad_total == 0:
    return x
  return F.pad(x, (pb, pe, pb, pe))


def to_device_images(images, graph: Graph) -> torch.Tensor:
  """NHWC float32 batch (reference tensor contract) -> logical NCHW / physical NHWC compute tensor."""
  if isinstance(images, np.ndarray):
    images = torch.from_numpy(images)
  x = images.to(graph.device, non_blocking=True)
  if x.dim() == 4:
    x = x.permute(0, 3, 1, 2)                  # view: logical NCHW over NHWC memory (channels_last)
  return x.to(graph.compute_dtype)
