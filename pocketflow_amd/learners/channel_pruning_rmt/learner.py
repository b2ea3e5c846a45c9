"""Channel pruning, remastered (reference learners/channel_pruning_rmt/learner.py), with channel selection on the device.

Every Conv2D layer of the network, in graph order, goes through three steps (reference __choose_channels :546-649):

  sampling  both networks run forward_train (batch-statistics BN, no BN update) on the cached mini-batches; per mini-batch and crop
            one output position is drawn, the pruned network's input patch and the full network's output vector there are gathered
            (pf_cpr_gather; __smpl_inputs_n_outputs :651-725), until more than cpr_nb_crops_per_smpl * cpr_nb_smpls rows exist; then
            np.random.choice keeps exactly that many;
  LASSO     on a secondary sample of the rows, X^T X and X^T y in float64 normalised by ||X^T X||_F (pf_cpr_gram), and a bisection on
            gamma over ISTA solves from one random initial mask (pf_cpr_ista; __solve_sparse_regression :727-813, meta LASSO :432-468);
  lstsq     cpr_lstsq_nb_iters Adam steps on the kept channels' least-squares fit to the full network's outputs (pf_cpr_lstsq_step;
            meta least squares :470-523, :815-841); the kernel written back is W * mask.

The pruned network is saved to cpr_save_path_ws and restored into the training network; the masks are the restored kernels' non-zero
input channels, and the whole network is fine-tuned with Momentum on masked gradients (:146-285, :525-544).

Host draws go through NumPy's global generator in the reference's order (per layer: randint pairs per mini-batch and crop, choice,
choice, uniform), so a seeded run picks the reference's rows and initial mask.  Selection runs in float32 on two float32 copies of the
network whatever --compute_dtype says (the reference's reconstruction checks need it); the fine-tune honours --compute_dtype.
"""
from __future__ import annotations

import logging
import math
import os
from timeit import default_timer as timer

import numpy as np
import torch

from pocketflow_amd import hip
from pocketflow_amd.flags import FLAGS, flags
from pocketflow_amd.graph import Conv2D, Graph
from pocketflow_amd.learners.abstract_learner import AbstractLearner, input_spec
from pocketflow_amd.learners.channel_pruning_gpu.learner import get_vars_by_scope
from pocketflow_amd.learners.distillation_helper import DistillationHelper
from pocketflow_amd.learners.layerwise import forward_tapped, layers_of_vars
from pocketflow_amd.learners.weight_sparsification.learner import calc_prune_ratio
from pocketflow_amd.optim import FlatOptimizer
from pocketflow_amd.utils import checkpoint
from pocketflow_amd.utils.multi_gpu_wrapper import MultiGpuWrapper as mgw

flags.DEFINE_string('cpr_save_path', './models_cpr/model.ckpt', 'CPR: model\'s save path')
flags.DEFINE_string('cpr_save_path_eval', './models_cpr_eval/model.ckpt', 'CPR: model\'s save path for evaluation')
flags.DEFINE_string('cpr_save_path_ws', './models_cpr_ws/model.ckpt', 'CPR: model\'s save path for warm start')
flags.DEFINE_float('cpr_prune_ratio', 0.5, 'CPR: pruning ratio')
flags.DEFINE_boolean('cpr_skip_frst_layer', True, 'CPR: skip the first layer for pruning')
flags.DEFINE_boolean('cpr_skip_last_layer', False, 'CPR: skip the last layer for pruning')
flags.DEFINE_string('cpr_skip_op_names', None, 'CPR: comma-separated Conv2D operations names to be skipped')
flags.DEFINE_integer('cpr_nb_smpls', 5000, 'CPR: # of cached training samples for channel pruning')
flags.DEFINE_integer('cpr_nb_crops_per_smpl', 10, 'CPR: # of random crops per sample')
flags.DEFINE_float('cpr_ista_lrn_rate', 1e-2, 'CPR: ISTA\'s learning rate')
flags.DEFINE_integer('cpr_ista_nb_iters', 100, 'CPR: # of iterations in ISTA')
flags.DEFINE_float('cpr_lstsq_lrn_rate', 1e-3, 'CPR: least-sqaure regression\'s learning rate')
flags.DEFINE_integer('cpr_lstsq_nb_iters', 100, 'CPR: # of iterations in least-square regression')
flags.DEFINE_boolean('cpr_warm_start', False, 'CPR: use a channel-pruned model for warm start '
                     '(the channel selection process will be skipped)')

log = logging.getLogger('pocketflow_amd')

ADAM_BETA1, ADAM_BETA2, ADAM_EPS = 0.9, 0.999, 1e-8


def same_pads_ref(size: int, k: int, stride: int) -> int:
  """Leading pad of 'SAME' as the reference's sampler computes it (:666-671)."""
  p = max(k - (stride if size % stride == 0 else size % stride), 0)
  return p // 2


def layer_pads(layer: Conv2D, ih: int, iw: int):
  """(pad_t, pad_l) of a layer's tap input: 'VALID' 0; a fixed pad (ResNet's strided convolutions, whose tap holds the unpadded tensor
  that the reference pads with tf.pad first: the padded taps read zeros either way); 'SAME' by the reference's formula."""
  if isinstance(layer.padding, int):
    return layer.padding, layer.padding
  if layer.padding == 'VALID':
    return 0, 0
  return same_pads_ref(ih, layer.k, layer.stride), same_pads_ref(iw, layer.k, layer.stride)


def lstsq_rate(step: int, lrn_rate: float) -> float:
  """lrn_rate * sqrt(1 - beta2^t) / (1 - beta1^t) with TF's float32 rounding of each op (:506-507)."""
  f = np.float32
  t = f(step)
  return float(f(lrn_rate) * np.sqrt(f(1.0) - np.power(f(ADAM_BETA2), t)) / (f(1.0) - np.power(f(ADAM_BETA1), t)))


def draw_positions(oh: int, ow: int, crops: int) -> np.ndarray:
  """One mini-batch's output positions, (oh, ow) per crop, drawn as the reference's sampler draws them (:675-677)."""
  return np.array([(np.random.randint(oh), np.random.randint(ow)) for __ in range(crops)], dtype=np.int32)


def draw_selection(nb_insts: int, nb_insts_min: int, c_out: int, c_in: int):
  """The draws after sampling, in the reference's order: the primary row choice (:609), the secondary choice (:748-749) and the
  initial LASSO mask (:766)."""
  idxs_inst = np.random.choice(nb_insts, size=(nb_insts_min), replace=False)
  bs_rdc = int(math.ceil(min(nb_insts_min, nb_insts_min / c_out * 10.0)))
  idxs_rdc = np.random.choice(nb_insts_min, size=(bs_rdc), replace=False)
  mask_init = np.random.uniform(size=(c_in, 1))
  return idxs_inst, idxs_rdc, mask_init


class LayerSelector(object):
  """Device buffers and the three selection steps of one layer (used by the learner and by tools/gpu/cpr_select_timing.py)."""

  def __init__(self, device):
    self.device = device
    self.timings = {}

  def _tick(self, name, t0):
    if self.device.type == 'cuda':
      torch.cuda.synchronize()
    self.timings[name] = self.timings.get(name, 0.0) + (timer() - t0)

  def lasso(self, P, Y, idxs_rdc, w_krsc, kk, c_in, c_out, mask_init, nb_chns_nnz_target, log_fn=None):
    """Gram + gamma search (:757-813); returns (binary mask as a bool tensor, [(gamma, nnz), ...])."""
    dev = self.device
    t0 = timer()
    ws = torch.empty(hip.cpr_gram_ws(c_in), dtype=torch.float64, device=dev)
    xtx = torch.empty(c_in * c_in, dtype=torch.float32, device=dev)
    xty = torch.empty(c_in, dtype=torch.float32, device=dev)
    idx = torch.from_numpy(np.asarray(idxs_rdc, dtype=np.int32)).to(dev)
    hip.cpr_gram(P, Y, idx, kk, c_in, c_out, w_krsc, ws, xtx, xty)
    del ws
    self._tick('gram', t0)
    t0 = timer()
    m0 = torch.from_numpy(np.asarray(mask_init, dtype=np.float32).reshape(-1)).to(dev)
    m_ws = torch.empty(2 * c_in, dtype=torch.float32, device=dev)
    mask = torch.empty(c_in, dtype=torch.float32, device=dev)
    nnz_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    path = []

    def solve(x):
      hip.cpr_ista(xtx, xty, m0, m_ws, mask, x, FLAGS.cpr_ista_lrn_rate, FLAGS.cpr_ista_nb_iters, nnz_dev)
      nnz = int(nnz_dev.item())
      path.append((x, nnz))
      if log_fn is not None:
        log_fn('x = %e -> nb_chns_nnz = %d' % (x, nnz))
      return nnz

    ubnd = 0.1
    while True:
      nb_chns_nnz = solve(ubnd)
      if nb_chns_nnz <= nb_chns_nnz_target:
        break
      ubnd *= 2.0
    lbnd = 0.0
    while nb_chns_nnz != nb_chns_nnz_target and ubnd - lbnd > 1e-8:
      val = (lbnd + ubnd) / 2.0
      nb_chns_nnz = solve(val)
      if nb_chns_nnz < nb_chns_nnz_target:
        ubnd = val
      elif nb_chns_nnz > nb_chns_nnz_target:
        lbnd = val
      else:
        break
    keep = mask.abs() > 0.0
    self._tick('ista', t0)
    return keep, path

  def lstsq(self, P, Y, N, w_krsc, kk, c_in, c_out, keep, wd):
    """Adam least squares (:815-841) on the kept channels; returns (new KRSC kernel * mask, (loss_reg, loss_dcy) before, after)."""
    dev = self.device
    t0 = timer()
    K = kk * c_in
    keep_np = keep.cpu().numpy().astype(bool)
    kidx_np = np.array([k * c_in + c for k in range(kk) for c in range(c_in) if keep_np[c]], dtype=np.int32)
    pos_np = np.full(K, -1, dtype=np.int32)
    pos_np[kidx_np] = np.arange(kidx_np.size, dtype=np.int32)
    kidx = torch.from_numpy(kidx_np).to(dev)
    pos = torch.from_numpy(pos_np).to(dev)
    w_mat = w_krsc.view(c_out, kk, c_in).permute(1, 2, 0).reshape(K, c_out).contiguous()        # HWIO -> [K][Co]
    m = torch.zeros_like(w_mat)
    v = torch.zeros_like(w_mat)
    R = torch.empty(N * c_out, dtype=torch.float32, device=dev)
    part = torch.empty(max(hip.cpr_lstsq_splits(N, kidx_np.size, c_out) * kidx_np.size * c_out, 1), dtype=torch.float32, device=dev)

    def losses():
      hip.cpr_lstsq_resid(P, kidx, w_mat, Y, R, N, c_out)
      loss_reg = float(np.float32((R.double() ** 2).sum().item() / 2.0) / np.float32(N))
      loss_dcy = float(np.float32(wd) * np.float32((w_mat.double() ** 2).sum().item() / 2.0))
      return loss_reg, loss_dcy

    before = losses()
    c1, c2 = float(np.float32(1.0 - ADAM_BETA1)), float(np.float32(1.0 - ADAM_BETA2))
    for step in range(1, FLAGS.cpr_lstsq_nb_iters + 1):
      hip.cpr_lstsq_step(P, kidx, pos, Y, R, w_mat, m, v, part, N, c_out, wd, lstsq_rate(step, FLAGS.cpr_lstsq_lrn_rate),
                         ADAM_BETA1, ADAM_BETA2, c1, c2, ADAM_EPS)
    after = losses()
    w_new = (w_mat.view(kk, c_in, c_out) * keep.view(1, c_in, 1).float()).permute(2, 0, 1).contiguous().view(-1)
    self._tick('lstsq', t0)
    return w_new, before, after


class ChannelPrunedRmtLearner(AbstractLearner):  # pylint: disable=too-many-instance-attributes
  """Channel pruning learner - remastered."""

  def __init__(self, sm_writer, model_helper):
    super(ChannelPrunedRmtLearner, self).__init__(sm_writer, model_helper)
    self.model_scope_full = 'model'
    self.model_scope_prnd = 'pruned_model'
    if self.is_primary_worker('local'):
      self.download_model()  # pre-trained model is required
    self.auto_barrier()
    if FLAGS.enbl_dst:
      self.helper_dst = DistillationHelper(sm_writer, model_helper, self.mpi_comm)
    self.__build_train()
    self.__build_eval()
    self.selection_log = []       # per layer: {'name', 'target', 'nnz', 'path', 'losses'}

  # -- reference surface ----------------------------------------------------------------------------------------
  def train(self):
    """Choose channels (or warm-start from cpr_save_path_ws), then fine-tune with the chosen channels only (:146-193)."""
    if not FLAGS.cpr_warm_start:
      time_prev = timer()
      self.__choose_channels()
      log.info('time (channel selection): %.2f (s)' % (timer() - time_prev))
    save_path = checkpoint.latest_checkpoint(os.path.dirname(FLAGS.cpr_save_path_ws))
    self.restore_vars(save_path)
    log.info('model restored from ' + save_path)
    self.__init_masks()
    if FLAGS.enbl_multi_gpu:
      self.bcast_op()

    if self.is_primary_worker('global'):
      self.__save_model(is_train=True)
      self.evaluate()
    self.auto_barrier()

    nb_iters = FLAGS.nb_iters_override or self.nb_iters_train
    time_prev = timer()
    for idx_iter in range(nb_iters):
      log_rslt = self.train_step()
      if (idx_iter + 1) % FLAGS.summ_step == 0 and self.is_primary_worker('global'):
        self.__monitor_progress(log_rslt, idx_iter, timer() - time_prev)
        time_prev = timer()
      if self.is_primary_worker('global') and (idx_iter + 1) % FLAGS.save_step == 0:
        self.__save_model(is_train=True)
        self.evaluate()
      self.auto_barrier()

    rslt = None
    if self.is_primary_worker('global'):
      self.__save_model(is_train=True)
      self.__restore_model(is_train=False)
      self.__save_model(is_train=False)
      rslt = self.evaluate()
    return rslt

  def evaluate(self):
    """Restore a model from the latest checkpoint files and then evaluate it (:195-209)."""
    self.__restore_model(is_train=False)
    return self.run_eval()

  def run_eval(self):
    nb_iters = FLAGS.nb_eval_batches_override or int(np.ceil(float(FLAGS.nb_smpls_eval) / FLAGS.batch_size_eval))
    g = self.graph
    g.store.sync_compute()
    self.iter_eval.reset()
    pr_trn = calc_prune_ratio(self.vars_prnd['trainable'], self.device)
    pr_krn = calc_prune_ratio(self.vars_prnd['maskable'], self.device)
    rows, names = [], None
    self.dump_n_eval(outputs=None, action='init')
    with torch.no_grad():
      for __ in range(nb_iters):
        images, labels = self.iter_eval.get_next()
        x, y = self.to_device(images, labels)
        g.begin_step()
        with g.as_default():
          logits = self.forward_eval(x)
          loss, metrics = self.calc_loss(y, logits, self.vars_prnd['trainable'])
          if FLAGS.enbl_dst:
            loss = loss + self.helper_dst.calc_loss(logits, self.helper_dst.calc_logits(None, x))
        self.dump_n_eval(outputs=logits, action='dump')
        names = ['loss', 'pr_trn', 'pr_krn'] + list(metrics.keys())
        rows.append([float(loss), pr_trn, pr_krn] + [float(v) for v in metrics.values()])
    self.dump_n_eval(outputs=None, action='eval')
    means = np.mean(np.array(rows), axis=0)
    out = {}
    for idx, name in enumerate(names):
      log.info('%s = %.4e' % (name, means[idx]))
      out[name] = float(means[idx])
    return out

  def train_step(self):
    """train_op: fwd, loss (+ distillation), bwd, [all-reduce], grad * mask + Momentum in one fused launch."""
    g = self.graph
    g.store.sync_compute()
    images, labels = self.iter_train.get_next()
    x, y = self.to_device(images, labels)
    g.begin_step()
    with g.as_default():
      logits_dst = self.helper_dst.calc_logits(None, x) if FLAGS.enbl_dst else None
      logits = self.forward_train(x)
      if FLAGS.enbl_dst:
        self.helper_dst.prime(logits, logits_dst)           # both losses out of calc_loss's one kernel launch
      loss, metrics = self.calc_loss(y, logits, self.vars_prnd['trainable'])
      if FLAGS.enbl_dst:
        loss = loss + self.helper_dst.calc_loss(logits, logits_dst)
    self.optimizer.backward(loss)
    lr = self.lrn_rate(self.global_step)
    self.optimizer.weight_decay = g.store.weight_decay
    self.optimizer.compute_gradients()
    self.optimizer.apply_gradients(lr)
    self.global_step += 1
    return [lr, float(loss.detach()), None, None] + [float(v) for v in metrics.values()], list(metrics.keys())

  # -- graphs ------------------------------------------------------------------------------------------------------
  def __build_train(self):
    self.graph = self.build_graph(self.model_scope_prnd)
    st = self.graph.store
    self.iter_train = self.build_dataset_train().to(self.device)
    self.vars_prnd = get_vars_by_scope(self.graph)
    self.global_step = 0
    self.lrn_rate, self.nb_iters_train = self.setup_lrn_rate(self.global_step)
    self.masks = torch.ones_like(st.w_master)                   # all pruning masks, one flat buffer
    base = FlatOptimizer(st, 'momentum', momentum=FLAGS.momentum)
    base.w_mask = self.masks
    self.optimizer = base if not FLAGS.enbl_multi_gpu else mgw.DistributedOptimizer(base)
    if FLAGS.enbl_multi_gpu:
      self.bcast_op = mgw.broadcast_global_variables(0, [st], [self.optimizer])

  def __build_eval(self):
    self.iter_eval = self.build_dataset_eval().to(self.device)

  def __build_f32_graph(self, scope, requires_grad):
    """build_graph with float32 compute whatever --compute_dtype says (the selection networks)."""
    graph = Graph(scope, self.device, torch.float32)
    graph.fuse_conv1x1 = False
    with graph.as_default():
      self.forward_train(input_spec(self.model_helper))
    graph.finalize(seed=FLAGS.init_seed, requires_grad=requires_grad)
    return graph

  def __build_prune(self):
    """The selection graphs (__build_prune :324-395): the full network restored from the pre-trained model and the pruned network
    initialised as its copy; built only when selection runs."""
    self.graph_full = self.__build_f32_graph(self.model_scope_full, False)
    self.graph_prnd = self.__build_f32_graph(self.model_scope_prnd, False)
    save_path = checkpoint.latest_checkpoint(os.path.dirname(FLAGS.save_path))
    self.graph_full.store.load_numpy(checkpoint.load(save_path), strict=False)
    st_f, st_p = self.graph_full.store, self.graph_prnd.store
    st_p.w_master.copy_(st_f.w_master)
    st_p.o_master.copy_(st_f.o_master)
    st_p.state.copy_(st_f.state)
    st_p.sync_compute()
    self.vars_full = get_vars_by_scope(self.graph_full)
    self.vars_sel = get_vars_by_scope(self.graph_prnd)
    images, __ = self.iter_train.get_next()
    self.iter_train.reset()
    state_f, state_p = st_f.state.clone(), st_p.state.clone()
    try:
      self.core_full = layers_of_vars(self.graph_full, self.forward_train, images, self.vars_full['maskable'], grad=True)
      self.core_prnd = layers_of_vars(self.graph_prnd, self.forward_train, images, self.vars_sel['maskable'], grad=True)
    finally:
      st_f.state.copy_(state_f)                                    # training-mode BN moved the moving statistics: restore both
      st_p.state.copy_(state_p)
    assert all(isinstance(l, Conv2D) for l in self.core_prnd)

  def __init_masks(self):
    """mask = (sum_{h, w, o} W^2 > 0) per input channel of every conv kernel of the restored model (:257-263), then fresh slots."""
    st = self.graph.store
    for var in self.vars_prnd['maskable']:
      kh, kw, cin, cout = var.ref_shape
      sl = slice(var.offset, var.offset + var.numel)
      norm = (st.w_master[sl].view(cout, kh * kw, cin).float() ** 2).sum(dim=(0, 1))
      keep_in = (norm > 0.0).to(torch.uint8)
      keep_out = torch.ones(cout, dtype=torch.uint8, device=keep_in.device)
      hip.cp_build_mask(self.masks[sl], keep_in, keep_out, cout, kh * kw, cin)
    self.global_step = 0
    self.optimizer.reset_slots()
    st.sync_compute()

  # -- channel selection ---------------------------------------------------------------------------------------------------
  def __tapped_pair(self, idx, images):
    """(input of the pruned network, output of the full network, input of the full network, output of the pruned network) at layer
    idx, both networks in training mode with their BN statistics left where they were."""
    layer_f, layer_p = self.core_full[idx], self.core_prnd[idx]
    st_f, st_p = self.graph_full.store, self.graph_prnd.store
    state_f, state_p = st_f.state.clone(), st_p.state.clone()
    try:
      tf_ = forward_tapped(self.graph_full, self.forward_train, images, layer_f, tap_dense=False, grad=True)[layer_f]
      tp_ = forward_tapped(self.graph_prnd, self.forward_train, images, layer_p, tap_dense=False, grad=True)[layer_p]
    finally:
      st_f.state.copy_(state_f)
      st_p.state.copy_(state_p)
    cl = torch.channels_last

    def conv_out(layer, x, y):
      # the reference reads the Conv2D op's output, which is before the bias of a biased layer (MobileNet's logits): that layer's
      # convolution is run once more without its bias, so the sampled outputs are the convolution's own values
      if layer.bias is not None:
        bias, layer.bias = layer.bias, None
        try:
          with torch.no_grad():
            y = layer.plain(x.detach())
        finally:
          layer.bias = bias
      return y.detach().contiguous(memory_format=cl)
    return (tp_[0].detach().contiguous(memory_format=cl), conv_out(layer_f, tf_[0], tf_[1]), tf_[0].detach().contiguous(memory_format=cl),
            conv_out(layer_p, tp_[0], tp_[1]))

  def __check_recon(self, P, Y, w_krsc, kk, c_in, c_out, name):
    """The reference's reconstruction asserts (:717-723): ||Y - P W||^2 / size < 1e-6, in float64."""
    w = w_krsc.view(c_out, kk * c_in).double().t()
    err = float(((Y.view(-1, c_out).double() - P.view(-1, kk * c_in).double() @ w) ** 2).mean())
    assert err < 1e-6, 'unable to recover output feature maps - %s (%e)' % (name, err)

  def __choose_channels(self):  # pylint: disable=too-many-locals,too-many-statements
    """__choose_channels (:546-649) with the per-layer arithmetic on the device."""
    self.__build_prune()
    nb_layers = len(self.core_prnd)
    prune_ratios = [FLAGS.cpr_prune_ratio] * nb_layers
    if FLAGS.cpr_skip_frst_layer:
      prune_ratios[0] = 0.0
    if FLAGS.cpr_skip_last_layer:
      prune_ratios[-1] = 0.0
    skip_names = FLAGS.cpr_skip_op_names.split(',') if FLAGS.cpr_skip_op_names is not None else []
    for idx_layer, var in enumerate(self.vars_sel['maskable']):
      for skip_name in skip_names:
        if skip_name in var.name:
          prune_ratios[idx_layer] = 0.0
          log.info('skip %s since no pruning is required' % var.name)
          break

    nb_mbtcs = int(math.ceil(FLAGS.cpr_nb_smpls / FLAGS.batch_size))
    images_cached = [self.iter_train.get_next()[0] for __ in range(nb_mbtcs)]
    primary = self.is_primary_worker('global')
    sel = LayerSelector(self.device)
    st_p = self.graph_prnd.store
    crops = FLAGS.cpr_nb_crops_per_smpl
    nb_insts_min = crops * FLAGS.cpr_nb_smpls
    self.selection_log = []
    for idx_layer in range(nb_layers):
      prune_ratio = prune_ratios[idx_layer]
      var, layer = self.vars_sel['maskable'][idx_layer], self.core_prnd[idx_layer]
      var_full = self.vars_full['maskable'][idx_layer]
      kh, kw, c_in, c_out = var.ref_shape
      kk = kh * kw
      if primary:
        log.info('layer #%d: pr = %.2f (target)' % (idx_layer, prune_ratio))
        log.info('kernel name = {}'.format(var.name))
        log.info('kernel shape = {}'.format(list(var.ref_shape)))
      w_full = self.graph_full.store.w_master[var_full.offset:var_full.offset + var_full.numel]
      w_prnd = st_p.w_master[var.offset:var.offset + var.numel].clone()

      # sampling (:586-607)
      time_beg = timer()
      P = Y = None
      nb_insts = 0
      for idx_mbtc in range(nb_mbtcs):
        x_p, y_f, x_f, y_p = self.__tapped_pair(idx_layer, images_cached[idx_mbtc])
        bs, __, ih, iw = x_p.shape
        oh, ow = y_f.shape[2], y_f.shape[3]
        if P is None:
          cap = min(nb_mbtcs, -(-(nb_insts_min + 1) // (crops * bs))) * crops * bs
          P = torch.empty(cap * kk * c_in, dtype=torch.float32, device=self.device)
          Y = torch.empty(cap * c_out, dtype=torch.float32, device=self.device)
        pos = torch.from_numpy(draw_positions(oh, ow, crops)).to(self.device)
        pad_t, pad_l = layer_pads(layer, ih, iw)
        t0 = timer()
        hip.cpr_gather(x_p, y_f, pos, kh, kw, layer.stride, pad_t, pad_l, P, Y, nb_insts)
        # the reference's checks: full patches x full kernel ~ full outputs, pruned patches x pruned kernel ~ pruned outputs
        n_mb = crops * bs
        P_chk = torch.empty(n_mb * kk * c_in, dtype=torch.float32, device=self.device)
        Y_chk = torch.empty(n_mb * c_out, dtype=torch.float32, device=self.device)
        hip.cpr_gather(x_f, y_p, pos, kh, kw, layer.stride, pad_t, pad_l, P_chk, Y_chk, 0)
        sel._tick('gather', t0)
        self.__check_recon(P_chk, Y[nb_insts * c_out:(nb_insts + n_mb) * c_out], w_full, kk, c_in, c_out, 'full')
        self.__check_recon(P[nb_insts * kk * c_in:(nb_insts + n_mb) * kk * c_in], Y_chk, w_prnd, kk, c_in, c_out, 'prnd')
        nb_insts += n_mb
        if nb_insts > nb_insts_min:
          break
      idxs_inst, idxs_rdc, mask_init = draw_selection(nb_insts, nb_insts_min, c_out, c_in)
      sel_rows = torch.from_numpy(idxs_inst.astype(np.int64)).to(self.device)
      P = P.view(-1, kk * c_in)[:nb_insts].index_select(0, sel_rows).contiguous().view(-1)
      Y = Y.view(-1, c_out)[:nb_insts].index_select(0, sel_rows).contiguous().view(-1)
      sel.timings['sampling'] = sel.timings.get('sampling', 0.0) + (timer() - time_beg)
      log.info('time elapsed (sampling): %.4f (s)' % (timer() - time_beg))

      # LASSO (:727-813)
      time_beg = timer()
      N = nb_insts_min
      nb_chns_nnz_target = int(c_in * (1.0 - prune_ratio))
      keep, path = sel.lasso(P, Y, idxs_rdc, w_prnd, kk, c_in, c_out, mask_init, nb_chns_nnz_target, log.info)
      nnz = int(keep.sum())
      if nnz != nb_chns_nnz_target:
        log.info('gamma search exhausted: nb_chns_nnz = %d (target %d)' % (nnz, nb_chns_nnz_target))

      # least squares (:815-841)
      w_new, before, after = sel.lstsq(P, Y, N, w_prnd, kk, c_in, c_out, keep, FLAGS.loss_w_dcy)
      log.info('losses: %e (reg) / %e (dcy)' % before)
      log.info('losses: %e (reg) / %e (dcy)' % after)
      st_p.w_master[var.offset:var.offset + var.numel].copy_(w_new)
      st_p.sync_compute()
      del P, Y
      log.info('time elapsed (selection): %.4f (s)' % (timer() - time_beg))
      self.selection_log.append({'name': var.name, 'target': nb_chns_nnz_target, 'nnz': nnz, 'path': path,
                                 'losses': (before, after)})
      pr_trn = calc_prune_ratio(self.vars_sel['trainable'], self.device)
      pr_krn = calc_prune_ratio(self.vars_sel['maskable'], self.device)
      log.info('pruning ratios: %e (trn) / %e (krn)' % (pr_trn, pr_krn))
    self.selection_timings = dict(sel.timings)

    if self.is_primary_worker('global'):
      save_path = checkpoint.save(st_p.export_numpy(), FLAGS.cpr_save_path_ws, None, fmt=FLAGS.ckpt_format)
      log.info('model saved to ' + save_path)
    self.auto_barrier()
    del self.graph_full, self.graph_prnd, self.core_full, self.core_prnd

  # -- checkpoints / logging -------------------------------------------------------------------------------------------------
  def __save_model(self, is_train):
    if is_train:
      save_path = self.save_vars(FLAGS.cpr_save_path, self.global_step)
    else:
      save_path = self.save_vars(FLAGS.cpr_save_path_eval)
    log.info('model saved to ' + save_path)

  def __restore_model(self, is_train):
    save_path = checkpoint.latest_checkpoint(os.path.dirname(FLAGS.cpr_save_path))
    self.restore_vars(save_path)
    log.info('model restored from ' + save_path)

  def __monitor_progress(self, log_rslt, idx_iter, time_step):
    vals, metric_names = log_rslt
    vals[2] = calc_prune_ratio(self.vars_prnd['trainable'], self.device)
    vals[3] = calc_prune_ratio(self.vars_prnd['maskable'], self.device)
    names = ['lr', 'loss', 'pr_trn', 'pr_krn'] + metric_names
    if self.sm_writer is not None:
      self.sm_writer.add_summary(dict(zip(names, vals)), idx_iter)
    speed = FLAGS.batch_size * FLAGS.summ_step / time_step
    if FLAGS.enbl_multi_gpu:
      speed *= mgw.size()
    log_str = ' | '.join(['%s = %.4e' % (name, value) for name, value in zip(names, vals)])
    log.info('iter #%d: %s | speed = %.2f pics / sec' % (idx_iter + 1, log_str, speed))
    self.last_speed = speed
