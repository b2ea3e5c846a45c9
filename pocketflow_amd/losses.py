"""Loss ops of the hot path as autograd functions over the fused HIP loss kernel.

`softmax_cross_entropy(labels, logits)` == tf.losses.softmax_cross_entropy (mean over the batch of
-sum_c labels*log_softmax(logits)); `distillation_loss` == DistillationHelper.calc_loss
(learners/distillation_helper.py:86-103).  Forward and backward come out of ONE kernel launch
(pf_ce_distill_fwd_bwd); backward only rescales the stored dlogits by the upstream scalar.

The training step's head (PF_HEAD_FUSE, graph.HEAD_FUSE): when the learner has told the logits tensor about the teacher
(`prime_distillation`, before ModelHelper.calc_loss), `softmax_cross_entropy` runs ONE launch for both losses, the top-1 / top-5
accuracy and both terms of dlogits (pf_ce_distill_head) and leaves the rest on the tensor; `distillation_loss` and
`top_k_accuracies` pick their part up when they are asked about the same tensors, and backward is one pf_ce_combine launch.
Without the priming the same launch runs without the soft term; values and gradients are bit for bit those of the separate path.
"""
from __future__ import annotations

import torch

from pocketflow_amd import hip


def _run_kernel(z_s, labels, z_t, tempr, loss_w):
  B, C = z_s.shape
  z_s = z_s.contiguous()
  losses = torch.empty(2, dtype=torch.float32, device=z_s.device)
  dz = torch.empty((B, C), dtype=z_s.dtype, device=z_s.device)
  row_ws = torch.empty(B * 2, dtype=torch.float32, device=z_s.device)
  hip.ce_distill_fwd_bwd(z_s, labels, z_t, tempr, loss_w, losses, dz, row_ws)
  return losses, dz


class _SoftmaxCE(torch.autograd.Function):
  @staticmethod
  def forward(ctx, logits, labels):
    losses, dz = _run_kernel(logits, labels.contiguous().float(), None, 1.0, 0.0)
    ctx.save_for_backward(dz)
    return losses[0]

  @staticmethod
  def backward(ctx, g):
    (dz,) = ctx.saved_tensors
    return dz * g.to(dz.dtype), None


class _DistillCE(torch.autograd.Function):
  @staticmethod
  def forward(ctx, logits_pri, logits_dst, tempr, loss_w):
    zeros = torch.zeros(logits_pri.shape, dtype=torch.float32, device=logits_pri.device)
    losses, dz = _run_kernel(logits_pri, zeros, logits_dst.contiguous(), float(tempr), float(loss_w))
    ctx.save_for_backward(dz)
    return losses[1]

  @staticmethod
  def backward(ctx, g):
    (dz,) = ctx.saved_tensors
    return dz * g.to(dz.dtype), None, None, None


class _HeadCE(torch.autograd.Function):
  """(L_model, L_dst, [top-1, top-5]) of one pf_ce_distill_head launch; the two terms of dlogits are kept apart because the upstream
  gradients of the two losses are device scalars: backward joins them in one pf_ce_combine launch, with the roundings autograd
  applied to `dz * g.to(dz.dtype)` per term and to the sum of the two."""

  @staticmethod
  def forward(ctx, logits, labels, logits_dst, tempr, loss_w):
    B, C = logits.shape
    z = logits.contiguous()
    out = torch.empty(4, dtype=torch.float32, device=z.device)
    dz_hard = torch.empty((B, C), dtype=z.dtype, device=z.device)
    dz_soft = torch.empty((B, C), dtype=z.dtype, device=z.device) if logits_dst is not None else None
    row_ws = torch.empty(B * 3, dtype=torch.float32, device=z.device)
    hip.ce_distill_head(z, labels, logits_dst, tempr, loss_w, out, dz_hard, dz_soft, row_ws)
    ctx.save_for_backward(dz_hard, dz_soft)
    ctx.set_materialize_grads(False)
    top = out[2:4]
    ctx.mark_non_differentiable(top)
    return out[0], out[1], top

  @staticmethod
  def backward(ctx, g0, g1, _g_top):
    dz_hard, dz_soft = ctx.saved_tensors
    if dz_soft is None:
      g1 = None
    if g0 is None and g1 is None:
      return None, None, None, None, None
    dz = torch.empty_like(dz_hard)
    hip.ce_combine(dz_hard, dz_soft if g1 is not None else None, g0.float() if g0 is not None else None,
                   g1.float() if g1 is not None else None, dz)
    return dz, None, None, None, None


def _head_ok(logits) -> bool:
  from pocketflow_amd import graph as G            # (graph.py reads the PF_* switches; it does not import this module)
  return (G.HEAD_FUSE and logits.dim() == 2 and (logits.is_cuda or G.HEAD_FUSE_ANY_DEVICE)
          and logits.dtype in (torch.float32, torch.bfloat16)
          and hasattr(hip, 'ce_distill_head') and hasattr(hip, 'ce_combine'))


def prime_distillation(logits_pri: torch.Tensor, logits_dst: torch.Tensor, tempr: float, loss_w: float) -> None:
  """Called by a learner BEFORE ModelHelper.calc_loss when DistillationHelper.calc_loss(logits_pri, logits_dst) follows it: lets
  `softmax_cross_entropy(labels, logits_pri)` compute both terms in its one launch.  Learners that do not call it lose nothing
  but the fusion."""
  if _head_ok(logits_pri):
    logits_pri._pf_dst = (logits_dst, float(tempr), float(loss_w))


def softmax_cross_entropy(labels: torch.Tensor, logits: torch.Tensor) -> torch.Tensor:
  if not _head_ok(logits):
    return _SoftmaxCE.apply(logits, labels)
  dst, tempr, loss_w = getattr(logits, '_pf_dst', None) or (None, 1.0, 0.0)
  z_t = dst.detach().contiguous() if dst is not None else None
  loss, loss_dst, top = _HeadCE.apply(logits, labels.contiguous().float(), z_t, tempr, loss_w)
  logits._pf_head = dict(labels=labels, dst=dst, tempr=tempr, loss_w=loss_w, loss_dst=loss_dst, top=top)
  return loss


def distillation_loss(logits_pri: torch.Tensor, logits_dst: torch.Tensor, tempr: float,
                      loss_w: float) -> torch.Tensor:
  h = getattr(logits_pri, '_pf_head', None)
  if h is not None and h['dst'] is logits_dst and h['tempr'] == float(tempr) and h['loss_w'] == float(loss_w):
    return h['loss_dst']                           # computed by softmax_cross_entropy's launch on the same tensors
  return _DistillCE.apply(logits_pri, logits_dst.detach(), tempr, loss_w)


def l2_regularization(trainable_vars, loss_filter, loss_w_dcy: float) -> torch.Tensor:
  """loss_w_dcy * add_n([tf.nn.l2_loss(v) for v in trainable_vars if loss_filter(v)]).

  The VALUE is returned (for the logged loss); its GRADIENT (wd * v) is applied inside the fused
  optimiser kernel, so the returned tensor is detached.  The filter must agree with the `l2` flag
  each variable was declared with (that flag decides the layout of the flat buffers)."""
  tot = None
  store = None
  for v in trainable_vars:
    want = bool(loss_filter(v))
    if want != bool(v.l2):
      raise ValueError('calc_loss regularises %s but the variable was declared with l2=%s' % (v.name, v.l2))
    store = store or getattr(v, 'store', None)
  store = store or (trainable_vars[0].store if trainable_vars else None)
  if store is None:
    return torch.zeros(())
  store.weight_decay = float(loss_w_dcy)
  w = store.w_master[:store.w_decay]
  o = store.o_master[:store.o_decay]
  tot = 0.5 * (torch.dot(w, w) + torch.dot(o, o))
  return (loss_w_dcy * tot).detach()


def in_top_k(outputs: torch.Tensor, targets: torch.Tensor, k: int) -> torch.Tensor:
  """tf.nn.in_top_k: fewer than k entries are strictly greater than the target's score."""
  o = outputs.float()
  t = o.gather(1, targets.view(-1, 1))
  return (o > t).sum(dim=1) < k


def top_k_accuracies(labels: torch.Tensor, outputs: torch.Tensor, ks=(1, 5)):
  """[in_top_k(outputs, argmax(labels), k).float().mean() for k in ks]: from the head launch of `softmax_cross_entropy` when it ran
  on these very tensors (it counts, per row, the logits above the label's -- pf_ce_distill_head), otherwise computed here."""
  h = getattr(outputs, '_pf_head', None)
  if h is not None and h['labels'] is labels and all(k in (1, 5) for k in ks):
    return [h['top'][0 if k == 1 else 1] for k in ks]
  targets = labels.argmax(dim=1)
  return [in_top_k(outputs, targets, k).float().mean() for k in ks]
