"""The fused network head on the GPU (PF_HEAD_FUSE): the last BN reduced to its spatial mean in pass 2 (pf_bn_act_quant_pool), the
pooled forms of the two BN-backward passes, and the step's one loss launch (pf_ce_distill_head + pf_ce_combine) -- each against the
separate kernels it replaces, then a whole training step with the switch off and on."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 3
HWS = (49, 4, 1)
ACTS = ('Relu', 'Relu6', None)
QUANT = (None, 8, 4)
DTYPES = {'bf16': torch.bfloat16, 'f32': torch.float32}
# C = 64 / 2048: the 16-byte path (several images per workgroup / one workgroup per image); 24 / 20: the element-wise path
CHANNELS = (64, 2048, 24, 20)


def _bn_inputs(C, hw, dtype, seed):
  gen = torch.Generator(device='cpu').manual_seed(seed)
  x = (torch.randn(B * hw, C, generator=gen) * 1.5).to(dtype).cuda()
  ss = torch.stack([0.5 + torch.rand(C, generator=gen), 0.5 * torch.randn(C, generator=gen)]).float().cuda().contiguous()
  return x, ss, gen


def _slot_of(hip, x, ss, act):
  """The min/max slot of y = act(scale * x + shift), filled by the product's own kernels."""
  y = torch.empty_like(x)
  hip.bn_act_quant_apply(x, y, x.shape[0], x.shape[1], ss, act, None, 8, False)
  slot = torch.zeros(2, dtype=torch.int32, device='cuda')
  hip.minmax_slots_init(slot)
  hip.minmax_tensor(y, slot, None)
  return slot


@pytest.mark.parametrize('C', CHANNELS)
@pytest.mark.parametrize('dt', sorted(DTYPES))
def test_pooled_forward_is_the_mean_of_what_the_apply_pass_stores(dt, C):
  """pooled == T(float64 mean over the pixels of q), q from pf_bn_act_quant_apply on the same inputs.
  bf16: the float32 sum of HW stored values differs from the exact one by round-off, which matters only where the exact mean lies
  that close to a bf16 rounding boundary: at most 0.1 % of the elements, each by one bf16 ulp, none by more.
  f32: within HW * 2^-24 * mean|q|, the bound of a float32 sum of HW terms.  Two runs are bit-equal."""
  from pocketflow_amd import hip
  dtype = DTYPES[dt]
  for hw in HWS:
    for ai, act in enumerate(ACTS):
      for bits in QUANT:
        x, ss, _ = _bn_inputs(C, hw, dtype, 1000 * hw + 10 * ai + (bits or 0))
        rows = B * hw
        slot = _slot_of(hip, x, ss, act) if bits is not None else None
        q = torch.empty_like(x)
        hip.bn_act_quant_apply(x, q, rows, C, ss, act, slot, bits or 8, bits is not None)
        got = torch.full((B, C), float('nan'), dtype=dtype, device='cuda')
        hip.bn_act_quant_pool(x, got, rows, C, hw, ss, act, slot, bits or 8, bits is not None)
        again = torch.full((B, C), float('nan'), dtype=dtype, device='cuda')
        hip.bn_act_quant_pool(x, again, rows, C, hw, ss, act, slot, bits or 8, bits is not None)
        what = (dt, C, hw, act, bits)
        assert torch.equal(got, again), what
        q64 = q.double().view(B, hw, C)
        ref64 = q64.mean(dim=1)
        if dtype == torch.bfloat16:
          ref = ref64.float().to(dtype)
          d = (got.view(torch.int16).int() - ref.view(torch.int16).int()).abs()
          n_diff = int((d != 0).sum())
          print('pooled forward', what, 'elements off by one bf16 ulp: %d of %d' % (n_diff, d.numel()))
          assert int(d.max()) <= 1, what
          assert n_diff <= 1e-3 * d.numel(), (what, n_diff)
        else:
          bound = hw * 2.0 ** -24 * q64.abs().mean(dim=1)
          err = (got.double() - ref64).abs()
          print('pooled forward', what, 'max error / bound: %.3f' % float((err / bound.clamp_min(1e-300)).max()))
          assert bool((err <= bound).all()), what


@pytest.mark.parametrize('C', CHANNELS)
@pytest.mark.parametrize('dt', sorted(DTYPES))
def test_pooled_backward_is_bit_identical_to_the_expanded_gradient(dt, C):
  """pf_bn_bwd_stats_pooled / pf_bn_bwd_apply_pooled on the [B][C] gradient g against the plain passes on
  dq = T(float(g) / HW) expanded to [B * HW][C]: partial, dgamma, dbeta and dx, also with zero sums (the frozen form).
  dq is built with the torch expression ON THE DEVICE, as autograd's mean / cast chain builds it: there aten evaluates a division
  by a host scalar as a product with the rounded reciprocal (one float32 ulp off the quotient on some elements, which is what the
  kernels reproduce; a kernel that divides fails this test in float32)."""
  from pocketflow_amd import hip
  dtype = DTYPES[dt]
  for hw in HWS:
    for ai, act in enumerate(ACTS):
      x, ss, gen = _bn_inputs(C, hw, dtype, 77 * hw + ai)
      rows = B * hw
      mi = torch.stack([0.3 * torch.randn(C, generator=gen), 0.5 + torch.rand(C, generator=gen)]).float().cuda().contiguous()
      g = torch.randn(B, C, generator=gen).to(dtype).cuda()
      dq = (g.float() / hw).to(dtype).view(B, 1, C).expand(B, hw, C).reshape(rows, C).contiguous()
      for nblk in (1, 3):
        what = (dt, C, hw, act, nblk)
        res = []
        for pooled in (False, True):
          partial = torch.full((nblk, 2, C), float('nan'), device='cuda')
          dgamma = torch.full((C,), float('nan'), device='cuda')
          dbeta = torch.full((C,), float('nan'), device='cuda')
          dx = torch.full((rows, C), float('nan'), dtype=dtype, device='cuda')
          dx0 = torch.full((rows, C), float('nan'), dtype=dtype, device='cuda')
          zero = torch.zeros(C, device='cuda')
          if pooled:
            hip.bn_bwd_stats_pooled(g, x, rows, C, hw, ss, mi, act, partial, nblk)
            hip.bn_bwd_finalize(partial, nblk, C, dgamma, dbeta)
            hip.bn_bwd_apply_pooled(g, x, dx, rows, C, hw, ss, mi, dgamma, dbeta, act)
            hip.bn_bwd_apply_pooled(g, x, dx0, rows, C, hw, ss, mi, zero, zero, act)
          else:
            hip.bn_bwd_stats(dq, x, rows, C, ss, mi, act, partial, nblk)
            hip.bn_bwd_finalize(partial, nblk, C, dgamma, dbeta)
            hip.bn_bwd_apply(dq, x, dx, rows, C, ss, mi, dgamma, dbeta, act)
            hip.bn_bwd_apply(dq, x, dx0, rows, C, ss, mi, zero, zero, act)
          res.append((partial, dgamma, dbeta, dx, dx0))
        for name, a, b in zip(('partial', 'dgamma', 'dbeta', 'dx', 'dx (zero sums)'), *res):
          assert not bool(torch.isnan(a.float()).any()), (what, name)
          assert torch.equal(a, b), (what, name)


@pytest.mark.parametrize('C', CHANNELS)
def test_backward_apply_adds_the_shortcut_gradient(C):
  """The addend of pf_bn_bwd_apply_add, which the dense and the pooled apply pass share a kernel with.
  float32: dx with the addend == dx without it + addend in torch, bit for bit (the kernel adds the same two float32 values).
  bf16: dx == the float32 kernel's dx on the same inputs upcast to float32, rounded to bf16, bit for bit: bf16 loads are exact,
  the arithmetic is the same float32 expression (the library is built without contraction) and both stores round to nearest
  even."""
  from pocketflow_amd import hip
  for rows in (12, 70):
    for ai, act in enumerate(ACTS):
      gen = torch.Generator(device='cpu').manual_seed(5000 + 10 * rows + ai)
      x = (torch.randn(rows, C, generator=gen) * 1.5).to(torch.bfloat16)
      dq = torch.randn(rows, C, generator=gen).to(torch.bfloat16)
      a = torch.randn(rows, C, generator=gen).to(torch.bfloat16)
      ss = torch.stack([0.5 + torch.rand(C, generator=gen), 0.5 * torch.randn(C, generator=gen)]).float().cuda().contiguous()
      mi = torch.stack([0.3 * torch.randn(C, generator=gen), 0.5 + torch.rand(C, generator=gen)]).float().cuda().contiguous()
      dgamma = torch.randn(C, generator=gen).cuda()
      dbeta = torch.randn(C, generator=gen).cuda()
      what = (C, rows, act)

      def run(dtype, addend):
        dx = torch.full((rows, C), float('nan'), dtype=dtype, device='cuda')
        hip.bn_bwd_apply(dq.to(dtype).cuda(), x.to(dtype).cuda(), dx, rows, C, ss, mi, dgamma, dbeta, act, addend)
        assert not bool(torch.isnan(dx.float()).any()), (what, dtype)
        return dx

      a32 = a.float().cuda()
      with_addend = run(torch.float32, a32)
      assert torch.equal(with_addend, run(torch.float32, None) + a32), what
      assert torch.equal(run(torch.bfloat16, a.cuda()), with_addend.to(torch.bfloat16)), what


def _loss_inputs(Bn, C, dtype, seed):
  gen = torch.Generator(device='cpu').manual_seed(seed)
  z = (2.0 * torch.randn(Bn, C, generator=gen)).to(dtype)
  z_t = (2.0 * torch.randn(Bn, C, generator=gen)).to(dtype)
  tgt = torch.randint(0, C, (Bn,), generator=gen)
  # row 1: three equal top logits, the label on the middle one (tf.nn.in_top_k counts STRICTLY greater logits: a tie is in favour)
  top = float(z[1].float().max()) + 1.0
  z[1, 2] = z[1, 5] = z[1, 7] = top
  tgt[1] = 5
  # row 2: the label's logit is exactly the sixth largest (in the top 5 it is not)
  order = torch.argsort(z[2].float(), descending=True)
  tgt[2] = int(order[5])
  labels = torch.zeros(Bn, C)
  labels[torch.arange(Bn), tgt] = 1.0
  return z.cuda(), z_t.cuda(), labels.cuda(), tgt.cuda()


@pytest.mark.parametrize('teacher', [False, True])
@pytest.mark.parametrize('shape', [(5, 10), (64, 1001)])
@pytest.mark.parametrize('dt', sorted(DTYPES))
def test_one_loss_launch_equals_the_two_launches_and_autograd(dt, shape, teacher):
  from pocketflow_amd import hip, losses
  from pocketflow_amd import graph as G
  dtype = DTYPES[dt]
  Bn, C = shape
  z, z_t, labels, tgt = _loss_inputs(Bn, C, dtype, 5 + Bn)
  tempr, w = 4.0, 4.0
  # today's two launches
  l1, l2 = torch.empty(2, device='cuda'), torch.empty(2, device='cuda')
  dz1, dz2 = torch.empty_like(z), torch.empty_like(z)
  ws = torch.empty(2 * Bn, device='cuda')
  hip.ce_distill_fwd_bwd(z, labels, None, 1.0, 0.0, l1, dz1, ws)
  if teacher:
    hip.ce_distill_fwd_bwd(z, torch.zeros_like(labels), z_t, tempr, w, l2, dz2, ws)
  # the one launch
  out = torch.full((4,), float('nan'), device='cuda')
  hard = torch.full_like(z, float('nan'))
  soft = torch.full_like(z, float('nan')) if teacher else None
  hip.ce_distill_head(z, labels, z_t if teacher else None, tempr if teacher else 1.0, w if teacher else 0.0, out, hard, soft,
                      torch.empty(3 * Bn, device='cuda'))
  assert torch.equal(out[0], l1[0]) and torch.equal(hard, dz1)
  if teacher:
    assert torch.equal(out[1], l2[1]) and torch.equal(soft, dz2)
  else:
    assert float(out[1]) == 0.0
  for k, got in ((1, out[2]), (5, out[3])):
    ref = losses.in_top_k(z, tgt, k).float().mean()
    assert torch.equal(got, ref), (k, float(got), float(ref))
  assert bool(losses.in_top_k(z, tgt, 1)[1]) and not bool(losses.in_top_k(z, tgt, 5)[2])      # the two prepared rows do their job
  # backward: upstream scalars 1 and other than 1, against the expression autograd evaluates for the two launches
  for g0v, g1v in ((1.0, 1.0), (0.75, -1.5)):
    g0, g1 = torch.tensor(g0v, device='cuda'), torch.tensor(g1v, device='cuda')
    ref = dz1 * g0.to(dtype)
    if teacher:
      ref = ref + dz2 * g1.to(dtype)
    got = torch.full_like(z, float('nan'))
    hip.ce_combine(hard, soft, g0, g1 if teacher else None, got)
    assert torch.equal(got, ref), (g0v, g1v)
  # ... and through the autograd functions of losses.py, switch off against switch on
  res = {}
  old = G.HEAD_FUSE
  try:
    for fuse in (False, True):
      G.HEAD_FUSE = fuse
      zz = z.clone().requires_grad_(True)
      if teacher:
        losses.prime_distillation(zz, z_t, tempr, w)
      ce = losses.softmax_cross_entropy(labels, zz)
      accs = losses.top_k_accuracies(labels, zz, (1, 5))
      total = 0.75 * ce
      dst = None
      if teacher:
        dst = losses.distillation_loss(zz, z_t, tempr, w)
        total = total + (-1.5) * dst
      total.backward()
      res[fuse] = (ce.detach(), dst.detach() if teacher else None, accs[0], accs[1], zz.grad)
  finally:
    G.HEAD_FUSE = old
  for a, b in zip(res[False], res[True]):
    assert (a is None and b is None) or torch.equal(a, b)


def test_a_training_step_is_unchanged_by_the_fused_head(tmp_path, monkeypatch):
  """ResNet-v2-50 at 64 x 64, batch 16, UQ w8/a8 + distillation, bf16 (the geometry of the 64 x 64 parity runs): two steps with
  PF_HEAD_FUSE off and on from the same checkpoint and batches.  Everything a step returns and updates must be EQUAL; a launch
  counter on the binding shows that the fused run made one loss launch per step and no apply / backward-statistics pass for the
  final BN.  (The pooled means are float32 sums in another order than aten's; with 2 x 2 pixels of 8-bit-quantised values both are
  exact, so no rounding tie separates the runs here.)"""
  from pocketflow_amd.flags import FLAGS
  import pocketflow_amd.learners.learner_utils  # noqa: F401  (defines flags)
  import pocketflow_amd.learners.abstract_learner  # noqa: F401
  import pocketflow_amd.datasets.abstract_dataset  # noqa: F401  (synthetic_pool)
  from pocketflow_amd import graph as G
  from pocketflow_amd import hip
  from pocketflow_amd.nets.resnet_at_ilsvrc12 import ModelHelper
  from pocketflow_amd.learners.uniform_quantization.learner import UniformQuantLearner
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  for k, v in dict(save_path=str(tmp_path / 'models' / 'model.ckpt'), save_path_eval=str(tmp_path / 'models_eval' / 'model.ckpt'),
                   synthetic_pool=2, batch_size=16, batch_size_eval=16, uql_weight_bits=8, uql_activation_bits=8, enbl_dst=True,
                   dst_eval_teacher=False, save_path_dst=str(tmp_path / 'models_dst' / 'model.ckpt'),
                   uql_save_quant_model_path=str(tmp_path / 'uql' / 'm.ckpt'), nb_eval_batches_override=1, resnet_size=50,
                   nb_classes=1001, image_size=64, uql_use_buckets=False, compute_dtype='bfloat16').items():
    setattr(FLAGS, k, v)
  # the initial values are not the subject: clipped normals instead of scipy's truncated-normal sampler (seconds per network)
  import scipy.stats
  monkeypatch.setattr(scipy.stats.truncnorm, 'rvs', lambda a, b, size=None, random_state=None:
                      np.clip(random_state.standard_normal(size), a, b))
  mh = ModelHelper()
  create_synthetic_checkpoint(mh)
  names = ('ce_distill_fwd_bwd', 'ce_distill_head', 'ce_combine', 'bn_act_quant_apply', 'bn_act_quant_pool', 'bn_bwd_stats',
           'bn_bwd_stats_pooled', 'bn_bwd_apply', 'bn_bwd_apply_pooled')
  steps = 2
  runs = {}
  calls = {}

  def counted(name, fn):
    def f(*a, **kw):
      calls[name] += 1
      return fn(*a, **kw)
    return f
  for n in names:
    monkeypatch.setattr(hip, n, counted(n, getattr(hip, n)))
  for fuse in (False, True):
    monkeypatch.setattr(G, 'HEAD_FUSE', fuse)
    learner = UniformQuantLearner(None, mh)
    calls.update(dict.fromkeys(names, 0))
    outs = [learner.train_step() for _ in range(steps)]
    torch.cuda.synchronize()
    st = learner.graph.store
    opt = getattr(learner.optimizer, 'opt', learner.optimizer)
    flat = {}
    for i, o in enumerate(outs):
      for k in ('dst_loss', 'model_loss', 'loss'):
        flat['step%d.%s' % (i, k)] = o[k].detach().float().cpu()
      for k, v in o['metrics'].items():
        flat['step%d.metrics.%s' % (i, k)] = v.detach().float().cpu()
      flat['step%d.lr' % i] = torch.tensor(float(o['lr']))
    flat.update(w_master=st.w_master.detach().cpu(), o_master=st.o_master.detach().cpu(), state=st.state.detach().cpu())
    for si, s in enumerate(list(opt.slots_w) + list(opt.slots_o)):
      flat['slot%d' % si] = s.detach().cpu()
    runs[fuse] = (flat, dict(calls))
    del learner
  (a, ca), (b, cb) = runs[False], runs[True]
  print('launches, switch off:', ca)
  print('launches, switch on: ', cb)
  assert sorted(a) == sorted(b)
  for k in a:
    assert torch.equal(a[k], b[k]), k
  # one loss launch (+ one combine) per step, none of the old ones; the old path: two launches per step, none of the new ones
  assert cb['ce_distill_head'] == steps and cb['ce_combine'] == steps and cb['ce_distill_fwd_bwd'] == 0
  assert ca['ce_distill_fwd_bwd'] == 2 * steps and ca['ce_distill_head'] == 0 and ca['ce_combine'] == 0
  # the final BN: student (every step) and teacher (every forward) pooled instead of applied; its backward in the pooled kernels
  assert ca['bn_act_quant_pool'] == 0 and cb['bn_act_quant_pool'] >= 2 * steps
  assert ca['bn_act_quant_apply'] - cb['bn_act_quant_apply'] == cb['bn_act_quant_pool']
  assert cb['bn_bwd_stats_pooled'] == steps == cb['bn_bwd_apply_pooled'] and ca['bn_bwd_stats_pooled'] == 0
  assert ca['bn_bwd_stats'] - cb['bn_bwd_stats'] == steps and ca['bn_bwd_apply'] - cb['bn_bwd_apply'] == steps
