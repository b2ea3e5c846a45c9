"""Fused 1x1-convolution kernels (pf_conv1x1_fwd / pf_conv1x1_wrw) against float32 torch references
built from the SAME bf16 inputs; the prologue is checked against the stand-alone BN+ReLU+fake-quant
kernel (pf_bn_act_quant_apply), which is itself bit-exact against the oracle (test_kernels_gpu.py)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hip():
  from pocketflow_amd import hip as h
  return h


def _bf(x):
  return x.to(torch.bfloat16)


def _close_bf16(got, ref, frac_tol=0.0, what='', scale=None):
  """Equal up to one bf16 ulp of the reference (different fp32 accumulation order); `scale`: magnitude
  the ulp refers to when the reference is a sum of larger terms."""
  got, ref = got.float(), ref.float()
  err = (got - ref).abs()
  mag = ref.abs() if scale is None else torch.maximum(ref.abs(), scale.float().abs())
  tol = mag * 2 ** -7 + 1e-3
  bad = float((~(err <= tol)).float().mean())             # not `err > tol`: a NaN in the output compares false either way
  assert bad <= frac_tol, '%s: %.3e of the elements differ by more than a bf16 ulp (max err %.3e)' % (
      what, bad, float(err.max()))


# M >= 4096 with K, N in {64..512} and K * N <= 64 Ki: the resident-kernel variant (pf_conv_stream.hip) -- slice widths 64 /
# 128 / 256, one and two column slices, row tails that are not multiples of the 16 / 32-row strips
@pytest.mark.parametrize('M,N,K', [(1000, 64, 64), (3000, 128, 96), (777, 192, 256), (4096, 256, 64), (130, 512, 128),
                                   (5000, 64, 64), (4133, 256, 64), (4100, 128, 256), (6001, 512, 128), (4500, 128, 512),
                                   (9999, 64, 256), (70001, 256, 128)])
def test_conv1x1_fwd_plain_and_residual_and_stats(hip, M, N, K):
  g = torch.Generator(device='cuda').manual_seed(M + N + K)
  X = _bf(torch.randn(M, K, device='cuda', generator=g))
  W = _bf(torch.randn(N, K, device='cuda', generator=g) * 0.1)
  R = _bf(torch.randn(M, N, device='cuda', generator=g))
  Y = torch.empty(M, N, device='cuda', dtype=torch.bfloat16)
  hip.conv1x1_fwd(X, W, Y, M, N, K)
  ref = X.float() @ W.float().t()
  _close_bf16(Y, _bf(ref), what='plain')
  # residual + statistics
  G = hip.conv1x1_stats_groups(M, N, K)
  partial = torch.full((G, 4, N), float('nan'), device='cuda')
  Y2 = torch.empty_like(Y)
  hip.conv1x1_fwd(X, W, Y2, M, N, K, R=R, partial=partial)
  ref2 = _bf(ref + R.float())
  # the residual is added to the fp32 accumulators and the sum rounded ONCE; what remains is the accumulation order (a
  # value next to a rounding boundary lands one bf16 ulp away)
  _close_bf16(Y2, ref2, what='residual', scale=ref)
  y = Y2.float()
  assert not torch.isnan(partial).any()
  s, q = partial[:, 0].sum(0), partial[:, 1].sum(0)
  torch.testing.assert_close(s, y.sum(0), rtol=1e-4, atol=1e-2)
  torch.testing.assert_close(q, (y * y).sum(0), rtol=1e-4, atol=1e-2)
  assert torch.equal(partial[:, 2].min(0).values, y.min(0).values)
  assert torch.equal(partial[:, 3].max(0).values, y.max(0).values)


@pytest.mark.parametrize('shape', [(2500, 128, 192), (5000, 128, 256), (4444, 256, 128), (8200, 64, 512)])
@pytest.mark.parametrize('act,bits', [('Relu', 8), ('Relu6', 4), ('Relu', None), (None, None)])
def test_conv1x1_fwd_prologue_matches_standalone_bn_act_quant(hip, act, bits, shape):
  M, N, K = shape
  g = torch.Generator(device='cuda').manual_seed(7)
  X = _bf(torch.randn(M, K, device='cuda', generator=g) * 2)
  W = _bf(torch.randn(N, K, device='cuda', generator=g) * 0.1)
  ss = torch.stack([torch.rand(K, device='cuda', generator=g) + 0.5, torch.randn(K, device='cuda', generator=g)])
  slot = torch.empty(2, dtype=torch.int32, device='cuda')
  hip.minmax_slots_init(slot)
  Q = torch.empty_like(X)
  if bits is not None:
    # activation range of act(scale*x+shift), written the way pf_bn_finalize does (atomicMin on the slot)
    y = X.float() * ss[0] + ss[1]
    y = torch.relu(y) if act == 'Relu' else torch.clamp(y, 0, 6)
    hip.minmax_tensor(y.contiguous(), slot)
  hip.bn_act_quant_apply(X, Q, M, K, ss, act, slot if bits is not None else None, bits or 8, bits is not None)
  Y = torch.empty(M, N, device='cuda', dtype=torch.bfloat16)
  hip.conv1x1_fwd(X, W, Y, M, N, K, scale_shift=ss, act=act, slot=slot if bits is not None else None, bits=bits or 8)
  ref = _bf(Q.float() @ W.float().t())
  # the folded-constant fake-quant of the prologue may differ from the five-rounding chain on exact ties
  _close_bf16(Y, ref, frac_tol=2e-3 if bits is not None else 0.0, what='prologue %s/%s' % (act, bits))


# the three-stage prologue kernel of pf_igemm.hip (k_igemm<..,3,IG_PRO>;
# 128 x 256 tiles for N % 256 == 0, 256 x 128 for N % 128 == 0): deep contractions (up to the 2048 channels whose folded constants fill the LDS to its last byte), row tails,
# persistent workgroups that walk several row tiles, residual + statistics in the epilogue, and PF_IGEMM_PRO3=0 (round 2's
# two-stage kernel) on the same inputs -- the two must agree to the last bit (same prologue arithmetic, same k order)
@pytest.mark.parametrize('M,N,K', [(3000, 256, 1024), (5003, 512, 192), (2600, 128, 2048), (4133, 1024, 256), (40000, 256, 576),
                                   (1, 256, 64), (129, 128, 64), (36000, 128, 640), (100003, 256, 192), (70001, 512, 64)])
@pytest.mark.parametrize('act,bits', [('Relu', 8), ('Relu', None)])
def test_conv1x1_fwd_prologue_three_stage_kernel(hip, M, N, K, act, bits, monkeypatch):
  g = torch.Generator(device='cuda').manual_seed(M + N + K)
  X = _bf(torch.randn(M, K, device='cuda', generator=g) * 2)
  W = _bf(torch.randn(N, K, device='cuda', generator=g) * (K ** -0.5))
  R = _bf(torch.randn(M, N, device='cuda', generator=g))
  ss = torch.stack([torch.rand(K, device='cuda', generator=g) + 0.5, torch.randn(K, device='cuda', generator=g)])
  slot = torch.empty(2, dtype=torch.int32, device='cuda')
  hip.minmax_slots_init(slot)
  if bits is not None:
    y = torch.relu(X.float() * ss[0] + ss[1])
    hip.minmax_tensor(y.contiguous(), slot)
  sl = slot if bits is not None else None
  Q = torch.empty_like(X)
  hip.bn_act_quant_apply(X, Q, M, K, ss, act, sl, bits or 8, bits is not None)
  out = {}
  # '3': the three-stage kernel (the product), '2': round 2's two-stage kernel
  for mode, pro3 in (('3', '1'), ('2', '0')):
    monkeypatch.setenv('PF_IGEMM_PRO3', pro3)
    G = hip.conv1x1_stats_groups(M, N, K, prologue=True)
    partial = torch.full((G, 4, N), float('nan'), device='cuda')
    Y = torch.full((M, N), float('nan'), device='cuda', dtype=torch.bfloat16)
    hip.conv1x1_fwd(X, W, Y, M, N, K, R=R, scale_shift=ss, act=act, slot=sl, bits=bits or 8, partial=partial)
    out[mode] = (Y, partial)
  Y, partial = out['3']
  acc = Q.float() @ W.float().t()
  ref = _bf(acc + R.float())                                   # residual on the fp32 accumulators: one rounding
  _close_bf16(Y, ref, frac_tol=2e-3 if bits is not None else 0.0, what='3-stage prologue', scale=acc)
  y = Y.float()
  assert not torch.isnan(partial).any()
  torch.testing.assert_close(partial[:, 0].sum(0), y.sum(0), rtol=1e-4, atol=1e-2)
  torch.testing.assert_close(partial[:, 1].sum(0), (y * y).sum(0), rtol=1e-4, atol=1e-2)
  assert torch.equal(partial[:, 2].min(0).values, y.min(0).values)
  assert torch.equal(partial[:, 3].max(0).values, y.max(0).values)
  assert torch.equal(Y, out['2'][0]), 'the two prologue kernels differ'
  # race screen for the cross-tile prefetch of the three-stage kernel (the next tile's first stage lands in ring buffer 2 while
  # the epilogue of this one runs; workgroups walk up to 4 tiles at the larger sizes): repeated launches must agree to the bit
  monkeypatch.setenv('PF_IGEMM_PRO3', '1')
  for _ in range(4):
    Y2 = torch.full((M, N), float('nan'), device='cuda', dtype=torch.bfloat16)
    p2 = torch.full_like(out['3'][1], float('nan'))
    hip.conv1x1_fwd(X, W, Y2, M, N, K, R=R, scale_shift=ss, act=act, slot=sl, bits=bits or 8, partial=p2)
    assert torch.equal(Y2, out['3'][0]) and torch.equal(p2, out['3'][1])
  for mode in ('2',):                                          # and so do their statistics (different partial layouts, same sums)
    torch.testing.assert_close(out[mode][1][:, 0].sum(0), partial[:, 0].sum(0), rtol=1e-5, atol=1e-3)
    assert torch.equal(out[mode][1][:, 2].min(0).values, partial[:, 2].min(0).values)


# PF_CONV_STREAM_MAXSPLIT > 2: the resident-kernel variant with a row panel cut into 4 / 8 / 32 column slices (the conv3 layers
# of ResNet-50 stages 3-4, 256 -> 1024 and 512 -> 2048): prologue + residual + statistics, against the tiled kernels on the
# same inputs (equal up to the accumulation order)
@pytest.mark.parametrize('M,N,K', [(4133, 1024, 256), (6000, 2048, 512), (4500, 1024, 128), (9000, 512, 64)])
@pytest.mark.parametrize('act,bits', [('Relu', 8), ('Relu', None)])
def test_conv1x1_fwd_stream_many_column_slices(hip, M, N, K, act, bits, monkeypatch):
  g = torch.Generator(device='cuda').manual_seed(M + N + K)
  X = _bf(torch.randn(M, K, device='cuda', generator=g) * 2)
  W = _bf(torch.randn(N, K, device='cuda', generator=g) * (K ** -0.5))
  R = _bf(torch.randn(M, N, device='cuda', generator=g))
  ss = torch.stack([torch.rand(K, device='cuda', generator=g) + 0.5, torch.randn(K, device='cuda', generator=g)])
  slot = torch.empty(2, dtype=torch.int32, device='cuda')
  hip.minmax_slots_init(slot)
  if bits is not None:
    hip.minmax_tensor(torch.relu(X.float() * ss[0] + ss[1]).contiguous(), slot)
  sl = slot if bits is not None else None
  Q = torch.empty_like(X)
  hip.bn_act_quant_apply(X, Q, M, K, ss, act, sl, bits or 8, bits is not None)
  out = {}
  for split in ('32', '2'):
    monkeypatch.setenv('PF_CONV_STREAM_MAXSPLIT', split)
    G = hip.conv1x1_stats_groups(M, N, K, prologue=True)
    partial = torch.full((G, 4, N), float('nan'), device='cuda')
    Y = torch.full((M, N), float('nan'), device='cuda', dtype=torch.bfloat16)
    hip.conv1x1_fwd(X, W, Y, M, N, K, R=R, scale_shift=ss, act=act, slot=sl, bits=bits or 8, partial=partial)
    out[split] = (Y, partial, G)
  Y, partial, G = out['32']
  assert G != out['2'][2] or N <= 512, 'the many-slice plan was not taken'
  acc = Q.float() @ W.float().t()
  ref = _bf(acc + R.float())
  _close_bf16(Y, ref, frac_tol=2e-3 if bits is not None else 0.0, what='stream, many slices', scale=acc)
  _close_bf16(Y, out['2'][0], frac_tol=1e-5, what='stream vs tiled', scale=acc)
  y = Y.float()
  assert not torch.isnan(partial).any()
  torch.testing.assert_close(partial[:, 0].sum(0), y.sum(0), rtol=1e-4, atol=1e-2)
  torch.testing.assert_close(partial[:, 1].sum(0), (y * y).sum(0), rtol=1e-4, atol=1e-2)
  assert torch.equal(partial[:, 2].min(0).values, y.min(0).values)
  assert torch.equal(partial[:, 3].max(0).values, y.max(0).values)
  # plain + residual and the backward-data form (BN-backward sums) go through the same plan
  Y2 = torch.empty_like(Y)
  hip.conv1x1_fwd(X, W, Y2, M, N, K, R=R)
  _close_bf16(Y2, _bf(X.float() @ W.float().t() + R.float()), what='stream plain + residual', scale=acc)


# (K, N) = (256, 512), (192, 320): the row-mapped backward-data launch has a contraction of 512 / 320 channels and goes to the staged
# implicit GEMM with its row scatter (round 6; 128- and 64-wide column tiles); (64, 128): the register-staged tiles
@pytest.mark.parametrize('K,N', [(64, 128), (256, 512), (192, 320)])
@pytest.mark.parametrize('n,H,Wd', [(3, 14, 10), (9, 46, 50)])
def test_conv1x1_fwd_strided_and_ymap(hip, n, H, Wd, K, N):
  s = 2
  Ho, Wo = H // s, Wd // s
  g = torch.Generator(device='cuda').manual_seed(3)
  X = _bf(torch.randn(n, H, Wd, K, device='cuda', generator=g))
  W = _bf(torch.randn(N, K, device='cuda', generator=g) * 0.1)
  M = n * Ho * Wo
  Y = torch.empty(M, N, device='cuda', dtype=torch.bfloat16)
  hip.conv1x1_fwd(X, W, Y, M, N, K, geom=(Ho, Wo, H, Wd, s))
  ref = X[:, ::s, ::s, :].reshape(M, K).float() @ W.float().t()
  _close_bf16(Y, _bf(ref), what='strided')
  # backward-data of that conv: dX[img, ho*s, wo*s, :] = dY @ W, zero elsewhere
  dY = _bf(torch.randn(M, N, device='cuda', generator=g))
  Wt = W.t().contiguous()                      # [K][N] -> acts as the [N'][K'] weight of the NT kernel
  dX = torch.zeros(n, H, Wd, K, device='cuda', dtype=torch.bfloat16)
  hip.conv1x1_fwd(dY, Wt, dX, M, K, N, geom=(Ho, Wo, H, Wd, s), ymap=True)
  refd = torch.zeros(n, H, Wd, K, device='cuda')
  refd[:, ::s, ::s, :] = (dY.float() @ W.float()).reshape(n, Ho, Wo, K)
  _close_bf16(dX, _bf(refd), what='ymap')


# M >= 2048 with N, K multiples of 64: the transposed-LDS-read kernel (pf_wrw.hip); tile widths 64 / 128, pixel tails
@pytest.mark.parametrize('M,N,K,dw_dtype', [(1000, 64, 64, torch.float32), (5000, 128, 96, torch.bfloat16),
                                            (20000, 256, 64, torch.float32), (333, 192, 512, torch.float32),
                                            (4096, 64, 64, torch.float32), (10001, 128, 256, torch.bfloat16),
                                            (7777, 512, 128, torch.float32), (3000, 64, 128, torch.float32),
                                            (50176, 256, 1024, torch.float32),
                                            # few output channels over 256 / 512 input channels: the 64 x 256 and 128 x 256 tiles of round 6
                                            (30000, 64, 256, torch.float32), (8001, 128, 512, torch.bfloat16), (2100, 64, 512, torch.float32)])
@pytest.mark.parametrize('impl', ['shared-tile', 'scatter', 'wave-private'])
def test_conv1x1_wrw(hip, monkeypatch, M, N, K, dw_dtype, impl):
  # the three backward-filter kernels: shared-tile transposed reads (pf_wrw.hip k_wrw2, default where it applies), the
  # 2-byte-scatter kernel (pf_conv.hip, fallback), the wave-private transposed-read kernel (pf_wrw.hip k_wrw_tr, opt-in)
  monkeypatch.setenv('PF_WRW2', '1' if impl == 'shared-tile' else '0')
  monkeypatch.setenv('PF_WRW_TR', '1' if impl == 'wave-private' else '0')
  g = torch.Generator(device='cuda').manual_seed(M)
  X = _bf(torch.randn(M, K, device='cuda', generator=g))
  dY = _bf(torch.randn(M, N, device='cuda', generator=g) * 0.1)
  ss = torch.stack([torch.rand(K, device='cuda', generator=g) + 0.5, torch.randn(K, device='cuda', generator=g)])
  ws = torch.empty((hip.conv1x1_wrw_splits(M, N, K) + 32) * N * K, device='cuda')
  dW = torch.empty(N, K, device='cuda', dtype=dw_dtype)
  hip.conv1x1_wrw(dY, X, dW, ws, M, N, K)
  ref = dY.float().t() @ X.float()
  torch.testing.assert_close(dW.float(), ref, rtol=2e-2 if dw_dtype == torch.bfloat16 else 1e-3, atol=2e-2)
  # with the prologue: Q = relu(scale*x+shift), no quantisation
  Q = torch.empty_like(X)
  hip.bn_act_quant_apply(X, Q, M, K, ss, 'Relu', None, 8, False)
  hip.conv1x1_wrw(dY, X, dW, ws, M, N, K, scale_shift=ss, act='Relu')
  ref = dY.float().t() @ Q.float()
  torch.testing.assert_close(dW.float(), ref, rtol=2e-2 if dw_dtype == torch.bfloat16 else 1e-3, atol=2e-2)
  # with the quantising prologue: Q = fake_quant(relu(scale*x+shift)), 8 bits (ties may differ from the stand-alone kernel)
  slot = torch.empty(2, dtype=torch.int32, device='cuda')
  hip.minmax_slots_init(slot)
  hip.minmax_tensor(torch.relu(X.float() * ss[0] + ss[1]).contiguous(), slot)
  hip.bn_act_quant_apply(X, Q, M, K, ss, 'Relu', slot, 8, True)
  dWq = torch.empty_like(dW)
  hip.conv1x1_wrw(dY, X, dWq, ws, M, N, K, scale_shift=ss, act='Relu', slot=slot, bits=8)
  refq = dY.float().t() @ Q.float()
  torch.testing.assert_close(dWq.float(), refq, rtol=3e-2 if dw_dtype == torch.bfloat16 else 5e-3, atol=5e-2)
  # bit-reproducible (two-stage reduction, no atomics)
  dW2 = torch.empty_like(dW)
  hip.conv1x1_wrw(dY, X, dW2, ws, M, N, K, scale_shift=ss, act='Relu')
  assert torch.equal(dW, dW2)


@pytest.mark.parametrize('n,H,Wd,K,N', [(2, 8, 12, 64, 64), (10, 30, 34, 128, 192), (12, 28, 28, 256, 128)])
@pytest.mark.parametrize('impl', ['shared-tile', 'scatter', 'wave-private'])
def test_conv1x1_wrw_strided(hip, monkeypatch, n, H, Wd, K, N, impl):
  monkeypatch.setenv('PF_WRW2', '1' if impl == 'shared-tile' else '0')
  monkeypatch.setenv('PF_WRW_TR', '1' if impl == 'wave-private' else '0')
  s = 2
  Ho, Wo = H // s, Wd // s
  M = n * Ho * Wo
  g = torch.Generator(device='cuda').manual_seed(5)
  X = _bf(torch.randn(n, H, Wd, K, device='cuda', generator=g))
  dY = _bf(torch.randn(M, N, device='cuda', generator=g))
  ws = torch.empty((hip.conv1x1_wrw_splits(M, N, K) + 32) * N * K, device='cuda')
  dW = torch.empty(N, K, device='cuda')
  hip.conv1x1_wrw(dY, X, dW, ws, M, N, K, geom=(Ho, Wo, H, Wd, s))
  ref = dY.float().t() @ X[:, ::s, ::s, :].reshape(M, K).float()
  torch.testing.assert_close(dW, ref, rtol=1e-3, atol=2e-2)


def _r50_learner(tmp_path, fuse, tag, a_bits=8, dtype='bfloat16'):
  from pocketflow_amd.flags import FLAGS
  import pocketflow_amd.learners.learner_utils  # noqa: F401
  import pocketflow_amd.learners.abstract_learner  # noqa: F401
  import pocketflow_amd.learners.distillation_helper  # noqa: F401
  from pocketflow_amd.nets.resnet_at_ilsvrc12 import ModelHelper
  from pocketflow_amd.learners.uniform_quantization.learner import UniformQuantLearner
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  FLAGS.reset()
  d = tmp_path / tag
  FLAGS.save_path = str(tmp_path / 'models' / 'model.ckpt')          # shared: identical initial weights
  FLAGS.save_path_dst = str(d / 'models_dst' / 'model.ckpt')
  FLAGS.uql_save_quant_model_path = str(d / 'uql' / 'm.ckpt')
  FLAGS.synthetic_pool = 2
  FLAGS.compute_dtype = dtype
  FLAGS.resnet_size, FLAGS.nb_classes, FLAGS.image_size, FLAGS.batch_size = 50, 1001, 96, 16
  FLAGS.uql_weight_bits, FLAGS.uql_activation_bits = 8, a_bits
  FLAGS.enbl_dst, FLAGS.dst_eval_teacher = True, False
  FLAGS.fuse_conv1x1 = fuse
  mh = ModelHelper()
  create_synthetic_checkpoint(mh)
  return UniformQuantLearner(None, mh)


def _one_fwd_bwd(lrn):
  st, g = lrn.graph.store, lrn.graph
  images, labels = lrn.iter_train.get_next()
  x, y = lrn.to_device(images, labels)
  g.begin_step()
  lrn.uni_quant.quantize_weights()
  with g.as_default():
    logits_dst = lrn.helper_dst.calc_logits(None, x)
    logits = lrn.forward_train(x)
    loss, _ = lrn.calc_loss(y, logits, lrn.trainable_vars)
    loss = loss + lrn.helper_dst.calc_loss(logits, logits_dst)
  loss.backward()
  return dict(loss=float(loss.detach()), student=logits.detach().float().flatten().clone(),
              teacher=logits_dst.float().flatten().clone(), kernel_grads=st.w_grad.float().clone(),
              bn_grads=st.o_grad.float().clone(), bn_state=st.state.clone())


@pytest.mark.parametrize('a_bits', [32])      # (the 8-bit variant compared noise with noise -- cosines 0.08-0.15 -- and was dropped in round 4: the
#                                               conditioned-state oracle tests of tests/test_parity_gpu.py are the bar for 8-bit activations)
def test_fused_path_is_as_accurate_as_unfused(tmp_path, a_bits):
  """ResNet-50 (bottleneck blocks, strided projections) UQ w8 + distillation: one forward/backward in
  float32 (the parity-checked mode, MIOpen convolutions) is the ground truth; the bf16 run with every
  activation materialised (pf_bn_* + MIOpen) and the bf16 run with the BN/act/quant prologue and the
  residual/statistics epilogue fused into the 1x1 convolutions (pf_conv.hip) must agree with it EQUALLY
  well.  A deep randomly initialised BN network amplifies bf16 rounding noise layer by layer, so neither
  bf16 run reproduces the float32 gradients closely -- what is asserted is that fusion adds no error."""
  ref = _one_fwd_bwd(_r50_learner(tmp_path, False, 'fp32', a_bits, 'float32'))
  unf = _one_fwd_bwd(_r50_learner(tmp_path, False, 'bf16u', a_bits))
  fus = _one_fwd_bwd(_r50_learner(tmp_path, True, 'bf16f', a_bits))
  cos = lambda a, b: float(torch.dot(a.flatten(), b.flatten()) / (a.norm() * b.norm() + 1e-30))
  report = {}
  for k in ('teacher', 'student', 'kernel_grads', 'bn_grads', 'bn_state'):
    report[k] = (round(cos(unf[k], ref[k]), 4), round(cos(fus[k], ref[k]), 4))
  report['loss'] = (ref['loss'], unf['loss'], fus['loss'])
  report['grad_norm'] = (float(ref['kernel_grads'].norm()), float(unf['kernel_grads'].norm()),
                         float(fus['kernel_grads'].norm()))
  print('a_bits=%d (cos vs float32: unfused, fused): %s' % (a_bits, report))
  assert np.isfinite(fus['loss']) and abs(fus['loss'] - ref['loss']) <= 2e-2 * abs(ref['loss']), report
  assert report['teacher'][1] > 0.999 and report['bn_state'][1] > 0.999, report
  for k in ('student', 'kernel_grads', 'bn_grads'):
    u, f = report[k]
    # with 8-bit activations on a randomly initialised network NEITHER bf16 run correlates with float32 (cosines 0.08-0.15:
    # the quantiser's step functions amplify every rounding difference; measured spread between two correct runs +-0.07), so
    # the margin only means something where the cosines do; the conditioned-state comparison with the oracle
    # (tests/test_parity_gpu.py::test_uq_resnet50_bf16_fused_path_matches_oracle_within_bf16_noise) is the quantitative bar
    assert f >= u - (0.05 if u >= 0.5 else 0.15), (k, report)
  assert 0.7 < report['grad_norm'][2] / report['grad_norm'][0] < 1.4, report


@pytest.mark.parametrize('M,N,K', [(3000, 256, 128), (5003, 256, 64), (4800, 64, 256), (7000, 128, 512), (4097, 512, 128)])
def test_conv1x1_bwd_data_with_bn_backward_statistics(hip, M, N, K):
  """dQ = dY @ W with {sum dy, sum dy*xhat} of the producer BN in the epilogue == pf_bn_bwd_stats on (dQ, x)."""
  g = torch.Generator(device='cuda').manual_seed(11)
  dY = _bf(torch.randn(M, N, device='cuda', generator=g) * 0.1)
  W = _bf(torch.randn(N, K, device='cuda', generator=g) * 0.1)
  x = _bf(torch.randn(M, K, device='cuda', generator=g))
  ss = torch.stack([torch.rand(K, device='cuda', generator=g) + 0.5, torch.randn(K, device='cuda', generator=g) * 0.3])
  mi = torch.stack([torch.randn(K, device='cuda', generator=g) * 0.1, torch.rand(K, device='cuda', generator=g) + 0.5])
  Wt = W.t().contiguous()
  dQ = torch.empty(M, K, device='cuda', dtype=torch.bfloat16)
  G = hip.conv1x1_stats_groups(M, K, N)
  partial = torch.full((G, 2, K), float('nan'), device='cuda')
  hip.conv1x1_bwd_data_bnstats(dY, Wt, dQ, x, ss, mi, 'Relu', partial, M, N, K)
  _close_bf16(dQ, _bf(dY.float() @ W.float()), what='bwd-data')
  nblk = 32
  ref_partial = torch.empty(nblk * 2 * K, device='cuda')
  hip.bn_bwd_stats(dQ, x, M, K, ss, mi, 'Relu', ref_partial, nblk)
  dgamma, dbeta = torch.empty(K, device='cuda'), torch.empty(K, device='cuda')
  hip.bn_bwd_finalize(ref_partial, nblk, K, dgamma, dbeta)
  dg2, db2 = torch.empty(K, device='cuda'), torch.empty(K, device='cuda')
  hip.bn_bwd_finalize(partial, G, K, dg2, db2)
  torch.testing.assert_close(db2, dbeta, rtol=1e-4, atol=1e-3)
  torch.testing.assert_close(dg2, dgamma, rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize('M,C', [(4096, 64), (1000, 128), (5000, 256)])
@pytest.mark.parametrize('act,bits', [('Relu', 8), ('Relu6', 8), ('Relu', 4)])
def test_prologue_fake_quant_equals_oracle_except_enumerated_ties(hip, M, C, act, bits):
  """The prologue of the fused convolutions (bf16 throughput mode) computes the fake-quant with folded constants,
  q = rint((y - beta) * (k / alpha)) * (alpha / k) + beta with y = act(fma(scale, x, shift)), instead of the
  reference's five-rounding chain (uq utils.py:163-199: ((y - beta) / alpha) * k -> round -> / k -> * alpha -> + beta).
  Pinned here against the oracle's chain ELEMENT BY ELEMENT: a convolution with the identity kernel returns the
  prologue's bf16 output itself.  The two may differ only where the exact grid coordinate t = (y - beta) / alpha * k
  lies within a few float32 ulps of a rounding boundary n + 1/2 (there the folded product and the chain's division +
  product round to different sides); every differing element is checked to be such a near-tie AND to sit on one of the
  two neighbouring grid points.  Everywhere else the results are equal after the bf16 rounding both undergo."""
  from oracle import pf_oracle as O
  g = torch.Generator(device='cuda').manual_seed(M + C + bits)
  X = _bf(torch.randn(M, C, device='cuda', generator=g) * 2)
  ss = torch.stack([torch.rand(C, device='cuda', generator=g) + 0.5, torch.randn(C, device='cuda', generator=g)])
  eye = _bf(torch.eye(C, device='cuda'))
  u = (X.float() * ss[0] + ss[1]).contiguous()                 # the reference's BN output (mul, then add)
  slot = torch.empty(2, dtype=torch.int32, device='cuda')
  hip.minmax_slots_init(slot)
  hip.minmax_tensor(u, slot, act)                              # range of act(u), as pf_bn_finalize leaves it
  Y = torch.empty(M, C, device='cuda', dtype=torch.bfloat16)
  hip.conv1x1_fwd(X, eye, Y, M, C, C, scale_shift=ss, act=act, slot=slot, bits=bits)
  got = Y.float().cpu().numpy()
  ref32, _ = O.activation_quantize(u.cpu().numpy(), bits, act)
  ref = torch.from_numpy(ref32).to(torch.bfloat16).float().numpy()
  diff = got != ref
  # exact grid coordinate of every element (float64)
  y = u.cpu().numpy().astype(np.float64)
  y = np.maximum(y, 0.0) if act == 'Relu' else np.clip(y, 0.0, 6.0)
  beta, alpha = float(y.min()), float(y.max() - y.min()) + 1e-10
  k = float(2 ** bits - 1)
  t = (y - beta) / alpha * k
  dist = np.abs(t - (np.floor(t) + 0.5))                       # distance to the nearest rounding boundary
  # a few float32 ulps of the TERMS of t: round 3 contracts the BN affine and the quantiser affine into one fma,
  # t = fma(scale * k/alpha, x, (shift - beta) * k/alpha), whose rounding error scales with |scale * x| * k/alpha, not with t
  mag = np.abs(X.float().cpu().numpy().astype(np.float64) * ss[0].cpu().numpy()) + np.abs(ss[1].cpu().numpy()) + abs(float(y.min()))
  near = dist <= 8 * np.spacing(np.float32(k)) + 2e-6 * k + 6e-7 * mag / alpha * k
  # second (tiny) class: the float32 results of the two chains differ in their last bits (alpha * (r / k) + beta vs
  # fma(r, alpha / k, beta)), which shows after the bf16 rounding only if the float32 value sits within a few ulps
  # of a bf16 rounding boundary (low 16 bits ~ 0x8000): then the stored values are adjacent bf16 numbers
  low = ref32.view(np.uint32) & 0xFFFF
  near16 = np.abs(low.astype(np.int64) - 0x8000) <= 8
  bad = diff & ~near & ~near16
  assert not np.any(bad), '%d elements differ away from a rounding boundary' % int(np.sum(bad))
  step = alpha / k
  d_grid, d_16 = diff & near, diff & ~near & near16
  assert np.all(np.abs(got[d_grid] - ref[d_grid]) <= step * 1.02 + np.abs(ref[d_grid]) * 2 ** -7)   # neighbouring grid point
  assert np.all(np.abs(got[d_16] - ref[d_16]) <= np.abs(ref[d_16]) * 2 ** -7 + 1e-30)               # adjacent bf16 number
  assert near.mean() < 2e-3                                    # grid ties are rare
  # (near16 is a property of the <= 2^bits distinct grid VALUES, not of the elements: a grid value whose float32 image sits
  # next to a bf16 boundary is shared by many elements; what is asserted above is that nothing ELSE differs)
  assert d_16.sum() <= near16.sum()
  print('prologue vs oracle: %d grid ties, %d bf16 ties of %d elements' % (int(d_grid.sum()), int(d_16.sum()), diff.size))


# M >= 4096 with small K * N: resident-kernel variant; deep K with a prologue: three-stage prologue kernel; K >= 512 without one: plain
# implicit GEMM; K = 96 / a strided launch: no kernel carries the folded pass -> plain launch + stand-alone pass in place
@pytest.mark.parametrize('M,N,K,pro,stride', [(20000, 64, 256, True, 1), (9000, 256, 64, True, 1), (5000, 128, 256, False, 1),
                                              (9000, 256, 1024, True, 1), (4133, 128, 2048, True, 1), (6000, 256, 512, False, 1),
                                              (3000, 128, 96, True, 1), (4096, 128, 256, True, 2), (70001, 64, 64, True, 1)])
@pytest.mark.parametrize('out_act', ['Relu', 'Relu6', None])
def test_conv1x1_fwd_with_the_consumers_inference_bn_in_the_epilogue(hip, M, N, K, pro, stride, out_act):
  """pf_conv1x1_fwd_affine (round 6): the consumer's inference-mode BN + activation applied in the row pass of the epilogue ==
  pf_conv1x1_fwd followed by pf_bn_act_quant_apply(quantize = 0) on the stored output, BIT FOR BIT (the pass reads the bf16 value
  the stand-alone kernel would read)."""
  g = torch.Generator(device='cuda').manual_seed(M + N + K)
  if stride == 1:
    X, geom, Mo = _bf(torch.randn(M, K, device='cuda', generator=g) * 2), None, M
  else:
    n, H = 4, 32
    X = _bf(torch.randn(n, H, H, K, device='cuda', generator=g) * 2)
    Mo = n * (H // stride) ** 2
    geom = (H // stride, H // stride, H, H, stride)
  W = _bf(torch.randn(N, K, device='cuda', generator=g) * (K ** -0.5))
  ss = torch.stack([torch.rand(K, device='cuda', generator=g) + 0.5, torch.randn(K, device='cuda', generator=g)]) if pro else None
  oss = torch.stack([torch.rand(N, device='cuda', generator=g) + 0.5, torch.randn(N, device='cuda', generator=g)])
  Y0 = torch.empty(Mo, N, device='cuda', dtype=torch.bfloat16)
  hip.conv1x1_fwd(X, W, Y0, Mo, N, K, scale_shift=ss, act='Relu' if pro else None, geom=geom)
  ref = torch.empty_like(Y0)
  hip.bn_act_quant_apply(Y0, ref, Mo, N, oss, out_act, None, 8, False)
  Y1 = torch.full_like(Y0, float('nan'))
  hip.conv1x1_fwd(X, W, Y1, Mo, N, K, scale_shift=ss, act='Relu' if pro else None, geom=geom, out_scale_shift=oss, out_act=out_act)
  assert torch.equal(Y1, ref), 'folded pass differs in %d elements' % int((Y1 != ref).sum())
