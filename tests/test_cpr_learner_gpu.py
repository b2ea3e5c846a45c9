"""The 'chn-pruned-rmt' learner end to end on the GPU: selection (sampling, Gram, gamma search, least squares), warm start, masked
fine-tune, evaluation."""
import logging
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _setup(tmp_path, **kw):
  from pocketflow_amd.flags import FLAGS
  import pocketflow_amd.learners.learner_utils  # noqa: F401
  import pocketflow_amd.learners.abstract_learner  # noqa: F401
  import pocketflow_amd.learners.channel_pruning_rmt.learner  # noqa: F401
  import pocketflow_amd.datasets.abstract_dataset  # noqa: F401
  FLAGS.save_path = str(tmp_path / 'models' / 'model.ckpt')
  FLAGS.save_path_eval = str(tmp_path / 'models_eval' / 'model.ckpt')
  FLAGS.synthetic_pool = 2
  FLAGS.learner = 'chn-pruned-rmt'
  FLAGS.cpr_save_path = str(tmp_path / 'cpr' / 'model.ckpt')
  FLAGS.cpr_save_path_eval = str(tmp_path / 'cpr_eval' / 'model.ckpt')
  FLAGS.cpr_save_path_ws = str(tmp_path / 'cpr_ws' / 'model.ckpt')
  FLAGS.cpr_prune_ratio, FLAGS.cpr_skip_frst_layer, FLAGS.cpr_skip_last_layer, FLAGS.cpr_skip_op_names = 0.5, True, False, None
  FLAGS.cpr_nb_smpls, FLAGS.cpr_nb_crops_per_smpl = 48, 4
  FLAGS.cpr_ista_lrn_rate, FLAGS.cpr_ista_nb_iters, FLAGS.cpr_lstsq_lrn_rate, FLAGS.cpr_lstsq_nb_iters = 1e-2, 100, 1e-3, 20
  FLAGS.cpr_warm_start = False
  FLAGS.nb_iters_override, FLAGS.summ_step, FLAGS.nb_eval_batches_override = 3, 2, 2
  FLAGS.enbl_dst, FLAGS.compute_dtype = False, 'float32'
  for k, v in kw.items():
    setattr(FLAGS, k, v)
  return FLAGS


def _check_selection(lrn, ratios):
  for rec, ratio in zip(lrn.selection_log, ratios):
    cin = None
    for var in lrn.vars_prnd['maskable']:
      if var.name == rec['name']:
        cin = var.ref_shape[2]
    assert rec['target'] == int(cin * (1.0 - ratio))
    assert rec['nnz'] == rec['target'] or rec['path'][-1][1] == rec['nnz']      # reached, or the search ran out (logged)


def _run(FLAGS, mh, caplog):
  import torch
  from pocketflow_amd.learners.learner_utils import create_learner, create_synthetic_checkpoint
  from pocketflow_amd.learners.channel_pruning_rmt.learner import ChannelPrunedRmtLearner
  from pocketflow_amd.utils import checkpoint
  create_synthetic_checkpoint(mh)
  full_before = checkpoint.load(checkpoint.latest_checkpoint(os.path.dirname(FLAGS.save_path)))
  np.random.seed(7)
  lrn = create_learner(None, mh)
  assert isinstance(lrn, ChannelPrunedRmtLearner)
  with caplog.at_level(logging.INFO, logger='pocketflow_amd'):
    rslt = lrn.train()
  assert np.isfinite(rslt['loss'])
  full_after = checkpoint.load(checkpoint.latest_checkpoint(os.path.dirname(FLAGS.save_path)))
  for k, v in full_before.items():
    assert np.array_equal(v, full_after[k]), k
  vals = lrn.graph.store.export_numpy()
  for var in lrn.vars_prnd['maskable']:
    w = vals[var.name]
    dead = np.all(w == 0, axis=(0, 1, 3))
    m = var.to_ref(lrn.masks[var.offset:var.offset + var.numel].cpu().numpy())
    assert np.array_equal(np.all(m == 0, axis=(0, 1, 3)), dead)
  torch.cuda.synchronize()
  return lrn, rslt


def test_cpr_resnet20_select_finetune_and_warm_start(tmp_path, caplog):
  from pocketflow_amd.nets.resnet_at_cifar10 import ModelHelper
  FLAGS = _setup(tmp_path, batch_size=16, batch_size_eval=16, resnet_size=20, nb_classes=10)
  mh = ModelHelper()
  lrn, rslt = _run(FLAGS, mh, caplog)
  n = len(lrn.selection_log)
  assert n == len(lrn.vars_prnd['maskable']) >= 19
  ratios = [0.0] + [0.5] * (n - 1)
  _check_selection(lrn, ratios)
  nnz = [r['nnz'] for r in lrn.selection_log]
  assert sum(r['nnz'] == r['target'] for r in lrn.selection_log) >= n - 2, nnz
  assert 0.2 < rslt['pr_krn'] < 0.6
  from pocketflow_amd.utils import checkpoint
  ws_vals = checkpoint.load(checkpoint.latest_checkpoint(str(tmp_path / 'cpr_ws')))
  # warm start: no selection, same restored kernels
  FLAGS.cpr_warm_start = True
  from pocketflow_amd.learners.learner_utils import create_learner
  lrn2 = create_learner(None, mh)
  with caplog.at_level(logging.INFO, logger='pocketflow_amd'):
    caplog.clear()
    lrn2.train()
  assert lrn2.selection_log == [] and not any('layer #' in r.getMessage() for r in caplog.records)
  for var in lrn2.vars_prnd['maskable']:
    dead_ws = np.all(ws_vals[var.name] == 0, axis=(0, 1, 3))
    w = lrn2.graph.store.export_numpy()[var.name]
    assert np.array_equal(np.all(w == 0, axis=(0, 1, 3)) & dead_ws, dead_ws)     # pruned channels stay pruned


def test_cpr_mobilenet_skip_last_layer(tmp_path, caplog):
  import pocketflow_amd.nets.mobilenet_at_ilsvrc12  # noqa: F401
  from pocketflow_amd.nets.mobilenet_at_ilsvrc12 import ModelHelper
  FLAGS = _setup(tmp_path, batch_size=16, batch_size_eval=16, image_size=64, nb_classes=17, mobilenet_depth_mult=0.5,
                 cpr_skip_last_layer=True, cpr_nb_smpls=32)
  mh = ModelHelper()
  lrn, rslt = _run(FLAGS, mh, caplog)
  n = len(lrn.selection_log)
  assert n == len(lrn.vars_prnd['maskable']) and 'Logits' in lrn.selection_log[-1]['name']
  ratios = [0.0] + [0.5] * (n - 2) + [0.0]
  _check_selection(lrn, ratios)
  assert lrn.selection_log[-1]['target'] == lrn.vars_prnd['maskable'][-1].ref_shape[2]
