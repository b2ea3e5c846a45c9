"""Per-layer phase times of the 'chn-pruned-rmt' channel selection on ResNet-50 at 224 x 224 from a synthetic checkpoint:
sampling forwards, gather, Gram, gamma search (ISTA solves), least squares, with GFLOP/s of the Gram and least-squares steps against
the 157 TF float32 rate.  Default flags (5000 samples x 10 crops, 100 ISTA / Adam iterations).  The ISTA launch alone is timed with
_timing.gpu_time_us.

  python tools/gpu/cpr_select_timing.py --layers 4 [--nb_smpls 5000] > profiles/cpr_select_timing.txt
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--layers', type=int, default=4, help='number of Conv2D layers to select (graph order)')
  ap.add_argument('--nb_smpls', type=int, default=5000)
  ap.add_argument('--batch', type=int, default=64)
  args = ap.parse_args()
  import numpy as np
  import torch
  from _timing import gpu_time_us
  from pocketflow_amd import hip
  from pocketflow_amd.flags import FLAGS
  import pocketflow_amd.learners.learner_utils  # noqa: F401
  import pocketflow_amd.datasets.abstract_dataset  # noqa: F401
  import pocketflow_amd.learners.channel_pruning_rmt.learner as CPR
  from pocketflow_amd.nets.resnet_at_ilsvrc12 import ModelHelper
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  tmp = tempfile.mkdtemp()
  FLAGS.save_path = os.path.join(tmp, 'models', 'model.ckpt')
  FLAGS.save_path_eval = os.path.join(tmp, 'models_eval', 'model.ckpt')
  FLAGS.cpr_save_path_ws = os.path.join(tmp, 'ws', 'model.ckpt')
  FLAGS.synthetic_pool, FLAGS.batch_size, FLAGS.resnet_size, FLAGS.nb_classes = 2, args.batch, 50, 1001
  FLAGS.cpr_nb_smpls, FLAGS.enbl_dst, FLAGS.compute_dtype = args.nb_smpls, False, 'float32'
  mh = ModelHelper()
  create_synthetic_checkpoint(mh)
  np.random.seed(0)
  lrn = CPR.ChannelPrunedRmtLearner(None, mh)
  rows = []
  orig_lasso, orig_lstsq = CPR.LayerSelector.lasso, CPR.LayerSelector.lstsq

  def lasso(self, P, Y, idxs_rdc, w, kk, c_in, c_out, m0, target, log_fn=None):
    t0 = dict(self.timings)
    keep, path = orig_lasso(self, P, Y, idxs_rdc, w, kk, c_in, c_out, m0, target, log_fn)
    A = torch.rand(c_in * c_in, device='cuda')
    b, m, ws, out, nnz = (torch.rand(c_in, device='cuda'), torch.rand(c_in, device='cuda'), torch.empty(2 * c_in, device='cuda'),
                          torch.empty(c_in, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda'))
    solve_us = gpu_time_us(lambda: hip.cpr_ista(A, b, m, ws, out, 0.1, 1e-2, FLAGS.cpr_ista_nb_iters, nnz), n=5)
    rows.append({'c_in': c_in, 'c_out': c_out, 'kk': kk, 'rows_gram': len(idxs_rdc) * c_out, 'solves': len(path),
                 'gram_s': self.timings['gram'] - t0.get('gram', 0.0), 'ista_s': self.timings['ista'] - t0.get('ista', 0.0),
                 'ista_solve_gpu_us': solve_us,
                 'gram_gflop': 2.0 * len(idxs_rdc) * c_out * (c_in + 1) * (c_in + 2) / 2 / 1e9})
    return keep, path

  def lstsq(self, P, Y, N, w, kk, c_in, c_out, keep, wd):
    t0 = self.timings.get('lstsq', 0.0)
    out = orig_lstsq(self, P, Y, N, w, kk, c_in, c_out, keep, wd)
    kp = int(keep.sum()) * kk
    rows[-1].update({'N': N, 'kept': int(keep.sum()), 'lstsq_s': self.timings['lstsq'] - t0,
                     'lstsq_gflop': FLAGS.cpr_lstsq_nb_iters * 2 * 2.0 * N * kp * c_out / 1e9})
    return out

  CPR.LayerSelector.lasso, CPR.LayerSelector.lstsq = lasso, lstsq
  lrn._ChannelPrunedRmtLearner__build_prune()
  n_layers = len(lrn.core_prnd)
  lrn._ChannelPrunedRmtLearner__build_prune = lambda: None
  lrn.core_prnd, lrn.core_full = lrn.core_prnd[:args.layers], lrn.core_full[:args.layers]
  lrn.vars_sel['maskable'] = lrn.vars_sel['maskable'][:args.layers]
  lrn.vars_full['maskable'] = lrn.vars_full['maskable'][:args.layers]
  lrn._ChannelPrunedRmtLearner__choose_channels()
  print('# %d of %d Conv2D layers, %d samples x %d crops, batch %d' % (args.layers, n_layers, args.nb_smpls, FLAGS.cpr_nb_crops_per_smpl,
                                                                     args.batch))
  print('# totals (s): ' + json.dumps({k: round(v, 4) for k, v in lrn.selection_timings.items()}))
  for r in rows:
    r['gram_gflops'] = r['gram_gflop'] / max(r['gram_s'], 1e-9)
    r['lstsq_gflops'] = r['lstsq_gflop'] / max(r['lstsq_s'], 1e-9)
    r['lstsq_frac_of_157tf'] = r['lstsq_gflops'] / 157e3
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}))


if __name__ == '__main__':
  main()
