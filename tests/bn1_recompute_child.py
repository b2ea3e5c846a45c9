"""Child process of tests/test_bn1_recompute_gpu.py: two seeded steps of the UQ learner (w8 / a8, distillation, bf16 fused path) on
ResNet-v2-50 at 64 x 64 with 16 images -- the size of the recorded-step tests with twice the images, so that stage 1 has the 4096
rows the resident 1x1 kernel takes and the two identity blocks there run whichever route PF_BN1_RECOMPUTE names.  Saves every
parameter, Adam slot and BN moving statistic, and how often the recomputing apply launch ran."""
import os
import pathlib
import tempfile

import torch


def run(out_path: str) -> None:
  from pocketflow_amd.flags import FLAGS
  import pocketflow_amd.learners.learner_utils  # noqa: F401  (defines flags)
  import pocketflow_amd.learners.abstract_learner  # noqa: F401
  import pocketflow_amd.datasets.abstract_dataset  # noqa: F401  (synthetic_pool)
  import pocketflow_amd.learners.distillation_helper  # noqa: F401
  from pocketflow_amd.nets.resnet_at_ilsvrc12 import ModelHelper
  from pocketflow_amd.learners.uniform_quantization.learner import UniformQuantLearner
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  import pocketflow_amd.graph as G

  tmp = pathlib.Path(tempfile.mkdtemp(dir=os.path.dirname(out_path)))
  for k, v in dict(save_path=str(tmp / 'models' / 'model.ckpt'), save_path_eval=str(tmp / 'models_eval' / 'model.ckpt'),
                   save_path_dst=str(tmp / 'models_dst' / 'model.ckpt'), uql_save_quant_model_path=str(tmp / 'uql' / 'm.ckpt'),
                   synthetic_pool=2, batch_size=16, batch_size_eval=16, uql_weight_bits=8, uql_activation_bits=8, enbl_dst=True,
                   dst_eval_teacher=False, resnet_size=50, nb_classes=1001, image_size=64, compute_dtype='bfloat16').items():
    setattr(FLAGS, k, v)
  launches = [0]
  entry = getattr(G.hip, 'conv1x1_bwd_data_bnapply')

  def counted(*a, **kw):
    launches[0] += 1
    return entry(*a, **kw)
  G.hip.conv1x1_bwd_data_bnapply = counted
  torch.manual_seed(0)
  mh = ModelHelper()
  create_synthetic_checkpoint(mh)
  learner = UniformQuantLearner(None, mh)
  for _ in range(2):
    out = learner.train_step()
  torch.cuda.synchronize()
  st = learner.graph.store
  params = {'w_master': st.w_master.cpu(), 'o_master': st.o_master.cpu(), 'state': st.state.cpu(),
            'loss': (out['loss'] if isinstance(out, dict) else out[1]).detach().float().cpu()}
  torch.save({'params': params, 'launches': launches[0]}, out_path)
