"""Model helper for MobileNet-v1 / -v2 on ILSVRC-12 (reference nets/mobilenet_at_ilsvrc12.py:32-148):
loss = CE + loss_w_dcy * L2 over every trainable whose name lacks 'batch_normalization' -- which for
slim's `BatchNorm/*` names means ALL of them, BN gamma/beta and depthwise kernels included
(SURVEY A.6); v1: 100 epochs, LR x0.1 at 30/60/80/90; v2: 412 epochs, LR x 0.98^2.5 every 2.5 epochs (:127-132);
batch_size_norm 96, lrn_rate_init 0.045."""
import torch

from pocketflow_amd import losses
from pocketflow_amd.datasets.ilsvrc12_dataset import Ilsvrc12Dataset
from pocketflow_amd.flags import FLAGS, flags
from pocketflow_amd.graph import get_default_graph
from pocketflow_amd.nets.abstract_model_helper import AbstractModelHelper
from pocketflow_amd.utils.external import mobilenet_v1 as MobileNetV1
from pocketflow_amd.utils.external import mobilenet_v2 as MobileNetV2
from pocketflow_amd.utils.lrn_rate_utils import setup_lrn_rate_exponential_decay
from pocketflow_amd.utils.lrn_rate_utils import setup_lrn_rate_piecewise_constant
from pocketflow_amd.utils.multi_gpu_wrapper import MultiGpuWrapper as mgw

flags.DEFINE_integer('mobilenet_version', 1, 'MobileNet\'s version (1 or 2)')
flags.DEFINE_float('mobilenet_depth_mult', 1.0, 'MobileNet\'s depth multiplier')
flags.DEFINE_float('nb_epochs_rat', 1.0, '# of training epochs\'s ratio')
flags.DEFINE_float('lrn_rate_init', 0.045, 'initial learning rate')
flags.DEFINE_float('batch_size_norm', 96, 'normalization factor of batch size')
flags.DEFINE_float('momentum', 0.9, 'momentum coefficient')
flags.DEFINE_float('loss_w_dcy', 4e-5, 'weight decaying loss\'s coefficient')


def forward_fn(inputs, is_train):
  if FLAGS.mobilenet_version not in (1, 2):
    raise ValueError('invalid MobileNet version: {}'.format(FLAGS.mobilenet_version))
  graph = get_default_graph()
  net = graph.nets.get('mobilenet')
  if net is None:
    net_cls = MobileNetV1.MobilenetV1 if FLAGS.mobilenet_version == 1 else MobileNetV2.MobilenetV2
    net = graph.nets['mobilenet'] = net_cls(graph, num_classes=FLAGS.nb_classes, depth_multiplier=FLAGS.mobilenet_depth_mult)
  if inputs.device.type == 'meta':
    return torch.empty((inputs.shape[0], FLAGS.nb_classes), device='meta')
  return net(inputs, is_train)


class ModelHelper(AbstractModelHelper):
  """Model helper for creating a MobileNet model for the ILSVRC-12 dataset."""

  def __init__(self, data_format='channels_last'):
    assert data_format == 'channels_last', 'MobileNet only supports \'channels_last\' data format'
    super(ModelHelper, self).__init__(data_format)
    self.dataset_train = Ilsvrc12Dataset(is_train=True)
    self.dataset_eval = Ilsvrc12Dataset(is_train=False)

  def build_dataset_train(self, enbl_trn_val_split=False):
    return self.dataset_train.build(enbl_trn_val_split)

  def build_dataset_eval(self):
    return self.dataset_eval.build()

  def forward_train(self, inputs):
    return forward_fn(inputs, is_train=True)

  def forward_eval(self, inputs):
    return forward_fn(inputs, is_train=False)

  def calc_loss(self, labels, outputs, trainable_vars):
    loss = losses.softmax_cross_entropy(labels, outputs)
    loss_filter = lambda var: 'batch_normalization' not in var.name
    loss = loss + losses.l2_regularization(trainable_vars, loss_filter, FLAGS.loss_w_dcy)
    acc_top1, acc_top5 = losses.top_k_accuracies(labels, outputs, (1, 5))
    metrics = {'accuracy': acc_top5, 'acc_top1': acc_top1, 'acc_top5': acc_top5}
    return loss, metrics

  def setup_lrn_rate(self, global_step):
    batch_size = FLAGS.batch_size * (1 if not FLAGS.enbl_multi_gpu else mgw.size())
    if FLAGS.mobilenet_version == 1:
      nb_epochs = 100
      idxs_epoch = [30, 60, 80, 90]
      decay_rates = [1.0, 0.1, 0.01, 0.001, 0.0001]
      lrn_rate = setup_lrn_rate_piecewise_constant(global_step, batch_size, idxs_epoch, decay_rates)
    elif FLAGS.mobilenet_version == 2:
      nb_epochs = 412
      epoch_step = 2.5
      decay_rate = 0.98 ** epoch_step
      lrn_rate = setup_lrn_rate_exponential_decay(global_step, batch_size, epoch_step, decay_rate)
    else:
      raise ValueError('invalid MobileNet version: {}'.format(FLAGS.mobilenet_version))
    nb_iters = int(FLAGS.nb_smpls_train * nb_epochs * FLAGS.nb_epochs_rat / batch_size)
    return lrn_rate, nb_iters

  @property
  def model_name(self):
    return 'mobilenet_v%d' % FLAGS.mobilenet_version

  @property
  def dataset_name(self):
    return 'ilsvrc_12'
