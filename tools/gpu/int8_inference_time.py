"""Whole-model inference time of an exported quantised model on the three routes of inference.load_int8: a synthetic ResNet-50
checkpoint goes through the UniformQuantLearner (8-bit weights in channel buckets, 8-bit activations) and
tools/conversion/export_quant_int8_model.py, then tools/benchmark/calc_inference_time runs on the artefact with --int8 off | auto | on,
B = 256 / 224 x 224, bf16, in ROUNDS alternating rounds inside one process.  Prints every run and, per route, the median and the
spread (max - min) over the rounds.  NET=mobilenet does the same for MobileNet-v1 1.0 with the routes --int8 off, --int8 on,
--int8 on --int8_depthwise on (the depthwise layers on pf_dw_i8_fwd as well) and --int8 auto --int8_depthwise auto (what
graph.int8_pays and graph.int8_dw_pays accept).

STATIC=1 times FIXED activation ranges instead: the artefact is calibrated over two evaluation batches (calibrate_act_ranges) and the
routes are the parent's two (--act_ranges batch with --int8 off, and with the best per-batch setting: --int8 auto, for MobileNet plus
--int8_depthwise auto) and the static ones (--act_ranges static with --int8 off, --int8 on, for MobileNet --int8 on --int8_depthwise on, and
--int8 auto --int8_depthwise auto: what graph.int8_pays_static and graph.int8_dw_pays_static accept).

  python tools/gpu/int8_inference_time.py > profiles/int8_inference_time.txt
  NET=mobilenet python tools/gpu/int8_inference_time.py > profiles/int8_mobilenet_inference_time.txt
  (NET=mobilenet STATIC=1 python tools/gpu/int8_inference_time.py; STATIC=1 python tools/gpu/int8_inference_time.py) \
      > profiles/int8_static_inference_time.txt
"""
import io
import json
import os
import sys
import tempfile
from contextlib import redirect_stdout

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch

B = int(os.environ.get('B', 256))
IMAGE = int(os.environ.get('IMAGE', 224))
ROUNDS = int(os.environ.get('ROUNDS', 3))
REPTS = int(os.environ.get('REPTS', 20))
NET = os.environ.get('NET', 'resnet50')
STATIC = os.environ.get('STATIC', '0') == '1'


def main():
  from pocketflow_amd.flags import FLAGS
  if NET == 'mobilenet':
    import pocketflow_amd.nets.mobilenet_at_ilsvrc12 as net
  else:
    import pocketflow_amd.nets.resnet_at_ilsvrc12 as net
  from pocketflow_amd.learners.learner_utils import create_synthetic_checkpoint
  from pocketflow_amd.learners.uniform_quantization.learner import UniformQuantLearner
  from pocketflow_amd.tools.benchmark import calc_inference_time as T
  from pocketflow_amd.tools.conversion import export_quant_int8_model as E
  from pocketflow_amd.utils import checkpoint
  with tempfile.TemporaryDirectory() as tmp:
    FLAGS.save_path = os.path.join(tmp, 'models', 'model.ckpt')
    FLAGS.uql_save_quant_model_path = os.path.join(tmp, 'uql', 'model.ckpt')
    FLAGS.nb_classes, FLAGS.image_size, FLAGS.batch_size = 1001, IMAGE, 8
    if NET == 'mobilenet':
      FLAGS.mobilenet_version, FLAGS.mobilenet_depth_mult = 1, 1.0
      net_args, title = ['--net', 'mobilenet_at_ilsvrc12', '--mobilenet_depth_mult', '1.0'], 'MobileNet-v1 1.0'
      routes = [('off', ['--int8', 'off']), ('on', ['--int8', 'on', '--int8_depthwise', 'off']),
                ('on+dw', ['--int8', 'on', '--int8_depthwise', 'on']), ('auto+dw', ['--int8', 'auto', '--int8_depthwise', 'auto'])]
    else:
      FLAGS.resnet_size = 50
      net_args, title = ['--net', 'resnet_at_ilsvrc12', '--resnet_size', '50'], 'ResNet-50'
      routes = [(mode, ['--int8', mode]) for mode in ('off', 'auto', 'on')]
    if STATIC:
      # (ResNet-50 has no depthwise layer: --int8_depthwise on would be the 'static on' row again)
      best = ['--int8', 'auto', '--int8_depthwise', 'auto' if NET == 'mobilenet' else 'off']
      routes = [('off', ['--act_ranges', 'batch', '--int8', 'off', '--int8_depthwise', 'off']),
                ('batch best', ['--act_ranges', 'batch'] + best),
                ('static off', ['--act_ranges', 'static', '--int8', 'off', '--int8_depthwise', 'off']),
                ('static on', ['--act_ranges', 'static', '--int8', 'on', '--int8_depthwise', 'off']),
                ] + ([('static on+dw', ['--act_ranges', 'static', '--int8', 'on', '--int8_depthwise', 'on'])] if NET == 'mobilenet' else []) + [
                ('static auto', ['--act_ranges', 'static', '--int8', 'auto', '--int8_depthwise', 'auto'])]
    else:
      routes = [(mode, args + ['--act_ranges', 'batch']) for mode, args in routes]
    FLAGS.compute_dtype, FLAGS.synthetic_pool = 'bfloat16', 2
    FLAGS.uql_weight_bits = FLAGS.uql_activation_bits = 8
    FLAGS.uql_use_buckets, FLAGS.uql_bucket_type = True, 'channel'
    mh = net.ModelHelper()
    create_synthetic_checkpoint(mh)
    learner = UniformQuantLearner(None, mh)
    learner.restore_vars(checkpoint.latest_checkpoint(os.path.dirname(FLAGS.save_path)))
    path = os.path.join(tmp, 'uql', 'model_int8.npz')
    E.export_from_learner(learner, path)
    del learner
    torch.cuda.empty_cache()
    if STATIC:
      E.calibrate_act_ranges(mh, path, 2, 8, 'cuda', torch.bfloat16)
      torch.cuda.empty_cache()
    common = net_args + ['--nb_classes', '1001', '--image_size', str(IMAGE), '--batch_size', str(B),
              '--compute_dtype', 'bfloat16', '--nb_repts_warmup', '5', '--nb_repts', str(REPTS), '--json', '--model_file', path,
              '--uql_activation_bits', '8']
    print('# %s, B = %d, %d x %d, bf16, w8 (channel buckets) / a8; %d passes per run after 5 warm-up passes; %d alternating rounds'
          % (title, B, IMAGE, IMAGE, REPTS, ROUNDS))
    ms = {mode: [] for mode, _ in routes}
    for rnd in range(ROUNDS):
      for mode, args in routes:
        buf = io.StringIO()
        with redirect_stdout(buf):
          T.main(common + args)
        line = json.loads([ln for ln in buf.getvalue().splitlines() if ln.startswith('{')][-1])
        ms[mode].append(line['ms_per_batch'])
        print('round %d  --int8 %-12s  %9.3f ms per batch  nb_int8_layers %3d (%d ran, %d requantising)'
              % (rnd, mode, line['ms_per_batch'], line['nb_int8_layers'], line['nb_int8_layers_ran'], line['nb_requant_layers']))
        torch.cuda.empty_cache()
    for mode, _ in routes:
      v = sorted(ms[mode])
      print('--int8 %-12s  median %9.3f ms  spread %7.3f ms  (off / this %.3f)'
            % (mode, v[len(v) // 2], v[-1] - v[0], sorted(ms['off'])[len(v) // 2] / v[len(v) // 2]))


if __name__ == '__main__':
  main()
