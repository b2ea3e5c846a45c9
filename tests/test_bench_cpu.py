"""bench.py's control flow end to end WITHOUT a GPU: the HIP entry points are replaced by the float32 emulations of
tests/fake_hip.py and the few torch.cuda calls bench.py makes are stubbed, so that every line of `main()` runs -- argument
handling, learner construction, warm-up, the self-diagnosis of --full (here forced into its host-bound branch), the timed region and
the JSON line with every key of the driver's contract.  (What it measures is meaningless; the GPU runs measure.)"""
import json
import sys

import torch

from fake_hip import FakeHipFull


import pytest


@pytest.mark.parametrize('config,extra', [('c2', []), ('c2a32', []), ('c1', []), ('c4', ['--resnet_size', '18']),
                                          ('c3', ['--image_size', '64'])])
def test_bench_main_runs_end_to_end_on_emulated_kernels(monkeypatch, capsys, tmp_path, config, extra):
  import pocketflow_amd.graph as G
  import pocketflow_amd.learners.channel_pruning.learner as CP
  import pocketflow_amd.plan as P
  import pocketflow_amd.losses as L
  import pocketflow_amd.optim as Opt
  import pocketflow_amd.profiling as PR
  import pocketflow_amd.learners.abstract_learner as AL
  import pocketflow_amd.learners.nonuniform_quantization.utils as NU
  import pocketflow_amd.learners.weight_sparsification.learner as WS
  import pocketflow_amd.learners.layerwise as LW
  import bench
  fake = FakeHipFull()
  for mod in (G, P, L, Opt, WS, NU, LW, CP):
    monkeypatch.setattr(mod, 'hip', fake)
  monkeypatch.setattr(AL, 'require_gpu', lambda: torch.device('cpu'))
  monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
  # pretend the process is host-bound: the diagnostic branch (one more step under cProfile) must work when it is needed
  monkeypatch.setattr(bench, 'launch_probe', lambda torch, n=1000: {'host_us_per_launch': 1.0, 'us_per_dispatch': 99.0})
  monkeypatch.setattr(bench, 'memory_snapshot', lambda torch: {'reserved_gb': 0.0, 'segments_allocated': 0})
  monkeypatch.setattr(PR, 'enable', lambda name: None)
  monkeypatch.setattr(PR, 'summary', lambda name, lo=0, hi=None, side=None: (72, 7.2, 72 * 3.0e8))
  monkeypatch.setenv('TMPDIR', str(tmp_path))
  monkeypatch.setattr(sys, 'argv', ['bench.py', '--config', config, '--steps', '1', '--warmup', '1', '--batch', '2',
                                    '--image_size', '32', '--dtype', 'float32', '--full', '--no_cpu_baseline'] + extra)
  from pocketflow_amd.flags import FLAGS
  try:
    bench.main()
  finally:
    FLAGS.reset()
  out, err = capsys.readouterr()
  line = json.loads([ln for ln in out.splitlines() if ln.startswith('{')][-1])
  for key in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
              'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
    assert key in line, key
  assert line['n_gpus'] == 1 and line['steps'] == 1 and line['warmup'] == 1 and line['scaling'] == 'weak'
  assert line['higher_is_better'] is True and line['vs_baseline'] is None and line['data'] == 'synthetic'
  assert line['unit'] == 'images/s' and line['value'] > 0 and 'workload' in line['config'] and 'model' not in line['config']
  assert line['config']['name'] == config
  want = {'c2': 'UniformQuantLearner w8/a8', 'c2a32': 'w8/a32', 'c1': 'WeightSparseLearner', 'c3': 'ChannelPrunedLearner',
          'c4': 'NonUniformQuantLearner 4-bit'}[config]
  assert want in line['config']['workload'], line['config']['workload']
  r = line['roofline']
  # headline: the MFMA roofline north_star names (whole-step FLOPs / step time / dense bf16 peak); the HBM-bound region measured launch
  # by launch is a sub-block, the figure with the chip to itself first
  assert r['bound'] == 'mfma' and r['unit'] == 'TFLOP/s' and abs(r['frac'] - r['achieved'] / r['peak']) < 1e-9 and r['traffic'] is None
  assert abs(r['frac'] - r['step_mfma_frac']) < 1e-12 and abs(r['achieved'] * 1e12 - line['value'] * bench.CONFIGS[config]['flops']) < 1e-3 * r['achieved'] * 1e12
  h = r['hbm_region']
  assert h['bound'] == 'hbm' and h['unit'] == 'GB/s' and list(h)[-2:] == ['unshared', 'shared'] and h['shared']['launches'] == 72
  assert abs(h['shared']['frac'] - h['shared']['achieved'] / h['peak']) < 1e-9
  assert line['launch_probe']['after_warmup']['us_per_dispatch'] == 99.0 and 'memory' in line
  assert 'host-bound process' in err and 'tottime' in err          # the self-diagnosis printed its profile


@pytest.mark.parametrize('config', ['c1', 'c2', 'c2a32', 'c3', 'c4'])
def test_bench_flag_setup_in_a_fresh_interpreter(config, tmp_path):
  """bench.py assigns reference flags that only exist once the module defining them was imported; in a fresh process
  (how the driver runs it) nothing else has imported them.  (Round 3, GPU call 2: `Unknown command line flag
  'enbl_multi_gpu'` -- the in-process test above had passed because other tests' imports had defined the flag.)"""
  import os
  import subprocess
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  code = ('import sys; sys.argv = ["bench.py", "--config", %r]; sys.path.insert(0, %r); import bench; '
          'a = bench.parse_args(); mh, ln = bench.set_flags(a, %r, 1); '
          'from pocketflow_amd.flags import FLAGS; print("OK", mh.__name__, ln.__name__, FLAGS.batch_size, FLAGS.enbl_multi_gpu)'
          % (config, root, str(tmp_path)))
  out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
  assert out.returncode == 0 and 'OK ModelHelper' in out.stdout, out.stderr[-2000:]


def _emulated_bench(monkeypatch, tmp_path, argv):
  """bench.main() on the emulated kernels of tests/fake_hip.py (as above); returns the number of train_step calls."""
  import pocketflow_amd.graph as G
  import pocketflow_amd.learners.channel_pruning.learner as CP
  import pocketflow_amd.plan as P
  import pocketflow_amd.losses as L
  import pocketflow_amd.optim as Opt
  import pocketflow_amd.profiling as PR
  import pocketflow_amd.learners.abstract_learner as AL
  import pocketflow_amd.learners.nonuniform_quantization.utils as NU
  import pocketflow_amd.learners.weight_sparsification.learner as WS
  import pocketflow_amd.learners.layerwise as LW
  import bench
  fake = FakeHipFull()
  for mod in (G, P, L, Opt, WS, NU, LW, CP):
    monkeypatch.setattr(mod, 'hip', fake)
  monkeypatch.setattr(AL, 'require_gpu', lambda: torch.device('cpu'))
  monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
  monkeypatch.setattr(bench, 'launch_probe', lambda torch, n=1000: {'host_us_per_launch': 1.0, 'us_per_dispatch': 1.0})
  monkeypatch.setattr(bench, 'memory_snapshot', lambda torch: {'reserved_gb': 0.0, 'segments_allocated': 0})
  monkeypatch.setattr(PR, 'enable', lambda name: None)
  monkeypatch.setattr(PR, 'summary', lambda name, lo=0, hi=None, side=None: (72, 7.2, 72 * 3.0e8))
  monkeypatch.setenv('TMPDIR', str(tmp_path))
  calls = [0]
  build = bench.build_learner

  def counting_build(*a, **k):
    learner, step = build(*a, **k)

    def counted():
      calls[0] += 1
      return step()
    return learner, counted
  monkeypatch.setattr(bench, 'build_learner', counting_build)
  monkeypatch.setattr(sys, 'argv', ['bench.py'] + argv)
  from pocketflow_amd.flags import FLAGS
  try:
    bench.main()
  finally:
    FLAGS.reset()
  return calls[0]


def test_bench_dump_outputs_do_not_depend_on_the_untimed_steps(monkeypatch, capsys, tmp_path):
  """--dump-outputs DIR writes the last timed step's outputs as float32 / float64 .npy files (64 MiB at most), and the learner
  state the timed steps start from does not depend on how many untimed steps the step-mode decision and --full took: a --full
  run that tries to record the step (--step_graph default: two sampled steps, the recording attempt, the self-diagnosis) dumps the
  same arrays as a plain one that runs launch by launch from the start (--step_graph 0).  --steps sets the number of timed steps."""
  import numpy as np
  import bench
  base = ['--config', 'c1', '--batch', '2', '--dtype', 'float32', '--no_cpu_baseline', '--warmup', '1',
          '--unshared_steps', '0']
  monkeypatch.setattr(bench, 'MAX_UNTIMED_STEPS', 12)     # (enough for the emulated runs, where no recording succeeds)
  runs = []
  for steps, mode in ((2, ['--full']), (2, ['--step_graph', '0']), (3, ['--step_graph', '0'])):
    d = tmp_path / ('dump_%d_%d' % (steps, len(mode)))
    n = _emulated_bench(monkeypatch, tmp_path, base + mode + ['--steps', str(steps), '--dump-outputs', str(d)])
    out, err = capsys.readouterr()
    line = json.loads([ln for ln in out.splitlines() if ln.startswith('{')][-1])
    assert line['steps'] == steps and line['ms_per_step'] > 0
    assert ('step graph not recorded' in err) == ('--step_graph' not in mode)
    assert n == 1 + bench.MAX_UNTIMED_STEPS + 2 * steps, n      # warm-up and untimed steps up to the fixed count, K-step backlog, K timed
    files = sorted(p.name for p in d.iterdir())
    assert files == sorted(name + '.npy' for name in line['dumped_outputs'])
    arrays = {f[:-4]: np.load(str(d / f)) for f in files}
    assert {'out.1', 'out.2.accuracy', 'params.weights', 'params.others'} <= set(arrays), sorted(arrays)   # (lr, loss, metrics)
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    runs.append(arrays)
  assert runs[0].keys() == runs[1].keys()
  for name in runs[0]:
    assert np.array_equal(runs[0][name], runs[1][name]), name
  # one more timed step: the outputs are those of a later step
  assert not np.array_equal(runs[1]['params.weights'], runs[2]['params.weights'])


@pytest.mark.parametrize('full', [False, True])
def test_bench_plain_run_does_only_what_the_headline_needs(monkeypatch, capsys, tmp_path, full):
  """A plain run makes the warm-up, backlog and timed steps and nothing else: no host-share sample, no self-diagnosis, no
  roofline.unshared steps, no launch probes, no CPU baseline.  --full runs all of them (the CPU baseline's child process is
  stood in for)."""
  import subprocess
  import bench
  started = []

  def fake_run(cmd, **kw):
    started.append(cmd)
    return subprocess.CompletedProcess(cmd, 0, stdout='CPU_BASELINE {"value": 1.5}\n', stderr='')
  monkeypatch.setattr(subprocess, 'run', fake_run)
  monkeypatch.setenv('PF_TEACHER_AHEAD', 'inline')           # (the teacher helper the roofline.unshared steps need)
  argv = ['--config', 'c2', '--resnet_size', '18', '--batch', '2', '--image_size', '32', '--dtype', 'float32',
          '--warmup', '1', '--steps', '2'] + (['--full'] if full else [])
  n = _emulated_bench(monkeypatch, tmp_path, argv)
  out, err = capsys.readouterr()
  line = json.loads([ln for ln in out.splitlines() if ln.startswith('{')][-1])
  assert line['steps'] == 2 and line['ms_per_step'] > 0 and line['value'] > 0
  unshared = line['roofline']['hbm_region']['unshared']
  share = line['config']['host_share_of_two_launch_by_launch_steps']
  if not full:
    assert n == 1 + 2 * 2, n                                  # warm-up, K-step backlog (no step is recorded here), K timed
    assert started == [] and line['cpu_baseline'] is None and unshared is None and share is None
    assert line['launch_probe'] is None and line['memory'] is None and 'host-bound process' not in err
    return
  profiled = 1 if 'host-bound process' in err else 0
  assert n == 1 + 2 + 2 + profiled + 2 * 2 + 1 + 2, n        # + host-share sample, self-diagnosis, hand-over and roofline.unshared
  assert share is not None
  assert len(started) == 1 and 'time_cpu_baseline' in started[0][-1] and line['cpu_baseline'] == {'value': 1.5}
  assert unshared['steps'] == 2 and line['launch_probe']['after_timed_region'] is not None
  assert line['memory']['after_warmup'] is not None
