"""Print what every host-side query of the convolution entries answers, over a fixed grid of shapes and tuning switches, for the
library named by PF_HIP_LIB (default: the one in the tree).  No GPU.  Two builds answer alike exactly when their outputs are equal:

    PF_HIP_LIB=/path/to/other/libpocketflow_hip.so python tools/conv_plan_sweep.py > a.txt
    python tools/conv_plan_sweep.py > b.txt && diff a.txt b.txt

Queries: pf_conv1x1_stats_groups_k (with and without prologue), pf_conv1x1_join_plan (with and without sums), pf_conv1x1_wrw_splits,
pf_conv2d_wrw_splits (1 and 9 taps) per GEMM shape (M, N, K); pf_conv2d_stats_groups_geom per convolution geometry.
Shapes: every convolution of ResNet-50 and MobileNet-v1 at batch 1, 32, 256; the shapes of the parametrize lists of
tests/test_conv_gpu.py, test_igemm_gpu.py, test_proj_join_gpu.py; a grid of M x N x K around the kernels' thresholds."""
import ast
import ctypes
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = [None, 'PF_CONV_STREAM=0', 'PF_CONV_IGEMM=0', 'PF_CONV_IGEMM_PRO=0', 'PF_IGEMM_PRO3=0', 'PF_IGEMM_TILE=256x128', 'PF_WRW2=0',
            'PF_WRW_TR=1', 'PF_CONV3X3_C64=0']
GRID_M = [130, 1000, 4095, 4096, 2 ** 17 - 1, 2 ** 17, 802816]
GRID_C = [64, 96, 128, 192, 256, 512, 1024, 2048]


def conv_out(H, k, stride, pad):
  return (H + 2 * pad - k) // stride + 1


def resnet50():
  """(H, W, C, N, k, stride, pad) of every convolution (utils/external/resnet_model.py, bottleneck v2, 224 x 224)."""
  convs = [(224, 224, 3, 64, 7, 2, 3)]
  H, C = 56, 64
  for f, blocks, stride in ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)):
    for b in range(blocks):
      s = stride if b == 0 else 1
      if b == 0:
        convs.append((H, H, C, 4 * f, 1, s, 0))                 # projection shortcut
      convs += [(H, H, C, f, 1, 1, 0), (H, H, f, f, 3, s, 1), (H // s, H // s, f, 4 * f, 1, 1, 0)]
      H, C = H // s, 4 * f
  return convs


def mobilenet_v1():
  """... of MobileNet-v1's dense convolutions (utils/external/mobilenet_v1.py): the stem and the pointwise layers."""
  convs = [(224, 224, 3, 32, 3, 2, 1)]
  H, C = 112, 32
  for N, stride in ((64, 1), (128, 2), (128, 1), (256, 2), (256, 1), (512, 2)) + ((512, 1),) * 5 + ((1024, 2), (1024, 1)):
    H //= stride                                                 # the depthwise layer in front carries the stride
    convs.append((H, H, C, N, 1, 1, 0))
    C = N
  return convs


class _Any:
  def __getattr__(self, name):
    return name


def test_shapes(path):
  """The argument dictionaries of every parametrized test of a test module (the product of its parametrize decorators)."""
  tree = ast.parse(open(path).read())
  ns = {'torch': _Any()}
  for node in tree.body:
    if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name):
      try:
        ns[node.targets[0].id] = eval(compile(ast.Expression(node.value), path, 'eval'), dict(ns))
      except NameError:                                          # an assignment that needs the module's imports: not a shape list
        pass
  out = []
  for node in tree.body:
    if not isinstance(node, ast.FunctionDef):
      continue
    axes = []
    for d in node.decorator_list:
      if isinstance(d, ast.Call) and getattr(d.func, 'attr', '') == 'parametrize':
        names = [n.strip() for n in ast.literal_eval(d.args[0]).split(',')]
        vals = eval(compile(ast.Expression(d.args[1]), path, 'eval'), dict(ns))
        axes.append([dict(zip(names, v if len(names) > 1 else (v,))) for v in vals])
    for combo in itertools.product(*axes) if axes else ():
      args = {}
      for c in combo:
        args.update(c)
      out.append(args)
  return out


def shapes():
  """-> (sorted GEMM shapes (M, N, K), sorted geometries (imgs, H, Wd, C, N, th, tw, stride, pad_h, pad_w, Ho, Wo))."""
  gemm, geom = set(), set()

  def add_conv(B, H, W, C, N, k, stride, pad):
    Ho, Wo = conv_out(H, k, stride, pad), conv_out(W, k, stride, pad)
    geom.add((B, H, W, C, N, k, k, stride, pad, pad, Ho, Wo))
    gemm.add((B * Ho * Wo, N, C))
    gemm.add((B * H * W, C, N) if stride == 1 else (B * Ho * Wo, C, N))       # backward-data reads the same product transposed

  for B in (1, 32, 256):
    for H, W, C, N, k, stride, pad in resnet50() + mobilenet_v1():
      add_conv(B, H, W, C, N, k, stride, pad)
  for name in ('test_conv_gpu.py', 'test_igemm_gpu.py', 'test_proj_join_gpu.py'):
    for a in test_shapes(os.path.join(ROOT, 'tests', name)):
      if 'shape' in a:
        a = dict(a, M=a['shape'][0], N=a['shape'][1], K=a['shape'][2])
      ints = {k: v for k, v in a.items() if isinstance(v, int)}
      N, K = ints.get('N'), ints.get('K', ints.get('C'))
      if N is None or K is None:                                 # (a test parametrized over something else than a convolution)
        continue
      if 'M' in ints:
        gemm.add((ints['M'], N, K))
        continue
      B = ints.get('B', ints.get('imgs', ints.get('n')))
      H = ints.get('H')
      if B is None or H is None:
        continue
      W = ints.get('W', ints.get('Wd', H))
      k, stride = ints.get('k', 3 if 'imgs' in ints else 1), ints.get('stride', 1)
      if 'plan' in ints:                                         # the joined backward-data: a 1x1 product over the dense grid
        gemm.add((B * H * W, N, K))
      else:
        add_conv(B, H, W, K, N, k, stride, ints.get('pad', k // 2))
  for M, N, K in itertools.product(GRID_M, GRID_C, GRID_C):
    gemm.add((M, N, K))
  return sorted(gemm), sorted(geom)


def main():
  path = os.environ.get('PF_HIP_LIB') or os.path.join(ROOT, 'pocketflow_amd', 'csrc', 'libpocketflow_hip.so')
  lib = ctypes.CDLL(path)
  gemm, geom = shapes()
  for setting in SETTINGS:
    key, val = setting.split('=') if setting else (None, None)
    old = os.environ.get(key) if key else None
    if key:
      os.environ[key] = val
    lib.pf_tuning_reload()
    try:
      tag = setting or 'default'
      for M, N, K in gemm:
        ans = [lib.pf_conv1x1_stats_groups_k(M, N, K, 0), lib.pf_conv1x1_stats_groups_k(M, N, K, 1), lib.pf_conv1x1_join_plan(M, N, K, 0),
               lib.pf_conv1x1_join_plan(M, N, K, 1), lib.pf_conv1x1_wrw_splits(M, N, K), lib.pf_conv2d_wrw_splits(M, N, K, 1),
               lib.pf_conv2d_wrw_splits(M, N, K, 9)]
        print('%s M=%d N=%d K=%d: G=%d G_pro=%d join=%d join_stats=%d wrw1x1=%d wrw2d_1=%d wrw2d_9=%d' % ((tag, M, N, K) + tuple(ans)))
      for g in geom:
        print('%s geom=%s: G=%d' % (tag, ','.join(map(str, g)), lib.pf_conv2d_stats_groups_geom(*g)))
    finally:
      if key:
        if old is None:
          del os.environ[key]
        else:
          os.environ[key] = old
      lib.pf_tuning_reload()
  return 0


if __name__ == '__main__':
  sys.exit(main())
