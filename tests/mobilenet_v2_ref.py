"""MobileNet-v2 restated for the tests, independent of pocketflow_amd: the variable list in slim's creation order and a forward pass
in plain torch functional ops at any dtype (float64: the yardstick; float32: the bar of a float32 run).

Derived by READING the reference (utils/external/mobilenet_v2.py V2_DEF, conv_blocks.py expanded_conv / _make_divisible,
mobilenet.py depth_multiplier / the Logits head / training_scope) and the paper's table 2 (t, c, n, s), which V2_DEF spells out op by
op.  Used by tests/test_mobilenet_v2_cpu.py and tests/test_mobilenet_v2_gpu.py; run as a script it writes the fixture
tests/golden/mobilenet_v2_vars.json (names, shapes and creation order at multipliers 1.0 and 0.5, 1001 classes)."""
import numpy as np
import torch
import torch.nn.functional as F

# (expansion t, channels c, repeats n, first stride s): arXiv 1801.04381 table 2
TABLE = [(1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1)]
BN_EPS = 1e-3
BN_LEAVES = ('beta', 'gamma', 'moving_mean', 'moving_variance')      # slim.batch_norm's creation order


def make_divisible(v, divisor, min_value=None):
  min_value = divisor if min_value is None else min_value
  new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
  return new_v + divisor if new_v < 0.9 * v else new_v


def blocks(mult):
  """[(scope, cin, inner, cout, stride, has_expand, residual)] and the stem / last widths."""
  depth = lambda d: make_divisible(d * mult, 8, 8)
  stem, out, cin, k = depth(32), [], depth(32), 0
  for t, c, n, s in TABLE:
    for i in range(n):
      stride = s if i == 0 else 1
      cout = depth(c)
      inner = cin if t == 1 else make_divisible(cin * t, 8)       # expand_input(1, divisible_by=1) / expand_input(6)
      out.append(('expanded_conv' if k == 0 else 'expanded_conv_%d' % k, cin, inner, cout, stride, inner > cin, stride == 1 and cin == cout))
      cin, k = cout, k + 1
  return stem, out, depth(1280)


def var_list(mult, num_classes, scope='MobilenetV2'):
  """[[name, shape]] in creation order: weights, then the BatchNorm's four; expand, depthwise, project inside a block."""
  stem, blks, last = blocks(mult)
  out = []

  def conv(name, shape, leaf='weights'):
    out.append(['%s/%s/%s' % (scope, name, leaf), list(shape)])
    out.extend(['%s/%s/BatchNorm/%s' % (scope, name, l), [shape[2] if leaf == 'depthwise_weights' else shape[3]]] for l in BN_LEAVES)
  conv('Conv', (3, 3, 3, stem))
  for name, cin, inner, cout, stride, has_expand, residual in blks:
    if has_expand:
      conv(name + '/expand', (1, 1, cin, inner))
    conv(name + '/depthwise', (3, 3, inner, 1), 'depthwise_weights')
    conv(name + '/project', (1, 1, inner, cout))
  conv('Conv_1', (1, 1, blks[-1][3], last))
  out.append(['%s/Logits/Conv2d_1c_1x1/weights' % scope, [1, 1, last, num_classes]])
  out.append(['%s/Logits/Conv2d_1c_1x1/biases' % scope, [num_classes]])
  return out


def _same(x, k, stride):
  pads = []
  for size in (x.shape[3], x.shape[2]):            # F.pad: last dimension first
    out = -(-size // stride)
    total = max((out - 1) * stride + k - size, 0)
    pads += [total // 2, total - total // 2]
  return F.pad(x, pads)


def forward(vals, images, mult, training, dtype=torch.float64, prefix='model/MobilenetV2', mask=None, device='cpu', fold=False,
            channels_last=False, raw_depthwise_of=None):
  """Logits [B][classes] in `dtype` of NCHW `images`; vals: {name: array in the reference layout}.  `training`: batch statistics
  (biased variance) and, with `mask` [B][features] (already divided by keep), dropout; else the moving statistics.  `fold` and
  `channels_last` change the ORDER of operations only (BN as x * scale + (beta - mean * scale) with the variance from the two raw
  moments; convolutions over NHWC memory): other float32 evaluations of the same function.  `raw_depthwise_of`: return, instead of
  the logits, the depthwise output of the block of that index BEFORE its BatchNorm."""
  t = lambda name: torch.as_tensor(np.asarray(vals[prefix + '/' + name]), dtype=dtype, device=device)
  stem, blks, last = blocks(mult)

  def bn(x, name, act):
    p = name + '/BatchNorm/'
    if training and fold:
      mean = x.mean(dim=(0, 2, 3))
      var = torch.clamp((x * x).mean(dim=(0, 2, 3)) - mean * mean, min=0.0)
    elif training:
      mean, var = x.mean(dim=(0, 2, 3)), x.var(dim=(0, 2, 3), unbiased=False)
    else:
      mean, var = t(p + 'moving_mean'), t(p + 'moving_variance')
    scale = t(p + 'gamma') * torch.rsqrt(var + BN_EPS)
    if fold:
      y = x * scale.view(1, -1, 1, 1) + (t(p + 'beta') - mean * scale).view(1, -1, 1, 1)
    else:
      y = (x - mean.view(1, -1, 1, 1)) * scale.view(1, -1, 1, 1) + t(p + 'beta').view(1, -1, 1, 1)
    return torch.clamp(y, 0.0, 6.0) if act else y

  def conv(x, name, stride=1):
    w = t(name + '/weights').permute(3, 2, 0, 1)                  # HWIO -> OIHW
    return F.conv2d(_same(x, w.shape[2], stride), w, stride=stride)

  def depthwise(x, name, stride):
    w = t(name + '/depthwise_weights').permute(2, 3, 0, 1)        # [kh][kw][C][1] -> [C][1][kh][kw]
    return F.conv2d(_same(x, 3, stride), w, stride=stride, groups=x.shape[1])
  x = torch.as_tensor(np.asarray(images), dtype=dtype, device=device)
  if channels_last:
    x = x.contiguous(memory_format=torch.channels_last)
  x = bn(conv(x, 'Conv', 2), 'Conv', True)
  for index, (name, cin, inner, cout, stride, has_expand, residual) in enumerate(blks):
    y = x
    if has_expand:
      y = bn(conv(y, name + '/expand'), name + '/expand', True)
    y = depthwise(y, name + '/depthwise', stride)
    if index == raw_depthwise_of:
      return y
    y = bn(y, name + '/depthwise', True)
    y = bn(conv(y, name + '/project'), name + '/project', False)
    x = x + y if residual else y
  x = bn(conv(x, 'Conv_1'), 'Conv_1', True)
  x = x.mean(dim=(2, 3))
  if training and mask is not None:
    x = x * torch.as_tensor(np.asarray(mask), dtype=dtype, device=device)
  w = t('Logits/Conv2d_1c_1x1/weights')[0, 0]                     # [in][out]
  return x @ w + t('Logits/Conv2d_1c_1x1/biases')


def write_fixture(path):
  import json
  out = {'scope': 'MobilenetV2', 'num_classes': 1001, 'multipliers': {}}
  for mult in (1.0, 0.5):
    vs = var_list(mult, 1001)
    trainable = sum(int(np.prod(s)) for n, s in vs if not n.rsplit('/', 1)[1].startswith('moving_'))
    out['multipliers']['%.1f' % mult] = {'vars': vs, 'trainable_parameters': trainable}
  with open(path, 'w') as f:
    json.dump(out, f, indent=0, separators=(',', ':'))
    f.write('\n')
  return {k: (len(v['vars']), v['trainable_parameters']) for k, v in out['multipliers'].items()}


if __name__ == '__main__':
  import os
  print(write_fixture(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mobilenet_v2_vars.json')))
