"""The pure host queries of the biased 5x5 'VALID' convolutions (pf_conv5v.hip): which shapes the kernels take and how many slabs the
backward-filter launch writes.  No device work: the library loads on the CPU."""
import itertools

import pytest

CN = [(3, 32), (3, 64), (32, 32), (32, 64)]
OK_SHAPES = [(H, Wd, C, N) for (H, Wd), (C, N) in itertools.product(((5, 5), (9, 14), (14, 14), (11, 21), (32, 32), (224, 64)), CN)]
# (H, Wd, C, N, k, stride, pad_h, pad_w): one thing wrong with each
NEAR_MISSES = [(14, 14, 32, 64, 3, 1, 0, 0), (14, 14, 32, 64, 5, 2, 0, 0), (14, 14, 32, 64, 5, 1, 2, 2), (14, 14, 32, 64, 5, 1, 0, 2),
               (14, 14, 32, 64, 5, 1, 2, 0), (14, 14, 16, 64, 5, 1, 0, 0), (14, 14, 64, 64, 5, 1, 0, 0), (14, 14, 32, 16, 5, 1, 0, 0),
               (14, 14, 32, 48, 5, 1, 0, 0), (14, 14, 32, 128, 5, 1, 0, 0), (4, 14, 32, 64, 5, 1, 0, 0), (14, 4, 32, 64, 5, 1, 0, 0),
               (14, 65, 32, 64, 5, 1, 0, 0), (32, 80, 3, 32, 5, 1, 0, 0)]


def _tiles(imgs, H, Wd):
  Ho, Wo = H - 4, Wd - 4
  per_img = -(-Ho // (128 // Wo))               # tiles of at most 128 pixels, whole output rows
  return imgs * per_img


@pytest.mark.parametrize('H,Wd,C,N', OK_SHAPES)
def test_supported_shapes_and_their_slabs(H, Wd, C, N):
  from pocketflow_amd import hip
  assert hip.conv5v_supported(H, Wd, C, N, 5, 1, 0, 0)
  for imgs in (1, 3, 128):
    S = hip.conv5v_wrw_slabs(imgs, H, Wd, C, N)
    operands = (imgs * H * Wd * C + imgs * (H - 4) * (Wd - 4) * N) * 2
    # one slab per persistent workgroup: never more than tiles or 256, and the slabs written stay below four times the operands read
    assert S == max(1, min(4 * operands // (N * 25 * C * 4), _tiles(imgs, H, Wd), 256))
  assert hip.conv5v_wrw_slabs(0, H, Wd, C, N) == 0 and hip.conv5v_wrw_slabs(-1, H, Wd, C, N) == 0


@pytest.mark.parametrize('H,Wd,C,N,k,stride,pad_h,pad_w', NEAR_MISSES)
def test_near_misses_are_refused(H, Wd, C, N, k, stride, pad_h, pad_w):
  from pocketflow_amd import hip
  assert not hip.conv5v_supported(H, Wd, C, N, k, stride, pad_h, pad_w)
  if (k, stride, pad_h, pad_w) == (5, 1, 0, 0):     # (the slabs query is asked of 5x5 / stride 1 / 'VALID' layers only)
    assert hip.conv5v_wrw_slabs(4, H, Wd, C, N) == 0


def test_lenet_layers_at_batch_128():
  from pocketflow_amd import hip
  assert hip.conv5v_wrw_slabs(128, 14, 14, 32, 64) == 63      # 3 244 032 bytes of operands, 204 800 a slab
  assert hip.conv5v_wrw_slabs(128, 32, 32, 3, 32) == 256       # 7.2 MB of operands, 9.4 KiB a slab: the cap


def test_byte_limit_of_the_31_bit_offsets():
  from pocketflow_amd import hip
  # the input, 64 x 64 x 32 channels = 2**18 bytes per image, reaches 2**31 first at 32 -> 32 ...
  assert hip.conv5v_wrw_slabs(8191, 64, 64, 32, 32) == 256 and hip.conv5v_wrw_slabs(8192, 64, 64, 32, 32) == 0
  # ... and the output, 60 x 60 x 64 channels = 460 800 bytes per image, at 3 -> 64
  assert hip.conv5v_wrw_slabs(4660, 64, 64, 3, 64) == 256 and hip.conv5v_wrw_slabs(4661, 64, 64, 3, 64) == 0
