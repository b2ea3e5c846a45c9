"""The pure host queries of the narrow 3x3 convolutions (pf_conv3x3_narrow.hip): which shapes the kernels take and how many slabs
the backward-filter launch writes.  No device work: the library loads on the CPU."""
import itertools

import pytest

OK_SHAPES = [(H, Wd, C, N) for H, Wd in ((1, 16), (5, 16), (16, 16), (32, 32), (7, 48), (64, 64), (224, 64))
             for C, N in itertools.product((16, 32), repeat=2)]
# (H, Wd, C, N, stride, pad_h, pad_w): one thing wrong with each
NEAR_MISSES = [(32, 32, 16, 16, 2, 1, 1), (32, 32, 16, 16, 1, 0, 0), (32, 32, 16, 16, 1, 0, 1), (32, 32, 16, 16, 1, 1, 0),
               (32, 32, 16, 16, 1, 2, 2), (32, 32, 8, 16, 1, 1, 1), (32, 32, 48, 16, 1, 1, 1), (32, 32, 64, 32, 1, 1, 1),
               (32, 32, 16, 8, 1, 1, 1), (32, 32, 32, 48, 1, 1, 1), (32, 32, 32, 64, 1, 1, 1), (32, 8, 16, 16, 1, 1, 1),
               (32, 20, 16, 16, 1, 1, 1), (32, 80, 16, 16, 1, 1, 1), (0, 32, 16, 16, 1, 1, 1)]


@pytest.mark.parametrize('H,Wd,C,N', OK_SHAPES)
def test_supported_shapes_and_their_slabs(H, Wd, C, N):
  from pocketflow_amd import hip
  assert hip.conv3x3n_supported(H, Wd, C, N, 1, 1, 1)
  TR = 4 if Wd <= 32 else 2
  for imgs in (1, 3, 128):
    S = hip.conv3x3n_wrw_slabs(imgs, H, Wd, C, N)
    assert 1 <= S <= 1024
    assert S == min(imgs * -(-H // TR), 256)          # one slab per persistent workgroup, never more than tiles
  assert hip.conv3x3n_wrw_slabs(0, H, Wd, C, N) == 0 and hip.conv3x3n_wrw_slabs(-1, H, Wd, C, N) == 0


@pytest.mark.parametrize('H,Wd,C,N,stride,pad_h,pad_w', NEAR_MISSES)
def test_near_misses_are_refused(H, Wd, C, N, stride, pad_h, pad_w):
  from pocketflow_amd import hip
  assert not hip.conv3x3n_supported(H, Wd, C, N, stride, pad_h, pad_w)
  if (stride, pad_h, pad_w) == (1, 1, 1):           # (the slabs query is asked of 3x3 / stride 1 / pad 1 layers only)
    assert hip.conv3x3n_wrw_slabs(4, H, Wd, C, N) == 0


def test_byte_limit_of_the_31_bit_offsets():
  from pocketflow_amd import hip
  # imgs * H * Wd * max(C, N) * 2 < 2**31: 64 x 64 x 32 channels are 2**18 bytes per image
  assert hip.conv3x3n_wrw_slabs(8191, 64, 64, 16, 32) == 256 and hip.conv3x3n_wrw_slabs(8192, 64, 64, 16, 32) == 0
  assert hip.conv3x3n_wrw_slabs(8192, 64, 64, 16, 16) == 256 and hip.conv3x3n_wrw_slabs(16384, 64, 64, 16, 16) == 0
