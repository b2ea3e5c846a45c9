"""The host predicates of pf_stem3x.hip through the loaded library (no device work), as test_abi_host.py has them for the other stems."""
import pytest


def _out(size, stride, pad):
  return -(-size // stride) if pad == 0 else (size + 2 * pad - 3) // stride + 1


# (H, Wd, C, N, k, stride, front pads): the CIFAR stem | MobileNet 0.75 on an even image ('SAME': nothing in front) | the smallest map
TAKEN = [(32, 32, 3, 16, 3, 1, 1), (224, 224, 3, 24, 3, 2, 0), (1, 16, 3, 8, 3, 1, 1)]
# four channels | N % 8 | N > 64 | stride 3 | Wd < 16 and Wd % 8 | a 5x5 window
REFUSED = [(32, 32, 4, 16, 3, 1, 1), (32, 32, 3, 12, 3, 1, 1), (32, 32, 3, 72, 3, 1, 1), (32, 32, 3, 16, 3, 3, 1), (32, 12, 3, 16, 3, 1, 1),
           (32, 32, 3, 16, 5, 1, 1)]


@pytest.mark.parametrize('case', TAKEN + REFUSED)
def test_supported_and_slabs(case):
  from pocketflow_amd import hip
  H, Wd, C, N, k, stride, pad = case
  Ho, Wo = _out(H, stride, pad), _out(Wd, stride, pad)
  took = hip.conv_stem3x_supported(H, Wd, C, N, k, stride, pad, pad, Ho, Wo)
  assert took == (case in TAKEN)
  if took:
    assert hip.conv_stem3x_wrw_slabs(4, H, Wd, N, stride, pad, pad, Ho, Wo) > 0
    assert hip.conv_stem3x_wrw_slabs(0, H, Wd, N, stride, pad, pad, Ho, Wo) == 0
