"""The pure host queries of the dense kernels (pf_dense.hip): which shapes they take and in how many slabs the forward and the
backward-data launch sum their contraction.  No device work: the library loads on the CPU."""
import pytest

OK_SHAPES = [(1, 32, 1), (256, 2048, 1001), (260, 1600, 256), (128, 64, 10)]
# K = 0 | K % 32 != 0 | no rows | no columns | B * K * 2, N * K * 4 and B * N * 2 bytes at 2**31
REFUSED = [(4, 0, 10), (4, 48, 10), (0, 64, 10), (4, 64, 0), (1 << 15, 1 << 15, 1), (1, 1 << 14, 1 << 15), (1 << 15, 32, 1 << 15)]


@pytest.mark.parametrize('B,K,N', OK_SHAPES)
def test_supported_shapes_and_their_splits(B, K, N):
  from pocketflow_amd import hip
  assert hip.dense_supported(B, K, N)
  fwd, bwd = hip.dense_splits(B, K, N), hip.dense_splits(B, K, N, True)
  assert fwd >= 1 and (K // 32) % fwd == 0                          # whole k-steps per slab, all slabs alike
  assert 1 <= bwd <= -(-N // 32)                                     # whole n-steps per slab, none empty
  tiles = -(-N // 16) * -(-B // 256)
  assert tiles * fwd <= 512 or fwd == 1                              # two workgroups per CU at most


@pytest.mark.parametrize('B,K,N', REFUSED)
def test_refused_shapes_have_no_splits(B, K, N):
  from pocketflow_amd import hip
  assert not hip.dense_supported(B, K, N)
  assert hip.dense_splits(B, K, N) == 0 and hip.dense_splits(B, K, N, True) == 0


def test_the_resnet50_head_runs_split():
  from pocketflow_amd import hip
  assert hip.dense_splits(256, 2048, 1001) == 8 and hip.dense_splits(256, 2048, 1001, True) == 8
  assert hip.dense_splits(1, 32, 1) == 1 and hip.dense_splits(1, 32, 1, True) == 1
