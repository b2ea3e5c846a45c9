"""Host queries of the kernels that take any channel count C % 8 == 0 up to 2048 (no device work: the library answers on the host):
pf_depthwise_supported / pf_depthwise_groups (pf_depthwise.hip) and pf_bn_vector_ok (the (row, 8-channel) vector map of the
BatchNorm / quantiser passes), which graph._bn_fast_ok hands on."""
import pytest


@pytest.fixture(scope='module')
def hip():
  from pocketflow_amd import hip as h
  return h


def test_depthwise_takes_every_multiple_of_eight_channels(hip):
  for C in range(8, 2049, 8):
    for stride in (1, 2):
      assert hip.depthwise_supported(C, 3, stride), (C, stride)


def test_depthwise_still_refuses_what_the_lane_map_cannot_hold(hip):
  for C in list(range(1, 8)) + [12, 20, 36, 100, 1001, 2047]:
    assert C % 8 != 0 and not hip.depthwise_supported(C, 3, 1), C
  for C in (0, 2056):
    for stride in (1, 2):
      assert not hip.depthwise_supported(C, 3, stride), (C, stride)
  for C in (32, 96):
    assert not hip.depthwise_supported(C, 5, 1) and not hip.depthwise_supported(C, 3, 3)


@pytest.mark.parametrize('B,Ho,Wo,C', [(3, 15, 13, 24), (2, 8, 10, 48), (256, 56, 56, 96), (2, 14, 14, 144), (256, 14, 14, 384),
                                       (3, 7, 7, 768), (2, 7, 7, 960), (1, 3, 2, 1032), (1, 6, 6, 2040), (4, 64, 344, 96),
                                       (256, 112, 112, 32), (5, 7, 7, 1024), (1, 1, 1, 2048)])
def test_depthwise_groups_round_the_strips_per_workgroup_down(hip, B, Ho, Wo, C):
  spb = 256 // (C // 8)                                   # strips a workgroup covers per pass: the left-over lanes idle
  strips = B * Ho * -(-Wo // 4)
  assert hip.depthwise_groups(B, Ho, Wo, C) == min(1024, -(-strips // spb))


def test_bn_vector_ok_is_what_the_graph_plans_with(hip):
  from pocketflow_amd import graph
  for C in range(1, 2100):
    want = C % 8 == 0 and C <= 2048
    assert hip.bn_vector_ok(C) == graph._bn_fast_ok(C) == want, C
  for C in (24, 96, 144, 576, 960, 2040):
    assert hip.bn_vector_ok(C), C
  assert not hip.bn_vector_ok(0) and not hip.bn_vector_ok(-8)


def test_bn_blocks_keep_the_plan_of_the_powers_of_two():
  """The row splits of the statistics passes where the channel groups fill whole slabs are what they were; a guarded last slab
  counts as a slab."""
  from pocketflow_amd import graph
  for C, cg in ((8, 1), (16, 2), (32, 4), (64, 8), (256, 8), (2048, 8)):
    nslab = C // (cg * 8)
    for rows in (1, 777, 256 * 56 * 56):
      assert graph._bn_blocks(rows, C) == max(1, min(256 // nslab, rows // ((1024 // cg) * 2))), (rows, C)
  assert graph._bn_blocks(1 << 30, 24) == 256             # 3 groups in one slab of 4
  assert graph._bn_blocks(1 << 30, 96) == 128             # 12 groups: 2 slabs of 8, the second half empty
  assert graph._bn_blocks(1 << 30, 2040) == 8             # 255 groups: 32 slabs
  assert graph._bn_blocks(1 << 30, 10) == 256             # scalar route
