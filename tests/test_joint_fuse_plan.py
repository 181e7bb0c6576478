"""The joint rescale + ReLU fusion rule and its runtime knob (csrc/hip/launch.h joint_fuse): host arithmetic only.

The planner defers a joint rescale's outputs to the ReLU's fused output kernel when ``hip_joint_fuse_pick(N, B)``
holds (mode -1, auto) or when the mode forces it (0 off, 1 on). The rule is ``B <= 2`` (latency batches) or a staged
shape (N % 16 == 0, N >= 256) with ``B * N`` at least ``hip_joint_fuse_min_elems()``. The threshold is an absolute
element count above 6192, because tests/test_gpu_launch_forms.py pins the two-kernel path for B = 3, N <= 2064
under every planning CU count. (The kernels behind the knob are tested on the GPU: test_gpu_joint_fused.py.)"""
import pytest

INT64_MAX = (1 << 63) - 1


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("N", [1, 144, 256, 1031, 2064, 57600])
def test_latency_batches_always_fuse(native, N, B):
    assert native.hip_joint_fuse_pick(N, B) is True


@pytest.mark.parametrize("N", [144, 256, 512, 528, 1031, 1040, 2064])
def test_batch3_small_layers_keep_two_kernels(native, N):
    assert native.hip_joint_fuse_pick(N, 3) is False


@pytest.mark.parametrize("B", [3, 24, 55, 165])
@pytest.mark.parametrize("N", [1031, 57601, 57608, (1 << 20) + 8])
def test_unstaged_shapes_never_fuse_above_batch2(native, N, B):
    assert N % 16 != 0
    assert native.hip_joint_fuse_pick(N, B) is False


def test_threshold_is_an_absolute_count(native):
    T = native.hip_joint_fuse_min_elems()
    assert T > 3 * 2064
    base = [native.hip_joint_fuse_pick(N, B) for N, B in [(57600, 55), (2064, 3), (576, 55)]]
    for count in (1, 1 << 20):
        native.hip_set_planning_cus(count)
        try:
            assert [native.hip_joint_fuse_pick(N, B) for N, B in [(57600, 55), (2064, 3), (576, 55)]] == base
        finally:
            native.hip_set_planning_cus(0)
    if T < INT64_MAX:  # the default is flipped for throughput batches: the headline's first layer takes the fusion
        assert native.hip_joint_fuse_pick(57600, 55) is True
        N = (T + 2) // 3 + 15
        N -= N % 16  # the first staged N with 3 N >= T
        assert native.hip_joint_fuse_pick(max(N, 256), 3) is True
        assert native.hip_joint_fuse_pick(max(N, 256) + 1, 3) is False
    else:  # not flipped: no batch above 2 takes it
        assert native.hip_joint_fuse_pick(57600, 55) is False
        assert native.hip_joint_fuse_pick(1 << 30, 165) is False


def test_mode_round_trips_and_restores(native):
    base = native.hip_joint_fuse()
    assert base in (-1, 0, 1)
    try:
        for mode in (1, 0, -1):
            native.hip_set_joint_fuse(mode)
            assert native.hip_joint_fuse() == mode
        # the mode does not change the rule itself
        native.hip_set_joint_fuse(0)
        assert native.hip_joint_fuse_pick(512, 1) is True
        native.hip_set_joint_fuse(1)
        assert native.hip_joint_fuse_pick(2064, 3) is False
        for bad in (-2, 2):
            with pytest.raises(Exception, match="mode must be"):
                native.hip_set_joint_fuse(bad)
        assert native.hip_joint_fuse() == 1
    finally:
        native.hip_set_joint_fuse(base)
    assert native.hip_joint_fuse() == base
