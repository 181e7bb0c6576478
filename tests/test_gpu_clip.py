"""The Clip layer on the GPU: the HIP evaluator (both sign constructions, both forms of the clip multiply)
bit-exact against the host evaluator, the GPU garbler byte-identical to the host garbler, the MobileNet-style
circuit end to end and the range guard's torch path on the device (docs/CLIP.md)."""
import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit, RangeGuard
from tests.test_clip import M7, clip_inputs, dense_clip_dense, guard_case, tiny_mobilenet
from tests.test_gpu_parity import _check, _gpu_vs_host

pytestmark = pytest.mark.gpu


def _labels_equal(cpu, gpu):
    for c, g in zip(cpu, gpu):
        assert len(c) == len(g)
        for (pc, ac), (pg, ag) in zip(c, g):
            assert pc == pg
            np.testing.assert_array_equal(ac, ag)


def _run_clip(N, lo, hi, crt, mrs, relu, xs, plain=True, log=None):
    """Two GCs (different seeds) of a single Clip layer on one evaluator, two input vectors per round: labels
    bit-exact against the host evaluator and decoded outputs == plain_q_eval. Returns the launch log of the
    first (eager) round when `log` (the native module) is given."""
    from dash_amd.runtime import HipEvaluator

    c = d.Circuit([d.Clip.from_quantized((N,), lo, hi)])
    gcs = [GarbledCircuit(c, crt, mrs, seed=bytes([i + 1]) * 16, relu=relu) for i in range(2)]
    ev = HipEvaluator([g.model for g in gcs])
    taken = None
    for r in range(0, len(xs), 2):
        pair = xs[r:r + 2]
        enc = [g.garble_inputs(x) for g, x in zip(gcs, pair)]
        cpu = [g.cpu_evaluate(e) for g, e in zip(gcs, enc)]
        if log is not None and r == 0:
            log.hip_launch_log_take()
            log.hip_launch_log(True)
            try:
                gpu = ev.evaluate(enc)  # the first run of an evaluator is eager
            finally:
                log.hip_launch_log(False)
            taken = log.hip_launch_log_take()
        else:
            gpu = ev.evaluate(enc)
        _labels_equal(cpu, gpu)
        if plain:
            for g, x, o in zip(gcs, pair, gpu):
                np.testing.assert_array_equal(g.decode_outputs(o), g.plain_q_eval(x))
    return taken


@pytest.mark.parametrize("N", [1, 75, 513, 1040])
@pytest.mark.parametrize("relu", ["approx", "mrs"])
def test_clip_layer(relu, N):
    """A single lane, an odd size below a wave multiple, one element past a 512 tile and 2 * 512 + 16; the
    values around both bounds also sit on the wave / tile boundary elements (tests.test_clip.clip_inputs)."""
    _run_clip(N, 0, 192, 7, 100.0, relu, clip_inputs(N, 0, 192, M7))


@pytest.mark.parametrize("relu", ["approx", "mrs"])
def test_clip_negative_lower_bound(relu):
    _run_clip(75, -37, 41, 7, 100.0, relu, clip_inputs(75, -37, 41, M7))


def test_clip_large_residue():
    """Activation bytes above 127 through the digit loop. The exact sign needs residue 0 = 2 and odd other
    residues, so it refuses the base [5, 7, 131]; [2, 131] is the smallest base with a residue above 127 that
    it accepts (M = 262: the domain of Clip(-37, 41) is [-90, 94)). Labels only."""
    with pytest.raises(Exception, match="residue 0 = 2"):
        GarbledCircuit(d.Circuit([d.Clip.from_quantized((75,), -37, 41)]), [5, 7, 131], None, relu="mrs",
                       seed=bytes(16))
    _run_clip(75, -37, 41, [2, 131], None, "mrs", clip_inputs(75, -37, 41, 262), plain=False)


@pytest.mark.parametrize("count", [1, 1 << 20], ids=["cus1", "cus1M"])
@pytest.mark.parametrize("N", [528, 1031])
def test_clip_mult_forms(native, N, count):
    """Both forms of the clip multiply, under both planning CU counts (which move the sign chains between
    their forms). The picker is launch_relu_mult's: the staged form needs whole 16-byte rows, so 528 = 2 * 256
    + 16 takes k_clip_mult_s and 1031 (odd) takes k_clip_mult whatever the CU count. (The issue that asked for
    this test expected the staged form under one planning CU and the per-lane form under 2^20 at both sizes; that
    contradicts the picker rule it also set, stage_ok(N) alone, so the form asserted here is the rule's. With one
    planning CU the staged kernel runs one block striding over the three tiles of N = 528.)"""
    native.hip_set_planning_cus(count)
    try:
        log = _run_clip(N, 0, 192, 7, 100.0, "mrs", clip_inputs(N, 0, 192, M7, max_rounds=2), log=native)
    finally:
        native.hip_set_planning_cus(0)
    print("\n".join(log))
    forms = [l.split()[0] for l in log if l.startswith("clip_mult.")]
    assert forms == ["clip_mult.staged" if N % 16 == 0 else "clip_mult.lane"], log


@pytest.mark.parametrize("relu", ["approx", "mrs"])
def test_gpu_garbler_bit_identical_clip(relu):
    """Both sign constructions of a Clip garble on the device (GpuGarbler::clip); the host garbler is the
    reference."""
    from dash_amd.runtime import HipEvaluator

    rng = np.random.default_rng(3)
    c = dense_clip_dense(rng)
    g = _gpu_vs_host(c, 7, 100.0, relu=relu)
    x = rng.integers(-20, 21, 30)
    ev = HipEvaluator(template=g.model, batch=1, device=0)
    ev.load(0, g.model)
    ev.encode_compressed_into(0, g, x)
    ev.upload_inputs_compressed()
    ev.run()
    ev.fetch_outputs()
    np.testing.assert_array_equal(ev.decode(0, g), g.plain_q_eval(x))


@pytest.mark.parametrize("relu", ["approx", "mrs"])
def test_gpu_garbler_clip_into_evaluator_slot(relu):
    """The GPU garbler writes a Clip's tables straight into an evaluator slot (HipEvaluator.sink)."""
    from dash_amd.runtime import HipEvaluator
    from tests.test_gpu_parity import _same

    rng = np.random.default_rng(4)
    c = dense_clip_dense(rng)
    first = GarbledCircuit(c, 7, 100.0, seed=bytes([7]) * 16, device=0, relu=relu)
    ev = HipEvaluator(template=first.model, batch=2, device=0)
    ev.load(0, first.model)
    seed = bytes(range(16))
    into = GarbledCircuit(c, 7, 100.0, seed=seed, device=0, sink=ev.sink(1), relu=relu)
    host = GarbledCircuit(c, 7, 100.0, seed=seed, relu=relu)
    assert _same(into.model.serialize(), host.model.serialize())
    ev.load(1, into.model)
    xs = [rng.integers(-20, 21, 30) for _ in range(2)]
    for b, gc in enumerate((first, into)):
        ev.encode_compressed_into(b, gc, xs[b])
    ev.upload_inputs_compressed()
    ev.run()
    ev.fetch_outputs()
    for b, gc in enumerate((first, into)):
        np.testing.assert_array_equal(ev.decode(b, gc), gc.plain_q_eval(xs[b]))


def test_tiny_mobilenet_flagship():
    """The cut-down MobileNet with the flagship constructions: GPU garbler, HIP evaluator, batch 1."""
    from dash_amd.runtime import HipEvaluator

    c, xs, _ = tiny_mobilenet()
    gc = GarbledCircuit(c, 7, 100.0, seed=bytes(range(16)), device=0, rescale="mrs", relu="joint", hardened=True)
    ev = HipEvaluator(template=gc.model, batch=1, device=0)
    ev.load(0, gc.model)
    for x in xs:
        ev.encode_into(0, gc, x)
        ev.upload_inputs()
        ev.run()
        np.testing.assert_array_equal(gc.decode_outputs(ev.get_outputs()[0]), gc.plain_q_eval(x))


def test_range_guard_torch_path_on_device():
    c, xs, want = guard_case()
    g = RangeGuard(c, M7, mrs=True, device=0)
    assert not g._native_ok()  # guard.hip has no Clip: the batched torch path on the device
    assert g.submit(xs).bad_indices() == [i for i, x in enumerate(xs) if g.violations_np(x)] == \
        [i for i, w in enumerate(want) if w]


def test_check_helper_agrees():
    """The parity suite's own helper on a Clip circuit (fresh evaluator, two GCs)."""
    rng = np.random.default_rng(6)
    c = dense_clip_dense(rng)
    _check(c, 7, 100.0, [rng.integers(-20, 21, 30) for _ in range(2)], relu="mrs", rescale="auto")
