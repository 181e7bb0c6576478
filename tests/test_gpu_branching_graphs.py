"""Concat and padded / ceil-mode pooling on the GPU: the HIP evaluator's k_concat_copy and k_pool_sum, the
clamped max-pool windows through the index gather, the GPU garbler's concat / ragged sum-pool maps, and the
SqueezeNet-style zoo model end to end."""
import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit
from tests.test_branching_graphs import concat_circuit, fire_circuit, pools_circuit
from tests.test_gpu_parity import _check, _gpu_vs_host

pytestmark = pytest.mark.gpu


def _concat3(rng):
    """Three 64-element operands (aligned rows and offsets): the circuit input and two dense layers on it."""
    a = d.Dense.from_quantized(rng.integers(-3, 4, (64, 64)), rng.integers(-5, 6, 64))
    b = d.Dense.from_quantized(rng.integers(-3, 4, (64, 64)), rng.integers(-5, 6, 64))
    b.in_src = -1
    return d.Circuit([a, b, d.Concat([(64,), (64,), (64,)], [-1, 0, 1])])


def _case(name, rng):
    if name == "concat_75_50_12":
        # odd sizes and unaligned offsets; operands: layer 0, the previous layer, the circuit input
        return concat_circuit(rng)
    if name == "concat_3x64":
        return _concat3(rng)
    if name == "sum_3x3_s1_p1":  # every border case
        return d.Circuit([d.SumPool2d(7, 5, 3, 3, 3, 1, 1, pad_width=1, pad_height=1)])
    if name == "sum_3x3_s2_ceil":  # the last window cut at the edge
        return d.Circuit([d.SumPool2d(6, 6, 2, 3, 3, 2, 2, ceil_mode=True)])
    if name == "sum_global_7x7":  # K = 49, unaligned planes
        return d.Circuit([d.SumPool2d(7, 7, 4, 7, 7)])
    if name == "max_3x3_s2_p1":
        return d.Circuit([d.MaxPool2d(7, 7, 3, 3, 3, 2, 2, pad_width=1, pad_height=1)])
    if name == "max_3x3_s2_ceil":
        return d.Circuit([d.MaxPool2d(6, 6, 2, 3, 3, 2, 2, ceil_mode=True)])
    raise KeyError(name)


CASES = ["concat_75_50_12", "concat_3x64", "sum_3x3_s1_p1", "sum_3x3_s2_ceil", "sum_global_7x7", "max_3x3_s2_p1",
         "max_3x3_s2_ceil"]


@pytest.mark.parametrize("name", CASES)
def test_labels_match_host(name):
    """HIP labels bit-exact against the host evaluator; decoded outputs equal plain_q_eval (base 7, 2 GCs)."""
    rng = np.random.default_rng(CASES.index(name) + 40)
    c = _case(name, rng)
    lim = 9 if name.startswith("concat") else 30
    xs = [rng.integers(-lim, lim + 1, c.input_size) for _ in range(2)]
    _check(c, 7, 100.0, xs)


def test_concat_labels_match_host_large_moduli():
    """[5, 7, 131]: activation bytes above 127 through the concat copy (the values exceed the CRT range, so
    only the labels are compared)."""
    rng = np.random.default_rng(50)
    c = concat_circuit(rng)
    xs = [rng.integers(-9, 10, c.input_size) for _ in range(3)]
    _check(c, [5, 7, 131], None, xs, plain=False)


@pytest.mark.parametrize("kw", [dict(rescale="mrs", relu="joint", hardened=True),
                                dict(rescale="legacy", relu="approx", hardened=False)], ids=["flagship", "reference"])
@pytest.mark.parametrize("name", ["fire", "pools"])
def test_gpu_garbler_matches_host_garbler(name, kw):
    """The GPU garbler (concat of saved device labels, ragged sum-pool maps, clamped max-pool windows) is
    byte-identical to the host garbler, and the GC it garbled evaluates to the plaintext outputs."""
    from dash_amd.runtime import HipEvaluator

    c, xs = fire_circuit() if name == "fire" else pools_circuit()
    g = _gpu_vs_host(c, 7, 100.0, **kw)
    ev = HipEvaluator(template=g.model, batch=1, device=0)
    ev.load(0, g.model)
    ev.encode_compressed_into(0, g, xs[0])
    ev.upload_inputs_compressed()
    ev.run()
    ev.fetch_outputs()
    np.testing.assert_array_equal(ev.decode(0, g), g.plain_q_eval(xs[0]))


def test_range_guard_torch_path_on_gpu():
    """A circuit with a padded max pool and a Concat is checked by the batched torch path on the device (the native
    guard has neither form) and flags the inputs the numpy model flags."""
    from dash_amd.garbling import RangeGuard
    from tests.test_branching_graphs import M7, guard_circuit, guard_inputs

    c = guard_circuit()
    xs = guard_inputs(c)
    g = RangeGuard(c, M7, mrs=True, device=0)
    assert g.batched and not g._native_ok()
    ref = [i for i, x in enumerate(xs) if g.violations_np(x)]
    assert ref == [3]
    assert sorted(g.submit(xs).bad_indices()) == ref
    np.testing.assert_array_equal(g.outputs(xs[:3]), np.stack([c.plain_q_eval(x, False, M7) for x in xs[:3]]))


def test_squeezenet_cifar_batch1():
    """SQUEEZENET_CIFAR: GPU-garbled with the flagship constructions, evaluated at batch 1, decoded outputs ==
    plain_q_eval."""
    from dash_amd.ir.quant import QuantizationMethod as Q
    from dash_amd.models import build_circuit, quantized_inputs
    from dash_amd.runtime import HipEvaluator

    name = "SQUEEZENET_CIFAR"
    c = build_circuit(name, Q.ScaleQuant, 5, seed=0)
    x = quantized_inputs(name, 1, Q.ScaleQuant, 5, seed=11)[0]
    gc = GarbledCircuit(c, 7, 100.0, seed=bytes([3]) * 16, device=0, rescale="mrs", relu="joint")
    ev = HipEvaluator(template=gc.model, batch=1, device=0)
    ev.load(0, gc.model)
    ev.encode_compressed_into(0, gc, x)
    ev.upload_inputs_compressed()
    ev.run()
    ev.fetch_outputs()
    np.testing.assert_array_equal(ev.decode(0, gc), gc.plain_q_eval(x))


def test_unpadded_sumpool_keeps_window_sum_kernel():
    """The unpadded sum pool stays on the index-table kernel (op "sum_pool#0"); pads or ceil_mode take the
    geometry-direct one (op "sum_pool#0.geom")."""
    from dash_amd.runtime import HipEvaluator

    for layer, want in ((d.SumPool2d(8, 8, 3, 4, 4), "sum_pool#0"),
                        (d.SumPool2d(8, 8, 3, 3, 3, 2, 2, ceil_mode=True), "sum_pool#0.geom")):
        c = d.Circuit([layer])
        x = np.arange(c.input_size) % 17 - 8
        gc = GarbledCircuit(c, 7, 100.0, seed=b"s" * 16)
        ev = HipEvaluator([gc.model], profile=True)
        out = ev.evaluate([gc.garble_inputs(x)])
        np.testing.assert_array_equal(gc.decode_outputs(out[0]), gc.plain_q_eval(x))
        names = [n for n, _ in ev.op_times()]
        assert want in names and not [n for n in names if n.startswith("sum_pool") and n != want]
