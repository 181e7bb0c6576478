"""Grouped / depthwise convolution on the GPU: the byte-stencil kernel k_conv_grp behind both the HIP evaluator
and the GPU garbler, the native range guard's grouped conv, and the depthwise-separable zoo model."""
import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit, RangeGuard
from tests.test_gpu_parity import _check, _gpu_vs_host
from tests.test_grouped_conv import M_GUARD, guard_circuit, guard_inputs

pytestmark = pytest.mark.gpu

# (W, H, C, F, g, kh, kw, sw, sh, pad): each shape for one thing that can break
SHAPES = {
    "odd_width": (9, 9, 4, 4, 4, 3, 3, 1, 1, 1),
    "multiplier2": (9, 9, 4, 8, 4, 3, 3, 1, 1, 1),
    "stride_pad": (11, 5, 6, 6, 6, 3, 3, 2, 2, 1),
    "unequal_strides": (12, 9, 3, 3, 3, 3, 3, 1, 2, 1),
    "cg4_fg6": (13, 6, 8, 12, 2, 3, 3, 1, 1, 0),
    "grouped_1x1": (7, 7, 6, 6, 3, 1, 1, 1, 1, 0),
    "kw5_two_dwords": (16, 6, 5, 5, 5, 5, 5, 1, 1, 2),
    "groups70": (8, 8, 70, 70, 70, 3, 3, 1, 1, 1),
    "two_bands": (32, 36, 2, 2, 2, 3, 3, 1, 1, 1),
    # 64 slots per plane (wave-uniform filter) through the 1x1 and the runtime-tap instances
    "wide_1x1": (32, 8, 4, 4, 2, 1, 1, 1, 1, 0),
    "wide_5x5": (32, 8, 2, 2, 2, 5, 5, 1, 1, 2),
}


def _layer(rng, W, H, C, F, g, kh, kw, sw, sh, pad):
    w = rng.integers(-5, 6, (F, C // g, kh, kw))
    flat = w.reshape(-1)
    flat[::4] = 0  # zero weights and multiples of the CRT primes take the Z_p quirk
    flat[1::9] = 5 * 7
    flat[2::11] = -131
    flat[3::13] = 2 * 3 * 5 * 7
    b = rng.integers(-5, 6, F)
    return d.Conv2d.from_quantized(w, b, W, H, C, F, kw, kh, sw, sh, pad_width=pad, pad_height=pad, groups=g)


@pytest.mark.parametrize("crt", [7, [5, 7, 131]], ids=["base7_2gc", "p131_3gc"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_grouped_conv_labels_match_host(name, crt):
    """HIP labels bit-exact against the host evaluator, decoded outputs equal to plain_q_eval where the CRT
    range holds the values (base 7). [5, 7, 131] has activation bytes above 127.

    two_bands: 32 x 36 input, 3x3, pad 1 gives OH = 36 rows of ceil(32 / 4) = 8 lane slots; 36 * 8 = 288 slots
    exceed the block's 256 lanes, so the band rule keeps 256 / 8 = 32 rows per block: bands of 32 and 4 rows.
    groups70: a block holds at most 32 groups (launch.h kGrpMaxGroups): three group blocks, the last with 6
    groups."""
    shape = SHAPES[name]
    W, H, C = shape[:3]
    rng = np.random.default_rng(sum(shape))
    c = d.Circuit([_layer(rng, *shape)])
    n = 2 if crt == 7 else 3
    xs = [rng.integers(-6, 7, C * H * W) for _ in range(n)]
    _check(c, crt, None, xs, plain=crt == 7)


def _dw_block(rng):
    """depthwise 3x3 -> rescale -> ReLU -> 1x1 conv on 8 x 8 x 8"""
    dw = _layer(rng, 8, 8, 8, 8, 8, 3, 3, 1, 1, 1)
    pw = d.Conv2d.from_quantized(rng.integers(-5, 6, (8, 8, 1, 1)), rng.integers(-5, 6, 8), 8, 8, 8, 8, 1, 1)
    c = d.Circuit([dw, d.Rescale(3, dw.out_dims), d.Relu(dw.out_dims), pw])
    xs = [rng.integers(-20, 21, c.input_size) for _ in range(4)]
    from dash_amd.ir.bases import crt_modulus, first_primes

    c.calibrate(xs, crt_modulus(first_primes(7)))
    return c, xs


@pytest.mark.parametrize("kw", [dict(rescale="mrs", relu="joint", hardened=True),
                                dict(rescale="legacy", relu="approx", hardened=False)], ids=["flagship", "reference"])
def test_gpu_garbler_matches_host_garbler(kw):
    """The GPU garbler (k_conv_grp on the zero labels) is byte-identical to the host garbler, and the GC it
    garbled evaluates to the plaintext outputs."""
    from dash_amd.runtime import HipEvaluator

    c, xs = _dw_block(np.random.default_rng(21))
    g = _gpu_vs_host(c, 7, 100.0, **kw)
    ev = HipEvaluator(template=g.model, batch=1, device=0)
    ev.load(0, g.model)
    ev.encode_compressed_into(0, g, xs[0])
    ev.upload_inputs_compressed()
    ev.run()
    ev.fetch_outputs()
    np.testing.assert_array_equal(ev.decode(0, g), g.plain_q_eval(xs[0]))


def test_native_range_guard_depthwise():
    """DevRangeGuard (k_g_conv with groups) flags exactly what the numpy model flags, the band input included;
    a grouped layer with several channels and filters per group passes its in-range inputs."""
    c = guard_circuit()
    xs = guard_inputs(c)
    g = RangeGuard(c, M_GUARD, mrs=True, device=0)
    ref = [i for i, x in enumerate(xs) if g.violations_np(x)]
    assert ref == [3]
    assert sorted(g.submit(xs).bad_indices()) == ref
    # C/g = 3, F/g = 10 (two filter blocks per group, the second clamped) ahead of a rescale whose limit the
    # scaled-up input crosses: the flags depend on the grouped sums themselves
    rng = np.random.default_rng(4)
    conv = _layer(rng, 9, 7, 6, 20, 2, 3, 3, 2, 1, 1)
    c2 = d.Circuit([conv, d.Rescale(3, conv.out_dims), d.Relu(conv.out_dims)])
    x2 = [rng.integers(-20, 21, c2.input_size) for _ in range(4)]
    c2.calibrate(x2, M_GUARD)
    x2.append(x2[0] * 4000)
    g2 = RangeGuard(c2, M_GUARD, mrs=True, device=0)
    ref2 = [i for i, x in enumerate(x2) if g2.violations_np(x)]
    assert ref2 == [4]
    assert sorted(g2.submit(x2).bad_indices()) == ref2


def test_dwsep_cifar_batch1():
    """MODEL_DWSEP_CIFAR: GPU-garbled with the flagship constructions, evaluated at batch 1, decoded outputs ==
    plain_q_eval."""
    from dash_amd.ir.quant import QuantizationMethod as Q
    from dash_amd.models import build_circuit, quantized_inputs
    from dash_amd.runtime import HipEvaluator

    name = "MODEL_DWSEP_CIFAR"
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
