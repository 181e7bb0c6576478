"""The ConvTranspose2d and Upsample layers on the host: semantics against PyTorch, the domain's refusals, the host
garbler and evaluator, the encodings, the wire format, range tracking, ONNX import and export, the range guard, the
zoo's UNET_CIFAR, the train mapping and the sub-pixel weight repack the HIP path uses (docs/CONV_TRANSPOSE.md).

The helpers below (shapes, layers, circuits) are shared with tests/test_gpu_conv_transpose.py.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit, RangeGuard, RangeGuardError
from dash_amd.ir.bases import crt_modulus, first_primes
from dash_amd.ir.layers import Kind
from dash_amd.ir.quant import QuantizationMethod as Q
from dash_amd.native import native
from tests.test_clip import _conv_attrs, _f32, _onnx_model

M7 = crt_modulus(first_primes(7))
SEED = bytes(range(16))
GOLDEN = Path(__file__).resolve().parent / "golden"
B3 = [5, 7, 131]


# ---------------------------------------------------------------- shared helpers
def ceil_div(a, b):
    return -(-a // b)


def in_domain(k, s, p, op):
    return 0 <= p <= k - 1 and 0 <= op < s and op <= s * ceil_div(k, s) - k + p


def convt_weights(rng, C, F, kh, kw):
    """Weights with zeros and multiples of 2, 3, 5 and 7 (zero mod a CRT prime), as tests/test_grouped_conv.py
    builds them."""
    w = rng.integers(-6, 7, (C, F, kh, kw))
    flat = w.reshape(-1)
    flat[::5] = 0
    flat[1::7] = 2 * 3 * 5
    flat[2::11] = -6
    flat[3::13] = 10
    flat[4::17] = 7
    return w, rng.integers(-9, 10, F)


def convt_layer(rng, shape):
    """shape = (W, H, C, F, kh, kw, sw, sh, pw, ph, opw, oph), the order of the constructor."""
    W, H, C, F, kh, kw, sw, sh, pw, ph, opw, oph = shape
    w, b = convt_weights(rng, C, F, kh, kw)
    return d.ConvTranspose2d.from_quantized(w, b, W, H, C, F, kw, kh, sw, sh, pad_width=pw, pad_height=ph,
                                            out_pad_width=opw, out_pad_height=oph)


def torch_convt(x, l, w=None, b=None, dtype=None):
    import torch

    dtype = dtype or torch.float64
    w = l.q_weights if w is None else w
    b = l.q_biases if b is None else b
    y = torch.nn.functional.conv_transpose2d(
        torch.tensor(np.asarray(x).reshape(1, l.C, l.H, l.W), dtype=dtype), torch.tensor(np.asarray(w), dtype=dtype),
        torch.tensor(np.asarray(b), dtype=dtype), stride=(l.sh, l.sw), padding=(l.ph, l.pw),
        output_padding=(l.oph, l.opw))
    return y.numpy().reshape(-1)


def convt_rescale_relu(rng, shape, l=2):
    ct = convt_layer(rng, shape)
    return d.Circuit([ct, d.Rescale(l, ct.out_dims), d.Relu(ct.out_dims)])


def conv_up_conv(rng, fh=2, fw=3):
    """Conv2d 3x3 -> Upsample(fh, fw) -> Conv2d 1x1 on a (2, 4, 5) input."""
    c1 = d.Conv2d.from_quantized(rng.integers(-4, 5, (3, 2, 3, 3)), rng.integers(-5, 6, 3), 5, 4, 2, 3, 3, 3,
                                 pad_width=1, pad_height=1)
    up = d.Upsample(c1.out_dims, fh, fw)
    c2 = d.Conv2d.from_quantized(rng.integers(-4, 5, (2, 3, 1, 1)), rng.integers(-5, 6, 2), up.out_dims[2],
                                 up.out_dims[1], 3, 2, 1, 1)
    return d.Circuit([c1, up, c2])


def _host_eval(gc, x):
    return gc.decode_outputs(gc.cpu_evaluate(gc.garble_inputs(x)))


def guard_case():
    """ConvTranspose2d (one tap per output, every weight 3) -> Rescale(4), mixed-radix, k = 7: M/2 = 255255 and
    the rescale's wrap band is [255247, 255255). Three inputs: small values; one product of 255270 (beyond M/2); one
    of 255249 (a signed CRT value, but inside the band)."""
    ct = d.ConvTranspose2d.from_quantized(np.full((1, 1, 2, 2), 3), [0], 3, 3, 1, 1, 2, 2, 2, 2)
    c = d.Circuit([ct, d.Rescale(4, ct.out_dims)])
    assert M7 // 2 == 255255 and c.layers[1].mrs_limit(M7) == 255247
    ok = np.random.default_rng(41).integers(-20, 21, c.input_size)
    big, band = ok.copy(), ok.copy()
    big[0] = 85090
    band[-1] = 85083
    return c, [ok, big, band]


# ---------------------------------------------------------------- 1. semantics
def _sweep():
    for k in range(1, 6):
        for s in range(1, 4):
            for p in range(k):
                for op in range(s):
                    if in_domain(k, s, p, op):
                        yield (k, k, s, s, p, p, op, op)
    # non-square kernels, unequal strides, unequal pads / output pads
    for kh, kw, sh, sw, ph, pw, oph, opw in [(3, 2, 1, 2, 0, 1, 0, 0), (2, 3, 2, 1, 1, 0, 0, 0), (5, 1, 3, 1, 2, 0, 0, 0),
                                             (1, 4, 1, 2, 0, 1, 0, 0), (4, 3, 2, 3, 1, 2, 0, 1), (3, 5, 2, 2, 1, 2, 1, 0),
                                             (2, 5, 2, 3, 0, 2, 0, 0), (4, 2, 3, 2, 2, 0, 0, 0)]:
        assert in_domain(kh, sh, ph, oph) and in_domain(kw, sw, pw, opw)
        yield (kh, kw, sh, sw, ph, pw, oph, opw)


def test_semantics_against_torch():
    """plain_q_eval (exact: small integers in float64) and plain_eval against torch's conv_transpose2d over every
    square (k, s, p, op) of the domain with k <= 5, s <= 3, and non-square / unequal ones."""
    pytest.importorskip("torch")
    import torch

    rng = np.random.default_rng(1)
    n = 0
    for kh, kw, sh, sw, ph, pw, oph, opw in _sweep():
        C, F, H, W = 2, 3, 5, 6  # the smallest image every (k, s, p) of the sweep leaves an output of
        l = convt_layer(rng, (W, H, C, F, kh, kw, sw, sh, pw, ph, opw, oph))
        assert l.out_dims == (F, (H - 1) * sh - 2 * ph + kh + oph, (W - 1) * sw - 2 * pw + kw + opw)
        x = rng.integers(-20, 21, C * H * W)
        y = l.plain_q_eval(x)
        np.testing.assert_array_equal(y, torch_convt(x, l).astype(np.int64))
        np.testing.assert_allclose(l.plain_eval(x.astype(np.float32)), torch_convt(x, l, dtype=torch.float32), rtol=0,
                                   atol=1e-2)
        n += 1
    assert n >= 90  # 83 square combinations of the domain + 8 unequal ones


def test_float_constructor_quantizes_like_conv2d():
    rng = np.random.default_rng(2)
    w, b = _f32(rng, 3, 4, 2, 2), _f32(rng, 4)
    ct = d.ConvTranspose2d(w, b, 5, 4, 3, 4, 2, 2, 2, 2, 5, Q.ScaleQuant)
    cv = d.Conv2d(w.reshape(3, 4, 2, 2), _f32(rng, 3), 5, 4, 4, 3, 2, 2, 1, 1, 5, Q.ScaleQuant)
    np.testing.assert_array_equal(ct.q_weights.reshape(-1), cv.q_weights.reshape(-1))  # quantize_params, as Conv2d
    kind, spec = ct.garble_spec()
    assert kind == Kind.CONVT == 17 and native().kind_name(17) == "conv_transpose2d"
    assert sorted(spec) == sorted("C H W F kh kw sh sw ph pw oph opw w b".split())


@pytest.mark.parametrize("dims,f", [((3, 2, 5), (2, 3)), ((1, 4, 4), (1, 2)), ((2, 3, 3), (3, 1)), ((4, 1, 1), (2, 2))])
def test_upsample_against_repeat(dims, f):
    rng = np.random.default_rng(3)
    u = d.Upsample(dims, *f)
    assert u.out_dims == (dims[0], dims[1] * f[0], dims[2] * f[1])
    x = rng.integers(-50, 51, int(np.prod(dims)))
    want = np.repeat(np.repeat(x.reshape(dims), f[0], axis=1), f[1], axis=2).reshape(-1)
    np.testing.assert_array_equal(u.plain_q_eval(x), want)
    np.testing.assert_array_equal(u.plain_eval(x.astype(np.float32)), want.astype(np.float32))
    kind, spec = u.garble_spec()
    assert kind == Kind.UPSAMPLE == 18 and native().kind_name(18) == "upsample"
    assert spec == dict(C=dims[0], H=dims[1], W=dims[2], fh=f[0], fw=f[1])
    assert d.Upsample(dims, 2).out_dims == (dims[0], dims[1] * 2, dims[2] * 2)


# ---------------------------------------------------------------- 2. refusals
BAD = [dict(groups=2), dict(dilation=2), dict(pad_height=-1), dict(pad_width=-1), dict(pad_height=3), dict(pad_width=3),
       dict(out_pad_height=2), dict(out_pad_width=2), dict(out_pad_height=-1), dict(out_pad_width=-1),
       dict(filter_height=2, out_pad_height=1), dict(filter_width=2, out_pad_width=1)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_domain_refusals(bad):
    """Every domain condition, from the constructor and from from_quantized; the last two are k = 2, s = 2, p = 0,
    op = 1: an output row that no tap reaches."""
    kw = dict(input_width=4, input_height=4, channel=2, filter=2, filter_width=3, filter_height=3, stride_width=2,
              stride_height=2)
    kw.update(bad)
    w, b = np.zeros((2, 2, kw["filter_height"], kw["filter_width"])), np.zeros(2)
    with pytest.raises(ValueError, match="conv_transpose2d"):
        d.ConvTranspose2d(w, b, **kw)
    with pytest.raises(ValueError, match="conv_transpose2d"):
        d.ConvTranspose2d.from_quantized(w, b, **kw)


def test_decoder_shapes_pass_and_the_native_geometry_agrees():
    for k, s, p, op in [(2, 2, 0, 0), (4, 2, 1, 0), (3, 2, 1, 1)]:
        assert in_domain(k, s, p, op)
        l = d.ConvTranspose2d.from_quantized(np.ones((1, 1, k, k)), [0], 4, 4, 1, 1, k, k, s, s, pad_width=p,
                                             pad_height=p, out_pad_width=op, out_pad_height=op)
        assert l.OH == 8 and l.OW == 8
        plan = native().hip_convt_plan(1, 4, 4, 1, k, k, s, s, p, p, op, op, first_primes(7), True)
        assert (plan["OH"], plan["OW"]) == (8, 8) and plan["VF"] == s * s
    with pytest.raises(Exception, match="output padding"):
        native().hip_convt_plan(1, 4, 4, 1, 2, 2, 2, 2, 0, 0, 1, 1, first_primes(7), True)
    for f in ((1, 1), (0, 2), (2, 0)):
        with pytest.raises(ValueError, match="upsample"):
            d.Upsample((2, 3, 3), *f)
    with pytest.raises(ValueError, match="upsample"):
        d.Upsample((6,), 2)


# ---------------------------------------------------------------- 3. garbled, host
SHAPES = {  # (W, H, C, F, kh, kw, sw, sh, pw, ph, opw, oph)
    "k2s2": (5, 4, 3, 5, 2, 2, 2, 2, 0, 0, 0, 0),
    "k4s2p1": (6, 5, 4, 4, 4, 4, 2, 2, 1, 1, 0, 0),
    "k3s2p1op1": (7, 6, 5, 3, 3, 3, 2, 2, 1, 1, 1, 1),
    "k3s1p1": (9, 5, 4, 6, 3, 3, 1, 1, 1, 1, 0, 0),
    "unequal": (6, 7, 3, 4, 3, 2, 1, 2, 0, 1, 0, 0),
    "s3k5": (4, 4, 2, 2, 5, 5, 3, 3, 2, 2, 0, 0),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_garbled_convt_rescale_relu(name):
    """ConvTranspose2d -> Rescale -> Relu, k = 7, hardened, the flagship constructions: decoded == plain_q_eval."""
    rng = np.random.default_rng(5)
    c = convt_rescale_relu(rng, SHAPES[name])
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED, rescale="mrs", relu="joint", hardened=True)
    assert gc.hardened
    for _ in range(2):
        x = rng.integers(-20, 21, c.input_size)
        y = _host_eval(gc, x)
        np.testing.assert_array_equal(y, gc.plain_q_eval(x))
        ct = c.layers[0]
        np.testing.assert_array_equal(ct.plain_q_eval(x, False), torch_convt(x, ct).astype(np.int64))


def test_garbled_upsample_between_convs():
    rng = np.random.default_rng(6)
    c = conv_up_conv(rng)
    for hardened in (True, False):
        gc = GarbledCircuit(c, 7, None, seed=SEED, hardened=hardened)
        x = rng.integers(-20, 21, c.input_size)
        np.testing.assert_array_equal(_host_eval(gc, x), gc.plain_q_eval(x))


@pytest.mark.parametrize("name", ["k2s2", "k3s2p1op1"])
def test_garbled_base_5_7_131(name):
    """The base [5, 7, 131]: a residue above 127, and weights that are zero mod 5 and 7."""
    rng = np.random.default_rng(7)
    ct = convt_layer(rng, SHAPES[name])
    c = d.Circuit([ct, d.Upsample(ct.out_dims, 2, 1)])
    gc = GarbledCircuit(c, B3, None, seed=SEED, hardened=True)
    x = rng.integers(-4, 5, c.input_size)
    assert np.abs(c.plain_q_eval(x, False)).max() < crt_modulus(B3) // 2
    np.testing.assert_array_equal(_host_eval(gc, x), gc.plain_q_eval(x))


# ---------------------------------------------------------------- 4. encodings
def test_reference_encoding_is_refused_for_convt():
    rng = np.random.default_rng(8)
    ct = convt_layer(rng, SHAPES["k2s2"])
    c = d.Circuit([d.Relu(ct.in_dims), ct])
    with pytest.raises(ValueError, match=r"layer 1 \(conv_transpose2d\).*hardened"):
        GarbledCircuit(c, 7, 100.0, seed=SEED, hardened=False)
    with pytest.raises(ValueError, match=r"layer 1 \(conv_transpose2d\).*hardened"):
        GarbledCircuit(c, 7, 100.0, seed=SEED, fused_sign=False)  # the reference casts cannot be hardened
    c2 = d.Circuit([ct, d.Rescale(2, ct.out_dims)])
    with pytest.raises(ValueError, match=r"layer 0 \(conv_transpose2d\).*hardened"):
        GarbledCircuit(c2, 7, 100.0, seed=SEED, rescale="legacy")
    with pytest.raises(Exception, match="hardened"):  # the native garbler refuses it too
        native().Garbler(first_primes(7), [], SEED, 0).garble(d.Circuit([ct]).garble_specs_native(), list(ct.in_dims), 0,
                                                              -1, True, False, False, False, None, False, False)


def test_reference_encoding_works_for_upsample_and_neither_layer_has_tables():
    rng = np.random.default_rng(9)
    c1 = d.Conv2d.from_quantized(rng.integers(-4, 5, (3, 2, 3, 3)), rng.integers(-5, 6, 3), 5, 4, 2, 3, 3, 3)
    c = d.Circuit([c1, d.Upsample(c1.out_dims, 2, 2), d.Relu((3, 4, 6))])
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED, hardened=False, rescale="legacy", relu="approx")
    assert not gc.hardened
    x = rng.integers(-20, 21, c.input_size)
    np.testing.assert_array_equal(_host_eval(gc, x), gc.plain_q_eval(x))
    assert dict(gc.model.layer_arrays(1)) == {}
    ct = convt_layer(rng, SHAPES["k4s2p1"])
    g2 = GarbledCircuit(d.Circuit([ct, d.Upsample(ct.out_dims, 3, 1)]), 7, None, seed=SEED)
    assert g2.hardened and g2.table_bytes == 0
    assert sorted(g2.model.layer_arrays(0)) == ["w"] and dict(g2.model.layer_arrays(1)) == {}  # public weights only
    assert list(g2.model.const_names()) == []


# ---------------------------------------------------------------- 5. wire format
def test_serialize_roundtrip():
    rng = np.random.default_rng(10)
    ct = convt_layer(rng, SHAPES["k3s2p1op1"])
    c = d.Circuit([ct, d.Upsample(ct.out_dims, 1, 2), d.Relu((ct.F, ct.OH, ct.OW * 2))])
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED)
    blob = gc.model.serialize()
    back = native().GarbledModel.deserialize(blob)
    assert bytes(back.serialize()) == bytes(blob)
    assert [back.layer_kind(i) for i in range(3)] == [17, 18, 2]
    assert {k: list(v) for k, v in back.layer_params(1).items()} == dict(C=[ct.F], H=[ct.OH], W=[ct.OW], fh=[1], fw=[2])
    p0 = back.layer_params(0)
    assert [int(p0[k][0]) for k in ("oph", "opw", "sh", "sw")] == [1, 1, 2, 2]
    x = rng.integers(-20, 21, c.input_size)
    enc = gc.garble_inputs(x)
    a, b = gc.cpu_evaluate(enc), native().cpu_evaluate(back, enc, 0)
    for (pa, la), (pb, lb) in zip(a, b):
        assert pa == pb
        np.testing.assert_array_equal(la, lb)
    np.testing.assert_array_equal(gc.decode_outputs(b), gc.plain_q_eval(x))


@pytest.mark.parametrize("blob", ["dense_rescale_relu_maxpool_v5.bin", "rescale_clip_separate_v4.bin"])
def test_committed_blobs_keep_their_bytes(blob):
    """The wire version is unchanged: blobs without the new kinds load and re-serialize to their bytes."""
    old = (GOLDEN / blob).read_bytes()
    back = native().GarbledModel.deserialize(old)
    assert bytes(back.serialize()) == old
    assert all(back.layer_kind(i) < 17 for i in range(back.num_layers))


# ---------------------------------------------------------------- 6. range tracking
def test_range_tracking_covers_partial_sums():
    """Partial sums exceed the outputs and the products: three channels with weights 1, 1, -1 on inputs of 1000 give
    products of +-1000, running sums 1000, 2000, 1000 in (c, dy, dx) order and outputs of 1000. infer_crt_base_size
    sizes for the 2000: six primes (30030 >= 4000 > 2310), where the outputs alone would take five."""
    w = np.ones((3, 1, 2, 2), dtype=np.int64)
    w[2] = -1
    ct = d.ConvTranspose2d.from_quantized(w, [0], 3, 3, 3, 1, 2, 2, 2, 2)
    x = np.full(3 * 3 * 3, 1000)
    c = d.Circuit([ct])
    np.testing.assert_array_equal(c.plain_q_eval(x, track=False), np.full(36, 1000))
    k = c.infer_crt_base_size([x])
    assert (ct.min_q, ct.max_q) == (-1000, 2000)
    assert k == 6 and crt_modulus(first_primes(5)) < 2 * 2000 <= crt_modulus(first_primes(6))
    # the order is (c, dy, dx): with the negative channel first the running sum dips to -1000 and peaks at 1000
    ct2 = d.ConvTranspose2d.from_quantized(w[::-1].copy(), [0], 3, 3, 3, 1, 2, 2, 2, 2)
    ct2.plain_q_eval(x)
    assert (ct2.min_q, ct2.max_q) == (-1000, 1000)
    # overlapping taps (k3 s2): the sums run over the taps that reach an output; the outputs are covered
    ct3 = convt_layer(np.random.default_rng(11), SHAPES["k3s2p1op1"])
    x3 = np.random.default_rng(12).integers(-20, 21, ct3.in_size)
    y3 = ct3.plain_q_eval(x3)
    assert ct3.min_q <= y3.min() and ct3.max_q >= y3.max()
    # ... and nothing else: the bound over all taps (every product at its extreme) is not reached
    bound = int(np.abs(ct3.q_weights).sum(axis=(0, 2, 3)).max()) * 20 + int(np.abs(ct3.q_biases).max())
    assert max(abs(ct3.min_q), abs(ct3.max_q)) < bound


# ---------------------------------------------------------------- 7. ONNX
def _convt_attrs(k, s, p, op, **extra):
    from dash_amd.ir import onnx as o

    a = (o._attr_ints("kernel_shape", list(k)) + o._attr_ints("strides", list(s))
         + o._attr_ints("pads", [p[0], p[1], p[0], p[1]]) + o._attr_ints("output_padding", list(op)))
    for key, v in extra.items():
        if isinstance(v, str):
            a += o._attr_str(key, v)
        elif isinstance(v, (list, tuple)):
            a += o._attr_ints(key, v)
        else:
            a += o._attr_int(key, v)
    return a


def _resize_attrs(ctm="asymmetric", nm="floor", mode="nearest"):
    from dash_amd.ir import onnx as o

    a = b""
    if ctm is not None:
        a += o._attr_str("coordinate_transformation_mode", ctm)
    if nm is not None:
        a += o._attr_str("nearest_mode", nm)
    return a + o._attr_str("mode", mode)


def test_onnx_convtranspose_import(tmp_path):
    """Conv -> ConvTranspose(k3 s2 p1 op1) -> Relu against the same network in PyTorch."""
    torch = pytest.importorskip("torch")
    from dash_amd.ir import onnx as o
    from dash_amd.ir.onnx import load_onnx_model

    F = torch.nn.functional
    rng = np.random.default_rng(21)
    w1, b1, w2, b2 = _f32(rng, 4, 3, 3, 3), _f32(rng, 4), _f32(rng, 4, 2, 3, 3), _f32(rng, 2)
    nodes = [o._node("Conv", ["input", "w1", "b1"], ["c"], "conv", _conv_attrs(3, 1, 1)),
             o._node("ConvTranspose", ["c", "w2", "b2"], ["t"], "up", _convt_attrs((3, 3), (2, 2), (1, 1), (1, 1))),
             o._node("Relu", ["t"], ["out"], "relu")]
    path = _onnx_model(tmp_path / "ct.onnx", nodes, dict(w1=w1, b1=b1, w2=w2, b2=b2), (1, 3, 5, 6), "out", (1, 2, 10, 12))
    c = load_onnx_model(path, Q.ScaleQuant, 10)
    assert [l.name for l in c.layers] == ["conv2d", "rescale", "conv_transpose2d", "rescale", "approx_relu"]
    assert c.output_dims == (2, 10, 12)
    for _ in range(4):
        x = _f32(rng, 3, 5, 6) * 4
        h = F.conv2d(torch.tensor(x)[None], torch.tensor(w1), torch.tensor(b1), padding=1)
        ref = F.relu(F.conv_transpose2d(h, torch.tensor(w2), torch.tensor(b2), stride=2, padding=1, output_padding=1))
        np.testing.assert_allclose(c.plain_eval(x.reshape(-1), track=False), ref.numpy().reshape(-1), rtol=1e-4,
                                   atol=1e-5)


def test_onnx_convtranspose_folds_batchnorm_and_the_average_factor(tmp_path):
    """AveragePool -> ConvTranspose -> BatchNormalization: the 1/K goes into the weights, the BatchNorm folds along
    axis 1 of the [C][F][kh][kw] weights."""
    torch = pytest.importorskip("torch")
    from dash_amd.ir import onnx as o
    from dash_amd.ir.onnx import load_onnx_model

    F = torch.nn.functional
    rng = np.random.default_rng(22)
    w, b = _f32(rng, 3, 5, 2, 2), _f32(rng, 5)
    bn = {"scale": rng.uniform(0.5, 1.5, 5).astype(np.float32), "shift": _f32(rng, 5), "mean": _f32(rng, 5),
          "var": rng.uniform(0.5, 2.0, 5).astype(np.float32)}
    pool = o._attr_ints("kernel_shape", [2, 2]) + o._attr_ints("pads", [0] * 4) + o._attr_ints("strides", [2, 2])
    nodes = [o._node("AveragePool", ["input"], ["a"], "pool", pool),
             o._node("ConvTranspose", ["a", "w", "b"], ["t"], "up", _convt_attrs((2, 2), (2, 2), (0, 0), (0, 0))),
             o._node("BatchNormalization", ["t", "scale", "shift", "mean", "var"], ["out"], "bn",
                     o._attr_float("epsilon", 1e-5))]
    path = _onnx_model(tmp_path / "bn.onnx", nodes, dict(w=w, b=b, **bn), (1, 3, 4, 6), "out", (1, 5, 4, 6))
    c = load_onnx_model(path, Q.ScaleQuant, 10)
    assert [l.name for l in c.layers] == ["sum_pool", "conv_transpose2d", "rescale"]
    g = bn["scale"] / np.sqrt(bn["var"] + 1e-5)
    np.testing.assert_allclose(c.layers[1].weights, w * 0.25 * g[None, :, None, None], rtol=1e-6)
    for _ in range(4):
        x = _f32(rng, 3, 4, 6) * 4
        t = F.conv_transpose2d(F.avg_pool2d(torch.tensor(x)[None], 2), torch.tensor(w), torch.tensor(b), stride=2)
        ref = F.batch_norm(t, torch.tensor(bn["mean"]), torch.tensor(bn["var"]), torch.tensor(bn["scale"]),
                           torch.tensor(bn["shift"]), eps=1e-5)
        np.testing.assert_allclose(c.plain_eval(x.reshape(-1), track=False), ref.numpy().reshape(-1), rtol=1e-4,
                                   atol=1e-5)


@pytest.mark.parametrize("attrs,what", [
    (dict(dilations=[2, 2]), "dilated"), (dict(auto_pad="SAME_UPPER"), "auto_pad"),
    (dict(output_shape=[10, 12]), "output_shape"), (dict(group=2), "group"), ("asym", "asymmetric"),
    ("domain", "output padding")])
def test_onnx_convtranspose_refusals(tmp_path, attrs, what):
    from dash_amd.ir import onnx as o
    from dash_amd.ir.onnx import load_onnx_model

    rng = np.random.default_rng(23)
    w, b = _f32(rng, 2, 2, 2, 2), _f32(rng, 2)
    if attrs == "asym":
        a = (o._attr_ints("kernel_shape", [2, 2]) + o._attr_ints("strides", [2, 2]) + o._attr_ints("pads", [0, 0, 1, 1]))
    elif attrs == "domain":
        a = _convt_attrs((2, 2), (2, 2), (0, 0), (1, 1))
    else:
        a = _convt_attrs((2, 2), (2, 2), (0, 0), (0, 0), **attrs)
    path = _onnx_model(tmp_path / "bad.onnx", [o._node("ConvTranspose", ["input", "w", "b"], ["out"], "decoder_up", a)],
                       dict(w=w, b=b), (1, 2, 3, 3), "out", (1, 2, 6, 6))
    with pytest.raises((NotImplementedError, ValueError), match=f"decoder_up.*{what}"):
        load_onnx_model(path, Q.ScaleQuant, 10)


@pytest.mark.parametrize("form", ["resize_scales", "resize_sizes", "upsample9", "upsample7"])
def test_onnx_resize_import(tmp_path, form):
    """Conv -> Resize / Upsample (nearest, x2 x3) -> Conv against PyTorch's nearest interpolation; a pending
    average factor passes through the upsampling into the second conv."""
    torch = pytest.importorskip("torch")
    from dash_amd.ir import onnx as o
    from dash_amd.ir.onnx import load_onnx_model

    F = torch.nn.functional
    rng = np.random.default_rng(24)
    w1, b1, w2, b2 = _f32(rng, 4, 3, 3, 3), _f32(rng, 4), _f32(rng, 2, 4, 1, 1), _f32(rng, 2)
    inits = dict(w1=w1, b1=b1, w2=w2, b2=b2)
    opset = 11
    if form == "resize_scales":
        inits["sc"] = np.asarray([1, 1, 2, 3], np.float32)
        up = o._node("Resize", ["p", "", "sc"], ["u"], "up", _resize_attrs())
    elif form == "resize_sizes":
        up = o._node("Resize", ["p", "", "", "sz"], ["u"], "up", _resize_attrs())
    elif form == "upsample9":
        opset = 9
        inits["sc"] = np.asarray([1, 1, 2, 3], np.float32)
        up = o._node("Upsample", ["p", "sc"], ["u"], "up", o._attr_str("mode", "nearest"))
    else:
        opset = 7
        fl = o._ld(5, o._s(1, "scales") + b"".join(o._key(7, 5) + np.float32(v).tobytes() for v in (1, 1, 2, 3))
                   + o._i(20, 6))
        up = o._node("Upsample", ["p"], ["u"], "up", o._attr_str("mode", "nearest") + fl)
    pool = o._attr_ints("kernel_shape", [2, 2]) + o._attr_ints("pads", [0] * 4) + o._attr_ints("strides", [2, 2])
    nodes = [o._node("Conv", ["input", "w1", "b1"], ["c"], "conv", _conv_attrs(3, 1, 1)),
             o._node("AveragePool", ["c"], ["p"], "pool", pool), up,
             o._node("Conv", ["u", "w2", "b2"], ["out"], "head", _conv_attrs(1))]
    path = tmp_path / "rs.onnx"
    _onnx_model(path, nodes, inits, (1, 3, 4, 6), "out", (1, 2, 4, 9), opset=opset)
    if form == "resize_sizes":  # an int64 initializer, appended to the graph written above
        path.write_bytes(_with_i64_init(nodes, inits, "sz", [1, 4, 4, 9], (1, 3, 4, 6), "out", (1, 2, 4, 9), opset))
    c = load_onnx_model(path, Q.ScaleQuant, 10)
    assert [l.name for l in c.layers] == ["conv2d", "rescale", "sum_pool", "upsample", "conv2d", "rescale"]
    assert (c.layers[3].fh, c.layers[3].fw) == (2, 3) and c.output_dims == (2, 4, 9)
    for _ in range(4):
        x = _f32(rng, 3, 4, 6) * 4
        h = F.avg_pool2d(F.conv2d(torch.tensor(x)[None], torch.tensor(w1), torch.tensor(b1), padding=1), 2)
        h = F.interpolate(h, scale_factor=(2, 3), mode="nearest")
        ref = F.conv2d(h, torch.tensor(w2), torch.tensor(b2))
        np.testing.assert_allclose(c.plain_eval(x.reshape(-1), track=False), ref.numpy().reshape(-1), rtol=1e-4,
                                   atol=1e-5)


def _with_i64_init(nodes, inits, name, vals, in_dims, out_name, out_dims, opset):
    from dash_amd.ir import onnx as o

    graph = b"".join(nodes) + o._s(2, "g") + b"".join(o._ld(5, o._tensor(n, v)) for n, v in inits.items())
    graph += o._ld(5, o._tensor_i64(name, vals))
    graph += o._ld(11, o._value_info("input", in_dims)) + o._ld(12, o._value_info(out_name, out_dims))
    return o._i(1, 7) + o._s(2, "test") + o._s(3, "1") + o._ld(7, graph) + o._ld(8, o._s(1, "") + o._i(2, opset))


@pytest.mark.parametrize("case,what", [
    ("linear", "mode"), ("half_pixel", "coordinate_transformation_mode"), ("default_ctm", "coordinate_transformation_mode"),
    ("round", "nearest_mode"), ("frac", "scales"), ("batch", "scales"), ("ones", "scales"), ("no_scales", "scales or sizes"),
    ("opset10", "opset")])
def test_onnx_resize_refusals(tmp_path, case, what):
    from dash_amd.ir import onnx as o
    from dash_amd.ir.onnx import load_onnx_model

    sc, attrs, ins, opset = [1, 1, 2, 2], _resize_attrs(), ["input", "", "sc"], 11
    if case == "linear":
        attrs = _resize_attrs(mode="linear")
    elif case == "half_pixel":
        attrs = _resize_attrs(ctm="half_pixel")
    elif case == "default_ctm":
        attrs = _resize_attrs(ctm=None)
    elif case == "round":
        attrs = _resize_attrs(nm="round_prefer_floor")
    elif case == "frac":
        sc = [1, 1, 1.5, 2]
    elif case == "batch":
        sc = [2, 1, 2, 2]
    elif case == "ones":
        sc = [1, 1, 1, 1]
    elif case == "no_scales":
        ins = ["input"]
    elif case == "opset10":
        opset = 10
    path = _onnx_model(tmp_path / "bad.onnx", [o._node("Resize", ins, ["out"], "decoder_resize", attrs)],
                       dict(sc=np.asarray(sc, np.float32)), (1, 2, 3, 3), "out", (1, 2, 6, 6), opset=opset)
    with pytest.raises(NotImplementedError, match=f"decoder_resize.*{what}"):
        load_onnx_model(path, Q.ScaleQuant, 10)


@pytest.mark.parametrize("scheme,param", [(Q.ScaleQuant, 5), (Q.SimpleQuant, -1), (Q.ScaleQuantPlus, 32)])
def test_onnx_export_import_roundtrip(tmp_path, scheme, param):
    from dash_amd.ir.onnx import load_onnx_model, parse_onnx, save_onnx_model
    from dash_amd.models import build_circuit, quantized_inputs

    c = build_circuit("UNET_CIFAR", scheme, param, seed=0)
    save_onnx_model(tmp_path / "u.onnx", c)
    ops = [n["op_type"] for n in parse_onnx(tmp_path / "u.onnx")["nodes"]]
    assert ops.count("ConvTranspose") == 1 and ops.count("Resize") == 1 and ops.count("Concat") == 2
    back = load_onnx_model(tmp_path / "u.onnx", scheme, param)
    assert [l.name for l in back.layers] == [l.name for l in c.layers]
    for x in quantized_inputs("UNET_CIFAR", 2, scheme, param, seed=1):
        np.testing.assert_array_equal(back.plain_q_eval(x, False), c.plain_q_eval(x, False))


# ---------------------------------------------------------------- 8. range guard
def test_range_guard_paths_agree():
    pytest.importorskip("torch")
    c, xs = guard_case()
    g = RangeGuard(c, M7, mrs=True, device=None)
    assert g.batched and not g.native_forms and not g._native_ok()
    want = [bool(g.violations_np(x)) for x in xs]
    assert want == [False, True, True]
    assert g.submit(xs).bad_indices() == [i for i, w in enumerate(want) if w]  # the torch path, CPU device
    np.testing.assert_array_equal(g.outputs(xs[:1]), [c.plain_q_eval(xs[0], False, M7)])
    with pytest.raises(RangeGuardError):
        g.check(xs)
    # Upsample: batched too, values pass through to the layers behind it
    rng = np.random.default_rng(42)
    c2 = conv_up_conv(rng)
    c2 = d.Circuit(list(c2.layers) + [d.Relu(c2.output_dims)])
    g2 = RangeGuard(c2, M7, mrs=True, device=None)
    assert g2.batched and not g2.native_forms
    ys = [rng.integers(-20, 21, c2.input_size), np.full(c2.input_size, M7 // 8)]
    assert g2.submit(ys).bad_indices() == [i for i, y in enumerate(ys) if g2.violations_np(y)] == [1]
    np.testing.assert_array_equal(g2.outputs(ys[:1]), [c2.plain_q_eval(ys[0], False, M7)])


# ---------------------------------------------------------------- 9. zoo and training
def unet():
    from dash_amd.models import BENCH_CONFIGS, build_circuit, quantized_inputs

    cfg = BENCH_CONFIGS["UNET_CIFAR/DASH"]
    assert (cfg["model"], cfg["q_method"], cfg["q_parameter"], cfg["crt"], cfg["mrs"]) == \
        ("UNET_CIFAR", Q.ScaleQuant, 5, 7, 100.0)
    c = build_circuit(cfg["model"], cfg["q_method"], cfg["q_parameter"], seed=0)
    xs = quantized_inputs("UNET_CIFAR", 2, cfg["q_method"], cfg["q_parameter"], seed=7)
    return cfg, c, xs


def test_zoo_unet_cifar():
    from dash_amd.models import synthetic_inputs
    from dash_amd.ir.quant import quantize_input

    cfg, c, _ = unet()
    names = [l.name for l in c.layers]
    assert c.input_dims == (3, 32, 32) and c.output_dims == (1, 32, 32)
    assert names.count("conv_transpose2d") == 1 and names.count("upsample") == 1 and names.count("concat") == 2
    assert names[-1] == "argmax"
    cats = [l for l in c.layers if l.name == "concat"]
    assert cats[0].out_dims == (32, 16, 16) and cats[1].out_dims == (24, 32, 32)  # skip first, then the decoder
    agree = []
    for xf in synthetic_inputs("UNET_CIFAR", 3, seed=3):
        yq = c.plain_q_eval(quantize_input(xf, cfg["q_method"], cfg["q_parameter"], 0.02), False)
        yf = c.plain_eval(xf, False)
        assert set(np.unique(yq)) <= {0, 1, 2, 3}
        agree.append(float(np.mean(yq == yf)))
    assert min(agree) > 0.8, agree


def test_zoo_unet_cifar_garbled_on_the_host():
    cfg, c, xs = unet()
    gc = GarbledCircuit(c, cfg["crt"], cfg["mrs"], seed=SEED, rescale="mrs")
    assert gc.hardened and gc.relu == "joint"
    y = _host_eval(gc, xs[0])
    np.testing.assert_array_equal(y, gc.plain_q_eval(xs[0]))
    assert y.shape == (32 * 32,)


def test_train_mapping_of_convt_and_up():
    torch = pytest.importorskip("torch")
    from dash_amd.models import zoo
    from dash_amd.models.train import build_torch_model, to_circuit

    zoo.ARCHS["_TINY_DECODER"] = {"input": (2, 4, 4), "ops": [
        ("conv", 3, 3, 1, 1), ("relu",), ("convt", 2, 3, 2, 1, 1), ("relu",), ("up", 2), ("conv", 2, 1, 1, 0)]}
    try:
        torch.manual_seed(0)
        m = build_torch_model("_TINY_DECODER")
        c = to_circuit(m, "_TINY_DECODER", Q.ScaleQuant, 10)
        assert [l.name for l in c.layers] == ["conv2d", "rescale", "approx_relu", "conv_transpose2d", "rescale",
                                              "approx_relu", "upsample", "conv2d", "rescale"]
        assert c.output_dims == (2, 16, 16)
        x = np.random.default_rng(5).uniform(-1, 1, (2, 4, 4)).astype(np.float32)
        with torch.no_grad():
            ref = m(torch.tensor(x)[None]).numpy().reshape(-1)
        np.testing.assert_allclose(c.plain_eval(x.reshape(-1), track=False), ref, rtol=1e-4, atol=1e-5)
        ref_c = zoo.build_circuit("_TINY_DECODER", Q.ScaleQuant, 10)
        assert [l.name for l in ref_c.layers] == [l.name for l in c.layers]
    finally:
        del zoo.ARCHS["_TINY_DECODER"]
    with pytest.raises(NotImplementedError, match="skip"):
        build_torch_model("UNET_CIFAR")


# ---------------------------------------------------------------- 10. the sub-pixel view (the HIP path's repack)
def _view_reference(x, l, wv):
    """The identity of docs/CONV_TRANSPOSE.md in numpy: stride-1 conv of the padded input with the view weights
    wv [F sh sw][C][Th][Tw], then the depth-to-space scatter and crop; hits counts how often each output is written."""
    Th, Tw = ceil_div(l.kh, l.sh), ceil_div(l.kw, l.sw)
    xp = np.pad(np.asarray(x, dtype=np.int64).reshape(l.C, l.H, l.W), ((0, 0), (Th - 1, Th - 1), (Tw - 1, Tw - 1)))
    VH, VW = l.H + Th - 1, l.W + Tw - 1
    v = np.zeros((l.F * l.sh * l.sw, VH, VW), dtype=np.int64)
    for ty in range(Th):
        for tx in range(Tw):
            v += np.einsum("fc,cyx->fyx", wv[:, :, ty, tx], xp[:, ty:ty + VH, tx:tx + VW])
    y = np.zeros((l.F, l.OH, l.OW), dtype=np.int64)
    hits = np.zeros_like(y)
    for fv in range(v.shape[0]):
        f, r = divmod(fv, l.sh * l.sw)
        ry, rx = divmod(r, l.sw)
        for qy in range(VH):
            for qx in range(VW):
                oy, ox = l.sh * qy + ry - l.ph, l.sw * qx + rx - l.pw
                if 0 <= oy < l.OH and 0 <= ox < l.OW:
                    y[f, oy, ox] = v[fv, qy, qx]
                    hits[f, oy, ox] += 1
    return y, hits


def test_sub_pixel_weight_repack():
    """native convt_view_weights against the identity written out here, and view conv + scatter == the layer, with
    every output written exactly once, over the square sweep's (k, s) and the unequal shapes."""
    rng = np.random.default_rng(13)
    seen = 0
    for kh, kw, sh, sw, ph, pw, oph, opw in _sweep():
        C, F, H, W = 2, 3, 5, 6  # the smallest image every (k, s, p) of the sweep leaves an output of
        l = convt_layer(rng, (W, H, C, F, kh, kw, sw, sh, pw, ph, opw, oph))
        w = l.q_weights
        Th, Tw = ceil_div(kh, sh), ceil_div(kw, sw)
        want = np.zeros((F * sh * sw, C, Th, Tw), dtype=np.int64)
        for f in range(F):
            for ry in range(sh):
                for rx in range(sw):
                    for ty in range(Th):
                        for tx in range(Tw):
                            dy, dx = ry + sh * (Th - 1 - ty), rx + sw * (Tw - 1 - tx)
                            if dy < kh and dx < kw:
                                want[f * sh * sw + ry * sw + rx, :, ty, tx] = w[:, f, dy, dx]
        got = np.asarray(native().convt_view_weights([int(v) for v in w.reshape(-1)], C, F, kh, kw, sh, sw))
        np.testing.assert_array_equal(got.reshape(want.shape), want)
        x = rng.integers(-20, 21, C * H * W)
        y, hits = _view_reference(x, l, got.reshape(want.shape))
        assert hits.min() == 1 and hits.max() == 1, (kh, kw, sh, sw, ph, pw, oph, opw)
        np.testing.assert_array_equal((y + l.q_biases[:, None, None]).reshape(-1), l.plain_q_eval(x, False))
        plan = native().hip_convt_plan(C, H, W, F, kh, kw, sh, sw, ph, pw, oph, opw, first_primes(7), True)
        assert (plan["VF"], plan["VOH"], plan["VOW"], plan["Th"], plan["Tw"], plan["OH"], plan["OW"]) == \
            (F * sh * sw, H + Th - 1, W + Tw - 1, Th, Tw, l.OH, l.OW)
        seen += 1
    assert seen >= 90


def test_plain_conv_plans_are_unaffected():
    """The planner binding of a plain conv has no scatter fields and equals the view's plan where the geometry is
    the same (the view is an ordinary conv to conv_layer_plan)."""
    n = native()
    plain = n.hip_conv_plan(64, 16, 16, 128, 1, 1, 1, 1, 0, 0, first_primes(7), True)
    view = n.hip_convt_plan(64, 16, 16, 32, 2, 2, 2, 2, 0, 0, 0, 0, first_primes(7), True)
    assert "tsc" not in plain
    for key in ("ur", "KS", "Cpad", "Kpad", "band", "nbands"):
        assert plain[key] == view[key], key
    assert view["tsc"] in (1, 2) and view["VF"] == 128


# ---------------------------------------------------------------- 11. command line
def test_cli_infer_unet_cifar(capsys):
    """python -m dash_amd infer --model UNET_CIFAR --scheme DASH (host backend here; tests/test_gpu_conv_transpose.py
    evaluates the model on the GPU): the CLI calibrates the circuit so that its rescales can be hardened."""
    from dash_amd.__main__ import main

    main(["infer", "--model", "UNET_CIFAR", "--scheme", "DASH", "--backend", "cpu", "--inputs", "1"])
    out = capsys.readouterr().out
    assert "ConvTranspose2d" in out and "Upsample" in out and "garbled==plaintext: True" in out
