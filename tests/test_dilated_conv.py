"""Dilated (atrous) Conv2d on the host: semantics against PyTorch, the host garbler and evaluator under both
encodings and two CRT bases, the wire format, the refusals, ONNX import / export with `dilations` and `auto_pad`, the
trainer mapping, the range guard, the zoo's ASPP_SEG_CIFAR and the HIP planner's geometry through its bindings
(docs/DILATED_CONV.md). The shape table and the builders are tests/dilated_cases.py; aspp_seg(), guard_case() and M7
are shared with tests/test_gpu_dilated_conv.py."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit, RangeGuard, RangeGuardError
from dash_amd.ir.bases import crt_modulus, first_primes
from dash_amd.ir.quant import QuantizationMethod as Q
from dash_amd.native import native
from tests.dilated_cases import (B3, DENSE, GROUPED, SHAPES, conv_layer, conv_rescale_relu, form_of, plan_of, torch_conv,
                                 undilated, weights)
from tests.gemm_cases import CONV_CASES
from tests.test_clip import _f32, _onnx_model

M7 = crt_modulus(first_primes(7))
SEED = bytes(range(16))
GOLDEN = Path(__file__).resolve().parent / "golden"
BASES = {"k7": 7, "b3": B3}
LDS_BUDGET = 40 * 1024  # the dense conv's default band budget (launch.h conv_img_geometry)


def _host_eval(gc, x):
    return gc.decode_outputs(gc.cpu_evaluate(gc.garble_inputs(x)))


def _centered(y, M):
    """The signed CRT value of y: what a decoder returns for a plaintext result outside [-M/2, M/2)."""
    h = M // 2
    return (np.asarray(y, dtype=np.int64) + h) % M - h


def guard_case():
    """Conv2d 3x3 with d = 2, p = 2 on a 5x5 plane, centre tap 3 and top-left tap 1 -> Rescale(4), mixed-radix,
    k = 7: M/2 = 255255 and the rescale's wrap band is [255247, 255255). Three inputs: small values; a centre pixel
    whose product alone is 255270; one whose output 3 * 85083 + 0 = 255249 is a signed CRT value inside the band."""
    w = np.zeros((1, 1, 3, 3), dtype=np.int64)
    w[0, 0, 1, 1], w[0, 0, 0, 0] = 3, 1
    cv = d.Conv2d.from_quantized(w, [0], 5, 5, 1, 1, 3, 3, pad_width=2, pad_height=2, dilation_width=2,
                                 dilation_height=2)
    c = d.Circuit([cv, d.Rescale(4, cv.out_dims)])
    assert M7 // 2 == 255255 and c.layers[1].mrs_limit(M7) == 255247
    ok = np.random.default_rng(41).integers(-20, 21, c.input_size)
    big, band = ok.copy(), ok.copy()
    big[12] = 85090 + 10  # output (2, 2) = 3 x[2][2] + x[0][0] >= 255280: beyond M/2
    band[12], band[0] = 85083, 0
    return c, [ok, big, band]


def aspp_seg():
    from dash_amd.models import BENCH_CONFIGS, build_circuit, quantized_inputs

    cfg = BENCH_CONFIGS["ASPP_SEG_CIFAR/DASH"]
    assert (cfg["model"], cfg["q_method"], cfg["q_parameter"], cfg["crt"], cfg["mrs"]) == \
        ("ASPP_SEG_CIFAR", Q.ScaleQuant, 5, 7, 100.0)
    c = build_circuit(cfg["model"], cfg["q_method"], cfg["q_parameter"], seed=2)
    xs = quantized_inputs("ASPP_SEG_CIFAR", 2, cfg["q_method"], cfg["q_parameter"], seed=7)
    return cfg, c, xs


# ---------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_plain_eval_against_torch(name):
    """plain_q_eval equals torch.nn.functional.conv2d in float64 exactly (the integers are far below 2^53);
    plain_eval agrees to float32 tolerance."""
    rng = np.random.default_rng(sum(map(ord, name)))
    W, H, C, F, kh, kw, sw, sh, pw, ph, dw, dh, g = SHAPES[name]
    l = conv_layer(rng, SHAPES[name])
    assert (l.dh, l.dw) == (dh if kh > 1 else 1, dw if kw > 1 else 1)
    assert (l.OH, l.OW) == ((H + 2 * ph - (kh - 1) * dh - 1) // sh + 1, (W + 2 * pw - (kw - 1) * dw - 1) // sw + 1)
    for _ in range(2):
        x = rng.integers(-20, 21, l.in_size)
        ref = torch_conv(x, l)
        assert np.abs(ref).max() < 2 ** 53
        y = l.plain_q_eval(x, False)
        assert y.dtype == np.int64
        np.testing.assert_array_equal(y.astype(np.float64), ref)
        import torch

        np.testing.assert_allclose(l.plain_eval(x.astype(np.float32), False), torch_conv(x, l, torch.float32),
                                   rtol=1e-5, atol=1e-3)


def test_range_tracking_is_unchanged_in_kind():
    """Products and running partial sums of the dilated taps are tracked as for the plain conv: three taps with
    weights 1, 1, -1 on inputs of 1000 reach a partial sum of 2000 that neither a product nor the output shows."""
    w = np.zeros((1, 1, 1, 3), dtype=np.int64)
    w[0, 0, 0] = [1, 1, -1]
    l = d.Conv2d.from_quantized(w, [0], 7, 1, 1, 1, 3, 1, dilation_width=3)
    assert (l.OH, l.OW) == (1, 1)
    x = np.zeros(7, dtype=np.int64)
    x[[0, 3, 6]] = 1000
    np.testing.assert_array_equal(l.plain_q_eval(x), [1000])
    assert l.max_q == 2000


# ---------------------------------------------------------------- 2. the host engines
@pytest.mark.parametrize("hardened", [True, False], ids=["hardened", "reference"])
@pytest.mark.parametrize("base", sorted(BASES))
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_host_garble_evaluate_decode(name, base, hardened):
    """One layer alone: the host garbler and the host evaluator decode to plain_q_eval (for the base [5, 7, 131]
    to its signed CRT value: the products of wide rows exceed M = 4585)."""
    rng = np.random.default_rng(sum(map(ord, name)) + 1)
    c = d.Circuit([conv_layer(rng, SHAPES[name])])
    gc = GarbledCircuit(c, BASES[base], None, seed=SEED, hardened=hardened)
    assert gc.hardened == hardened
    x = rng.integers(-20, 21, c.input_size) if base == "k7" else rng.integers(-1, 2, c.input_size)
    want = gc.plain_q_eval(x)
    if base == "b3":
        want = _centered(want, crt_modulus(B3))
    np.testing.assert_array_equal(_host_eval(gc, x), want)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_host_conv_rescale_relu_flagship(name):
    """Conv2d -> Rescale -> Relu, k = 7, hardened, the flagship constructions: decoded == plain_q_eval."""
    rng = np.random.default_rng(5)
    c = conv_rescale_relu(rng, SHAPES[name])
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED, rescale="mrs", relu="joint", hardened=True)
    assert gc.hardened
    x = rng.integers(-20, 21, c.input_size)
    assert np.abs(c.layers[0].plain_q_eval(x, False)).max() < c.layers[1].mrs_limit(M7)
    np.testing.assert_array_equal(_host_eval(gc, x), gc.plain_q_eval(x))


# ---------------------------------------------------------------- 3. the wire format
def test_undilated_layers_keep_their_wire_bytes():
    """dh / dw are written only when > 1: an undilated layer's spec has neither, and its garbled model is byte for
    byte the blob the code before dilation wrote for the same circuit and seed (tests/golden)."""
    rng = np.random.default_rng(10)
    shape = undilated(SHAPES["d2_same"])
    cv = conv_layer(rng, shape)
    _, spec = cv.garble_spec()
    assert "dh" not in spec and "dw" not in spec
    _, spec1 = conv_layer(rng, SHAPES["k1_d2"]).garble_spec()  # moot dilation: the plain conv on the wire too
    assert "dh" not in spec1 and "dw" not in spec1
    _, specd = conv_layer(rng, SHAPES["unequal"]).garble_spec()
    assert specd["dh"] == 3 and "dw" not in specd
    c = d.Circuit([cv])
    for hardened in (True, False):  # the reference encoding's model also holds the bias labels
        blob = bytes(GarbledCircuit(c, 7, None, seed=SEED, hardened=hardened).model.serialize())
        back = native().GarbledModel.deserialize(blob)
        assert "dh" not in back.layer_params(0) and "dw" not in back.layer_params(0)
        old = (GOLDEN / f"conv_undilated_{'hardened' if hardened else 'reference'}_v5.bin").read_bytes()
        assert blob == old


@pytest.mark.parametrize("blob", ["dense_rescale_relu_maxpool_v5.bin", "rescale_clip_separate_v4.bin",
                                  "conv_undilated_hardened_v5.bin", "conv_undilated_reference_v5.bin"])
def test_committed_blobs_keep_loading(blob):
    """The wire version is unchanged: committed blobs load and re-serialize to their bytes."""
    old = (GOLDEN / blob).read_bytes()
    assert bytes(native().GarbledModel.deserialize(old).serialize()) == old


def test_dilated_model_roundtrips_and_evaluates():
    rng = np.random.default_rng(11)
    c = conv_rescale_relu(rng, SHAPES["unequal"])
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED, rescale="mrs", relu="joint", hardened=True)
    blob = gc.model.serialize()
    back = native().GarbledModel.deserialize(blob)
    assert bytes(back.serialize()) == bytes(blob)
    p0 = back.layer_params(0)
    assert [int(v) for v in p0["dh"]] == [3] and "dw" not in p0
    x = rng.integers(-20, 21, c.input_size)
    enc = gc.garble_inputs(x)
    a, b = gc.cpu_evaluate(enc), native().cpu_evaluate(back, enc, 0)
    for (pa, la), (pb, lb) in zip(a, b):
        assert pa == pb
        np.testing.assert_array_equal(la, lb)
    np.testing.assert_array_equal(gc.decode_outputs(b), gc.plain_q_eval(x))


# ---------------------------------------------------------------- 4. refusals
@pytest.mark.parametrize("bad,what", [(dict(dilation_height=0), "dilation"), (dict(dilation_width=0), "dilation"),
                                      (dict(dilation_width=-2), "dilation"), (dict(dilation_height=1.5), "dilation"),
                                      (dict(dilation_height=3), "empty output"),
                                      (dict(dilation_width=3, pad_width=1), "empty output")],
                         ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()) if isinstance(b, dict) else b)
def test_refusals(bad, what):
    """dh < 1, dw < 1 and an empty output (the effective kernel exceeds the padded 4 x 4 input), from the
    constructor and from from_quantized, with the layer's name."""
    kw = dict(input_width=4, input_height=4, channel=2, filter=2, filter_width=3, filter_height=3)
    kw.update(bad)
    w, b = np.zeros((2, 2, 3, 3)), np.zeros(2)
    with pytest.raises(ValueError, match=f"conv2d.*{what}"):
        d.Conv2d(w, b, **kw)
    with pytest.raises(ValueError, match=f"conv2d.*{what}"):
        d.Conv2d.from_quantized(w, b, **kw)


def test_native_refusals():
    """The native geometry (ConvGeom) refuses the same: a hand-made spec through the host garbler, and the planner
    bindings."""
    cv = d.Conv2d.from_quantized(np.ones((1, 1, 3, 3)), [0], 4, 4, 1, 1, 3, 3)
    kind, spec = cv.garble_spec()
    for extra, what in [(dict(dh=[0]), "dilation"), (dict(dw=[0]), "dilation"), (dict(dh=[2]), "empty output"),
                        (dict(dw=[5]), "empty output")]:
        specs = native().GarbleSpecs([(kind, dict(spec, **extra))])
        with pytest.raises(Exception, match=f"conv2d.*{what}"):
            native().Garbler(first_primes(7), [], SEED, 0).garble(specs, [1, 4, 4], 0, -1, True, False, False, False,
                                                                  None, False, False)
    for f, pre in ((native().hip_conv_plan, ()), (native().hip_conv_grp_plan, (2,))):
        geom = (2, 4, 4, 2, 3, 3, 1, 1, 0, 0)
        with pytest.raises(Exception, match="dilation"):
            f(*geom, *pre, first_primes(7), dh=0)
        with pytest.raises(Exception, match="empty output"):
            f(*geom, *pre, first_primes(7), dw=2)


def test_transposed_conv_and_pooling_still_refuse_dilation(tmp_path):
    from dash_amd.ir import onnx as o
    from dash_amd.ir.onnx import load_onnx_model

    with pytest.raises(ValueError, match="conv_transpose2d.*dilation"):
        d.ConvTranspose2d(np.zeros((2, 2, 3, 3)), np.zeros(2), 4, 4, 2, 2, 3, 3, dilation=2)
    attrs = o._attr_ints("kernel_shape", [2, 2]) + o._attr_ints("strides", [1, 1]) + o._attr_ints("dilations", [2, 2])
    path = _onnx_model(tmp_path / "pool.onnx", [o._node("MaxPool", ["input"], ["out"], "atrous_pool", attrs)], {},
                       (1, 2, 6, 6), "out", (1, 2, 4, 4))
    with pytest.raises(NotImplementedError, match="atrous_pool.*undilated"):
        load_onnx_model(path, Q.ScaleQuant, 10)
    ct = (o._attr_ints("kernel_shape", [3, 3]) + o._attr_ints("strides", [1, 1]) + o._attr_ints("dilations", [2, 2]))
    path = _onnx_model(tmp_path / "ct.onnx", [o._node("ConvTranspose", ["input", "w", "b"], ["out"], "atrous_up", ct)],
                       dict(w=np.zeros((2, 2, 3, 3), np.float32), b=np.zeros(2, np.float32)), (1, 2, 6, 6), "out",
                       (1, 2, 10, 10))
    with pytest.raises(NotImplementedError, match="atrous_up.*dilated"):
        load_onnx_model(path, Q.ScaleQuant, 10)


# ---------------------------------------------------------------- 5. ONNX
def _conv_node(name, k, dil=None, pads=None, strides=(1, 1), auto_pad=None, group=1):
    from dash_amd.ir import onnx as o

    a = o._attr_int("group", group) + o._attr_ints("kernel_shape", list(k)) + o._attr_ints("strides", list(strides))
    if dil is not None:
        a += o._attr_ints("dilations", list(dil))
    if pads is not None:
        a += o._attr_ints("pads", list(pads))
    if auto_pad is not None:
        a += o._attr_str("auto_pad", auto_pad)
    return o._node("Conv", ["input", "w", "b"], ["out"], name, a)


def test_onnx_export_import_reproduces_the_layer(tmp_path):
    from dash_amd.ir.onnx import load_onnx_model, parse_onnx, save_onnx_model

    rng = np.random.default_rng(20)
    layers, dims = [], (4, 8, 9)
    for name in ("unequal", "dw"):
        shape = (dims[2], dims[1], dims[0], 4, 3, 2, 2, 1, 1, 0, 1, 3, 1) if name == "unequal" else \
            (dims[2], dims[1], dims[0], 4, 3, 3, 1, 1, 2, 2, 2, 2, 4)
        wq, bq = weights(rng, shape)
        W, H, C, F, kh, kw, sw, sh, pw, ph, dw, dh, g = shape
        l = d.Conv2d(wq.astype(np.float32), bq.astype(np.float32), W, H, C, F, kw, kh, sw, sh, -1, Q.SimpleQuant, 1.0,
                     pad_width=pw, pad_height=ph, groups=g, dilation_width=dw, dilation_height=dh)
        layers += [l, d.Relu(l.out_dims)]
        dims = l.out_dims
    c = d.Circuit(layers)
    save_onnx_model(tmp_path / "dil.onnx", c)
    convs = [n for n in parse_onnx(tmp_path / "dil.onnx")["nodes"] if n["op_type"] == "Conv"]
    assert [[int(v) for v in n["attrs"]["dilations"]] for n in convs] == [[3, 1], [2, 2]]
    back = load_onnx_model(tmp_path / "dil.onnx", Q.SimpleQuant, -1, 1.0)
    got = [l for l in back.layers if isinstance(l, d.Conv2d)]
    assert [(l.dh, l.dw, l.groups, l.ph, l.pw, l.sh, l.sw) for l in got] == [(3, 1, 1, 0, 1, 1, 2), (2, 2, 4, 2, 2, 1, 1)]
    for a, b in zip([l for l in c.layers if isinstance(l, d.Conv2d)], got):
        np.testing.assert_array_equal(a.q_weights, b.q_weights)
        assert a.out_dims == b.out_dims
    x = rng.integers(-10, 11, c.input_size)
    np.testing.assert_array_equal(back.plain_q_eval(x, False), c.plain_q_eval(x, False))


def test_onnx_hand_built_dilated_conv(tmp_path):
    """A Conv node with dilations = [2, 3] (and explicit pads) against the same layer in PyTorch."""
    torch = pytest.importorskip("torch")
    from dash_amd.ir.onnx import load_onnx_model

    rng = np.random.default_rng(21)
    w, b = _f32(rng, 4, 3, 3, 3), _f32(rng, 4)
    path = _onnx_model(tmp_path / "d23.onnx", [_conv_node("atrous", (3, 3), dil=(2, 3), pads=(2, 1, 2, 1))],
                       dict(w=w, b=b), (1, 3, 8, 9), "out", (1, 4, 8, 5))
    c = load_onnx_model(path, Q.ScaleQuant, 10)
    cv = c.layers[0]
    assert (cv.dh, cv.dw, cv.ph, cv.pw) == (2, 3, 2, 1) and cv.out_dims == (4, 8, 5)
    for _ in range(3):
        x = _f32(rng, 3, 8, 9) * 4
        ref = torch.nn.functional.conv2d(torch.tensor(x)[None], torch.tensor(w), torch.tensor(b), padding=(2, 1),
                                         dilation=(2, 3))
        np.testing.assert_allclose(c.plain_eval(x.reshape(-1), track=False), ref.numpy().reshape(-1), rtol=1e-4,
                                   atol=1e-5)


def test_onnx_auto_pad(tmp_path):
    """VALID: no pads. SAME_UPPER of a 3x3 with dilation 2 at stride 1: total 4 per axis, pads (2, 2), against
    PyTorch's padding='same'. SAME_UPPER of a 3x3 at stride 2 on an even size: total 1, asymmetric, refused with
    the node's name; an unknown mode likewise."""
    torch = pytest.importorskip("torch")
    from dash_amd.ir.onnx import load_onnx_model

    rng = np.random.default_rng(22)
    w, b = _f32(rng, 2, 3, 3, 3), _f32(rng, 2)
    inits = dict(w=w, b=b)
    valid = load_onnx_model(_onnx_model(tmp_path / "v.onnx", [_conv_node("v", (3, 3), dil=(2, 2), auto_pad="VALID")],
                                        inits, (1, 3, 8, 8), "out", (1, 2, 4, 4)), Q.ScaleQuant, 10)
    assert (valid.layers[0].ph, valid.layers[0].pw) == (0, 0) and valid.layers[0].out_dims == (2, 4, 4)
    for mode in ("SAME_UPPER", "SAME_LOWER"):
        same = load_onnx_model(_onnx_model(tmp_path / "s.onnx", [_conv_node("s", (3, 3), dil=(2, 2), auto_pad=mode)],
                                           inits, (1, 3, 8, 7), "out", (1, 2, 8, 7)), Q.ScaleQuant, 10)
        cv = same.layers[0]
        assert (cv.ph, cv.pw, cv.dh, cv.dw) == (2, 2, 2, 2) and cv.out_dims == (2, 8, 7)
        x = _f32(rng, 3, 8, 7) * 4
        ref = torch.nn.functional.conv2d(torch.tensor(x)[None], torch.tensor(w), torch.tensor(b), padding="same",
                                         dilation=2)
        np.testing.assert_allclose(same.plain_eval(x.reshape(-1), track=False), ref.numpy().reshape(-1), rtol=1e-4,
                                   atol=1e-5)
    # stride 2 with an odd total (width 7: ceil(7 / 2) = 4 outputs need (4 - 1) 2 + 3 - 7 = 2, height 8: 1)
    bad = _onnx_model(tmp_path / "a.onnx", [_conv_node("lopsided", (3, 3), strides=(2, 2), auto_pad="SAME_UPPER")],
                      inits, (1, 3, 8, 7), "out", (1, 2, 4, 4))
    with pytest.raises(NotImplementedError, match="lopsided.*asymmetric"):
        load_onnx_model(bad, Q.ScaleQuant, 10)
    odd = _onnx_model(tmp_path / "o.onnx", [_conv_node("odd_mode", (3, 3), auto_pad="SAME")], inits, (1, 3, 8, 7),
                      "out", (1, 2, 8, 7))
    with pytest.raises(NotImplementedError, match="odd_mode.*auto_pad"):
        load_onnx_model(odd, Q.ScaleQuant, 10)


# ---------------------------------------------------------------- 6. trainer, guard, zoo
def test_train_mapping_of_dilation():
    torch = pytest.importorskip("torch")
    from dash_amd.models import zoo
    from dash_amd.models.train import build_torch_model, to_circuit

    zoo.ARCHS["_TINY_ATROUS"] = {"input": (2, 7, 7), "ops": [
        ("conv", 4, 3, 1, 2, 2), ("relu",), ("dwconv", 3, 1, 0, 2), ("relu",), ("conv", 2, 1, 1, 0)]}
    try:
        torch.manual_seed(0)
        m = build_torch_model("_TINY_ATROUS")
        m.fq.c = 0.0
        convs = [x for x in m if isinstance(x, torch.nn.Conv2d)]
        assert [x.dilation for x in convs] == [(2, 2), (2, 2), (1, 1)] and convs[1].groups == 4
        c = to_circuit(m, "_TINY_ATROUS", Q.ScaleQuant, 10)
        got = [l for l in c.layers if isinstance(l, d.Conv2d)]
        assert [(l.dh, l.dw, l.groups) for l in got] == [(2, 2, 1), (2, 2, 4), (1, 1, 1)]
        assert c.output_dims == (2, 3, 3)
        x = np.random.default_rng(5).uniform(-1, 1, (2, 7, 7)).astype(np.float32)
        with torch.no_grad():
            ref = m(torch.tensor(x)[None]).numpy().reshape(-1)
        np.testing.assert_allclose(c.plain_eval(x.reshape(-1), track=False), ref, rtol=1e-4, atol=1e-5)
        ref_c = zoo.build_circuit("_TINY_ATROUS", Q.ScaleQuant, 10)
        assert [(l.name, getattr(l, "dh", 0)) for l in ref_c.layers] == [(l.name, getattr(l, "dh", 0)) for l in c.layers]
        # a plain nn.Conv2d with unequal dilations maps too
        seq = torch.nn.Sequential(torch.nn.Conv2d(2, 3, (3, 2), dilation=(1, 3)))
        l = to_circuit(seq, "_TINY_ATROUS", Q.ScaleQuant, 10).layers[0]
        assert (l.dh, l.dw, l.out_dims) == (1, 3, (3, 5, 4))
    finally:
        del zoo.ARCHS["_TINY_ATROUS"]


def test_range_guard_on_a_dilated_circuit():
    pytest.importorskip("torch")
    c, xs = guard_case()
    g = RangeGuard(c, M7, mrs=True, device=None)
    assert g.batched and not g.native_forms and not g._native_ok()  # the batched torch path, as for ConvTranspose2d
    want = [bool(g.violations_np(x)) for x in xs]
    assert want == [False, True, True]
    assert g.submit(xs).bad_indices() == [1, 2]
    np.testing.assert_array_equal(g.outputs(xs[:1]), [c.plain_q_eval(xs[0], False, M7)])
    with pytest.raises(RangeGuardError):
        g.check(xs)
    # an undilated conv keeps the native forms
    plain = d.Circuit([conv_layer(np.random.default_rng(0), undilated(SHAPES["d2_same"]))])
    assert RangeGuard(plain, M7, mrs=True).native_forms
    # grouped and dilated through the torch path: the same outputs as numpy
    import torch

    rng = np.random.default_rng(2)
    c2 = d.Circuit([conv_layer(rng, SHAPES["grp2_d2_s2"])])
    x2 = [rng.integers(-20, 21, c2.input_size) for _ in range(3)]
    bad, out = RangeGuard(c2, M7, mrs=True)._bad_batch(torch.tensor(np.stack(x2)), want_out=True)
    assert not bool(bad.any())
    np.testing.assert_array_equal(out.cpu().numpy(), np.stack([c2.plain_q_eval(x, track=False) for x in x2]))


def test_zoo_aspp_seg_cifar():
    cfg, c, xs = aspp_seg()
    names = [l.name for l in c.layers]
    assert c.input_dims == (3, 32, 32) and c.output_dims == (1, 32, 32)
    assert names[-2:] == ["argmax", "upsample"] and names.count("concat") == 1
    convs = [l for l in c.layers if isinstance(l, d.Conv2d)]
    assert [(l.dh, l.ph) for l in convs] == [(1, 1), (1, 1), (1, 1), (2, 2), (4, 4), (1, 0), (1, 0)]
    branches = convs[2:5]
    assert all(l.out_dims == (16, 16, 16) for l in branches)
    assert branches[0].in_src is None and branches[1].in_src == branches[2].in_src  # all read the same tensor
    assert [l for l in c.layers if l.name == "concat"][0].out_dims == (48, 16, 16)
    assert c.infer_crt_base_size(xs) <= cfg["crt"]  # the quantised model fits its CRT base on the sample inputs
    for x in xs:
        y = c.plain_q_eval(x, False)
        assert y.shape == (32 * 32,) and set(np.unique(y)) <= {0, 1, 2, 3}


def test_zoo_aspp_seg_cifar_garbled_on_the_host():
    cfg, c, xs = aspp_seg()
    gc = GarbledCircuit(c, cfg["crt"], cfg["mrs"], seed=SEED, rescale="mrs")
    assert gc.hardened and gc.relu == "joint"
    np.testing.assert_array_equal(_host_eval(gc, xs[0]), gc.plain_q_eval(xs[0]))


def test_cli_infer_aspp_seg_cifar(capsys):
    from dash_amd.__main__ import main

    main(["infer", "--model", "ASPP_SEG_CIFAR", "--scheme", "DASH", "--backend", "cpu", "--inputs", "1"])
    assert "online time per inference" in capsys.readouterr().out


# ---------------------------------------------------------------- 7. the HIP planner (bindings; no device)
def _k7_plans():
    return {n: plan_of(native(), s, first_primes(7)) for n, s in SHAPES.items()}


def test_table_covers_every_dilated_form():
    """The planner decides the form: the table reaches the unrolled view, the forms with 1, 4 and 9 k-steps and the
    generic one, more than one band on both kernels, and every dilated instantiation."""
    plans = _k7_plans()
    forms = {n: form_of(SHAPES[n], p) for n, p in plans.items()}
    assert forms["d2_valid_rgb"] == "conv.img2d<1,1>" and plans["d2_valid_rgb"]["ur"] == 1
    assert plans["d2_valid_rgb"]["KS"] == 1 and plans["c64_k2_d3"]["KS"] == 4 and plans["c64_k3"]["KS"] == 9
    assert forms["c64_k2_d3"] == "conv.img2d<4,0>" and forms["c64_k3"] == "conv.img2d<9,0>"
    assert forms["c70_f20"] == "conv.img2d<0,0>" and plans["c70_f20"]["Cpad"] == 128 and plans["c70_f20"]["KS"] == 18
    assert forms["ur0_c20"] == "conv.img2d<0,1>" and plans["ur0_c20"]["KS"] == 3
    assert forms["two_bands_c64"] == "conv.img2d<9,0>" and plans["two_bands_c64"]["nbands"] > 1
    assert plans["dw_two_bands"]["gnbands"] > 1
    assert {forms[n] for n in DENSE if n != "k1_d2"} == \
        {"conv.img2d<1,1>", "conv.img2d<0,1>", "conv.img2d<9,0>", "conv.img2d<4,0>", "conv.img2d<0,0>"}
    assert {forms[n] for n in GROUPED} == {"conv.grpd<3,3,1>", "conv.grpd<3,3,2>", "conv.grpd<0,0,0>"}
    assert forms["grp_k2x5_d3"] == "conv.grpd<0,0,0>" and SHAPES["grp_k2x5_d3"][5] > 4
    # the same forms under the base [5, 7, 131]
    assert {n: form_of(SHAPES[n], plan_of(native(), SHAPES[n], B3)) for n in SHAPES} == forms


def test_moot_dilation_is_the_plain_conv():
    """A kernel axis of size 1: the layer stores dilation 1, and plans and names its form as the plain conv."""
    rng = np.random.default_rng(3)
    l = conv_layer(rng, SHAPES["k1_d2"])
    assert (l.dh, l.dw) == (1, 1) and l.out_dims == conv_layer(rng, undilated(SHAPES["k1_d2"])).out_dims
    a, b = plan_of(native(), SHAPES["k1_d2"], first_primes(7)), plan_of(native(), undilated(SHAPES["k1_d2"]), first_primes(7))
    assert a == b and a["dil"] == 0 and form_of(SHAPES["k1_d2"], a) == "conv.img2<1,0>"
    one_axis = d.Conv2d.from_quantized(np.ones((1, 1, 1, 3)), [0], 9, 3, 1, 1, 3, 1, dilation_width=2, dilation_height=5)
    assert (one_axis.dh, one_axis.dw) == (1, 2) and one_axis.garble_spec()[1].get("dh") is None


@pytest.mark.parametrize("name", DENSE)
def test_dense_band_fits_the_lds_budget(name):
    """The staged band (input rows x row stride, the launch's dynamic LDS) stays within the budget, and the input
    rows are the definition's: from the band's first tap to its last."""
    W, H, C, F, kh, kw, sw, sh, pw, ph, dw, dh, g = SHAPES[name]
    for crt in (first_primes(7), B3):
        p = plan_of(native(), SHAPES[name], crt)
        assert p["nbands"] >= 1 and p["band"] * p["nbands"] >= p["OH"]
        assert 0 < p["band_input_rows"] * p["ldsR"] <= LDS_BUDGET
        rows = min(p["band"], p["OH"])
        if p["ur"]:  # staged per output position
            assert p["band_input_rows"] == rows and p["ldsR"] >= p["OW"] * p["ldsS"]
        else:
            kdh = dh if kh > 1 else 1
            assert p["band_input_rows"] == (rows - 1) * sh + (kh - 1) * kdh + 1
            assert p["band_input_rows"] <= H + 2 * ph and p["ldsR"] >= (W + 2 * pw) * p["ldsS"]
        assert p["staged_bytes"] >= p["band_input_rows"] * p["ldsR"]


@pytest.mark.parametrize("name", GROUPED)
def test_grouped_band_fits_lds(name):
    """conv_grp_lds is at most 64 KiB, a row covers the furthest dword any lane reads ((kw - 1) dw past its last
    window), and the weights take one dword per tap."""
    W, H, C, F, kh, kw, sw, sh, pw, ph, dw, dh, g = SHAPES[name]
    p = plan_of(native(), SHAPES[name], first_primes(7))
    assert 0 < p["lds"] <= 64 * 1024
    OWq = -(-p["OW"] // 4)
    assert p["gR"] % 16 == 0 and p["gR"] >= W + 2 * pw
    assert p["gR"] >= 4 * (OWq - 1) * sw + 3 * sw + (kw - 1) * dw + 4
    assert p["kwd"] == kw and p["dil"] == 1
    assert p["band_input_rows"] == (p["gband"] - 1) * sh + (kh - 1) * dh + 1
    Cg, Fg = C // g, F // g
    assert p["lds"] == p["gpb"] * Cg * p["band_input_rows"] * p["gR"] + p["gpb"] * Fg * (Cg * kh * kw + 1) * 4
    # the undilated row keeps the packed weights
    q = plan_of(native(), undilated(SHAPES[name]), first_primes(7))
    assert q["dil"] == 0 and q["kwd"] == -(-kw // 4)


@pytest.mark.parametrize("c", CONV_CASES, ids=[c["name"] for c in CONV_CASES])
def test_plans_of_undilated_layers_are_unchanged(c):
    """hip_conv_plan(..., dh=1, dw=1) equals the call without them, for every row of the conv form table."""
    args = (c["C"], c["H"], c["W"], c["F"], c["kh"], c["kw"], c["sh"], c["sw"], c["ph"], c["pw"], c["crt"], True)
    a, b = native().hip_conv_plan(*args), native().hip_conv_plan(*args, dh=1, dw=1)
    assert a == b and a["dil"] == 0
    assert (a["ur"], a["KS"], a["band"], a["nbands"], a["sh24"]) == (c["ur"], c["KS"], c["band"], c["nbands"], c["sh24"])
