"""The Bilinear layer on the host (docs/BILINEAR.md): the weight tables against PyTorch's bilinear interpolation, the
edge cases of the tables, garbler + host evaluator bit-exact against plain_q_eval, the refusals, the wire format, ONNX
import / export, the range guard, the zoo models, the trainer's mapping and the command line. The GPU side is
tests/test_gpu_bilinear.py; circuits and inputs shared by both: tests/bilinear_cases.py."""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit, RangeGuard
from dash_amd.ir.quant import QuantizationMethod as Q
from dash_amd.native import native
from tests.bilinear_cases import (B3, M7, SEED, SHAPES, bilinear_argmax, bilinear_circuit, conv_bilinear_conv, inputs,
                                  layer, torch_bilinear)
from tests.test_clip import _conv_attrs, _f32, _onnx_model
from tests.test_conv_transpose import _host_eval, _resize_attrs, _with_i64_init


# ---------------------------------------------------------------- 1. weights against torch
@pytest.mark.parametrize("dims,kw,bits", [
    ((2, 3, 5), dict(factors=2), (2, 2)), ((2, 3, 5), dict(factors=4), (3, 3)),
    ((1, 3, 3), dict(size=(5, 5), mode="align_corners"), (1, 1)), ((3, 4, 2), dict(factors=(2, 4)), (2, 3))])
def test_dyadic_weights_equal_torch_exactly(dims, kw, bits):
    """Every lambda 2^b is an integer: plain_q_eval == 2^s F.interpolate in float64 with exact equality, and the
    default b is the minimal one."""
    pytest.importorskip("torch")
    l = d.Bilinear(dims, **kw)
    assert (l.by, l.bx) == bits and l.scale_bits == sum(bits)
    for b, n, m in ((l.by, l.H, l.OH), (l.bx, l.W, l.OW)):
        if b:  # one bit fewer loses a fraction
            assert d.Bilinear.axis_table(n, m, l.mode, 1)[3] == b
            lam = [(Fraction(2 * o + 1, 2) * Fraction(n, m) - Fraction(1, 2)) if l.mode == "half_pixel"
                   else Fraction(o * (n - 1), m - 1) for o in range(m)]
            assert any((v * (1 << (b - 1))).denominator != 1 for v in lam)
    rng = np.random.default_rng(1)
    for _ in range(3):
        x = rng.integers(-1000, 1001, l.in_size)
        want = torch_bilinear(x, l) * float(1 << l.scale_bits)
        got = l.plain_q_eval(x, False)
        assert got.dtype == np.int64 and np.array_equal(got.astype(np.float64), want)
        assert np.array_equal(l.plain_eval(x, False).astype(np.float64) * (1 << l.scale_bits), got)


@pytest.mark.parametrize("dims,kw,bits", [
    ((2, 3, 5), dict(factors=3), (6, 6)), ((1, 4, 4), dict(size=(7, 7), mode="align_corners"), (1, 1)),
    ((1, 4, 4), dict(size=(8, 7), mode="align_corners"), (6, 1)), ((2, 3, 5), dict(factors=3, bits=3), (3, 3)),
    ((1, 5, 3), dict(size=(7, 8), bits=8), (8, 4))])
def test_rounded_weights_stay_within_the_bound(dims, kw, bits):
    """Factor 3 and align_corners 4 -> 7 / 4 -> 8 (4 -> 7 has halves only and stays exact at b = 1; thirds and sevenths
    round to `bits`): the tap pairs sum to 2^b and |plain_eval - torch| <= 2^(1 - b) max|x|, b the smaller of the
    two axes' bits (each axis' weight error is at most 2^-(b + 1) with the pair sum kept: at most
    2 2^-(b + 1) max|x| per axis, so 2^-by + 2^-bx together)."""
    pytest.importorskip("torch")
    l = d.Bilinear(dims, **kw)
    assert (l.by, l.bx) == bits
    want_bits = min(bits)
    for b, n1 in ((l.by, l.ny), (l.bx, l.nx)):
        assert np.all((n1 >= 0) & (n1 <= (1 << b)))  # n0 = 2^b - n1 >= 0: the pair sums to 2^b by construction
    rng = np.random.default_rng(2)
    x = rng.uniform(-8, 8, l.in_size)
    err = np.abs(l.plain_eval(x, False).astype(np.float64) - torch_bilinear(x, l)).max()
    bound = (2.0 ** -l.by + 2.0 ** -l.bx) * np.abs(x).max() + 1e-5  # + float32 rounding
    print(f"{l}: max error {err:.6f}, bound {bound:.6f}")
    assert err <= bound <= 2.0 ** (1 - want_bits) * np.abs(x).max() + 1e-5
    # the integer formula is the same dyadic weights times 2^s
    xi = rng.integers(-50, 51, l.in_size)
    np.testing.assert_allclose(l.plain_q_eval(xi, False) / float(1 << l.scale_bits), l.plain_eval(xi, False), rtol=1e-6)


# ---------------------------------------------------------------- 2. edges
def test_table_edges():
    pytest.importorskip("torch")
    # H = 1: both row taps are row 0 and the row axis has b = 0 (every lambda is 0 after the clamp)
    l = d.Bilinear((2, 1, 4), 2)
    assert l.out_dims == (2, 2, 8) and l.by == 0 and list(l.y0) == list(l.y1) == [0, 0] and list(l.ny) == [0, 0]
    x = np.arange(8) * 3 - 7
    assert np.array_equal(l.plain_q_eval(x, False).astype(np.float64), torch_bilinear(x, l) * 4)
    # W = 1, a factor on the rows only
    l = d.Bilinear((2, 3, 1), (2, 1))
    assert l.out_dims == (2, 6, 1) and (l.by, l.bx) == (2, 0) and list(l.x0) == list(l.x1) == [0]
    x = np.arange(6) * 5 - 9
    assert np.array_equal(l.plain_q_eval(x, False).astype(np.float64), torch_bilinear(x, l) * 4)
    # clamped borders under half_pixel: the first and last output rows read one row (i0 == i1 at the far edge)
    l = d.Bilinear((1, 3, 3), 2)
    assert list(l.y0) == [0, 0, 0, 1, 1, 2] and list(l.y1) == [1, 1, 1, 2, 2, 2] and list(l.ny) == [0, 1, 3, 1, 3, 0]
    assert l.y0[-1] == l.y1[-1] == 2
    # output size 1 with align_corners: src = 0
    l = d.Bilinear((1, 3, 4), size=(1, 7), mode="align_corners")
    assert list(l.y0) == [0] and list(l.ny) == [0] and l.by == 0 and l.bx == 1
    x = np.arange(12) - 4
    assert np.array_equal(l.plain_q_eval(x, False).astype(np.float64), torch_bilinear(x, l) * 2)
    # asymmetric: src = o n / m, the last taps clamp to the last column
    l = d.Bilinear((1, 2, 2), 2, mode="asymmetric")
    assert list(l.x0) == [0, 0, 1, 1] and list(l.x1) == [1, 1, 1, 1] and list(l.nx) == [0, 1, 0, 1] and l.bx == 1
    # an axis whose size stays gets b = 0 and the identity taps
    l = d.Bilinear((1, 3, 2), size=(3, 4))
    assert l.by == 0 and list(l.y0) == [0, 1, 2] and list(l.ny) == [0, 0, 0]


def test_constructor_refusals():
    for bad, what in [(dict(dims=(4, 4), factors=2), r"\(C, H, W\)"), (dict(dims=(1, 4, 4), factors=2, mode="cubic"), "mode"),
                      (dict(dims=(1, 4, 4), factors=2, bits=0), "bits"), (dict(dims=(1, 4, 4), factors=2, bits=9), "bits"),
                      (dict(dims=(1, 4, 4), factors=1), "equals the input"),
                      (dict(dims=(1, 4, 4), size=(4, 4)), "equals the input"), (dict(dims=(1, 4, 4)), "factors or size"),
                      (dict(dims=(1, 4, 4), factors=2, size=(8, 8)), "factors or size"),
                      (dict(dims=(1, 3, 3), factors=1.5), "whole size")]:
        with pytest.raises(ValueError, match=what):
            d.Bilinear(**bad)
    assert d.Bilinear((1, 4, 4), 1.5).out_dims == (1, 6, 6)
    assert "Bilinear(in=(1, 4, 4), out=(1, 8, 8), mode=half_pixel, bits=(2, 2))" == repr(d.Bilinear((1, 4, 4), 2))
    assert d.Bilinear.kind == 24 and d.Bilinear.name == "bilinear"


def test_range_tracking_is_the_outputs_own():
    l = d.Bilinear((1, 2, 2), 2)
    x = np.array([100, -100, 50, 0])
    y = l.plain_q_eval(x)
    assert (l.get_min_plain_q_val(), l.get_max_plain_q_val()) == (int(y.min()), int(y.max())) == (-1600, 1600)


# ---------------------------------------------------------------- 3. host garbled
# Bilinear keywords on the (3, 4, 5) tensor behind the first conv; the non-dyadic ones at few bits, so that the
# 2^s-scaled values stay inside the small CRT ranges of these tests
KW = {"f2": dict(factors=2), "f3": dict(factors=3, bits=3), "corners": dict(size=(6, 7), mode="align_corners", bits=3),
      "rows_only": dict(factors=(2, 1)), "asym": dict(factors=2, mode="asymmetric")}


def _garbled_equals_plain(gc, c, rng, lim, M):
    assert gc.hardened
    bi = next(i for i, l in enumerate(c.layers) if l.name == "bilinear")
    assert dict(gc.model.layer_arrays(bi)) == {} and gc.model.layer_kind(bi) == 24  # no tables
    for _ in range(2):
        x = rng.integers(-lim, lim + 1, c.input_size)
        assert np.abs(c.plain_q_eval(x, False)).max() < M // 2
        np.testing.assert_array_equal(_host_eval(gc, x), gc.plain_q_eval(x))


@pytest.mark.parametrize("case", sorted(KW))
def test_garbled_conv_bilinear_conv_rescale_relu(case):
    """Garbler + host evaluator at k = 7 with the flagship constructions: decoded == plain_q_eval."""
    rng = np.random.default_rng(11)
    c = conv_bilinear_conv(rng, **KW[case])
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED, rescale="mrs", relu="joint", hardened=True)
    _garbled_equals_plain(gc, c, rng, 3, M7)


def test_garbled_bilinear_argmax():
    rng = np.random.default_rng(12)
    c = bilinear_argmax()
    _garbled_equals_plain(GarbledCircuit(c, 7, 100.0, seed=SEED, hardened=True), c, rng, 20, M7)


@pytest.mark.parametrize("case", sorted(KW))
def test_garbled_base_5_7_131(case):
    """The base (5, 7, 131) of tests/test_conv_transpose.py: a residue above 127, and tap weights that are zero mod 5
    and 7. No residue 2, hence no rescale and no ArgMax: conv -> bilinear."""
    rng = np.random.default_rng(13)
    kw = dict(KW[case], bits=2) if "bits" in KW[case] else KW[case]
    c = d.Circuit(list(conv_bilinear_conv(rng, **kw).layers[:2]))
    bl = c.layers[1]
    wts = [int(a) * int(b) for a in set(bl.ny) | {(1 << bl.by) - int(v) for v in bl.ny}
           for b in set(bl.nx) | {(1 << bl.bx) - int(v) for v in bl.nx}]
    assert any(w % 5 == 0 or w % 7 == 0 for w in wts)
    _garbled_equals_plain(GarbledCircuit(c, B3, None, seed=SEED, hardened=True), c, rng, 1, 5 * 7 * 131)


def test_bare_layer_has_no_tables_and_no_constants():
    c = bilinear_circuit("byte_f2x3")
    gc = GarbledCircuit(c, 7, None, seed=SEED)
    assert gc.hardened and gc.table_bytes == 0 and list(gc.model.const_names()) == []
    x = inputs(c, 1)[0]
    np.testing.assert_array_equal(_host_eval(gc, x), c.plain_q_eval(x, False))


# ---------------------------------------------------------------- 4. refusals
def test_reference_encoding_is_refused():
    c = d.Circuit([d.Relu((2, 3, 3)), d.Bilinear((2, 3, 3), 2)])
    with pytest.raises(ValueError, match=r"layer 1 \(bilinear\).*hardened"):
        GarbledCircuit(c, 7, 100.0, seed=SEED, hardened=False)
    with pytest.raises(ValueError, match=r"layer 1 \(bilinear\).*hardened"):
        GarbledCircuit(c, 7, 100.0, seed=SEED, fused_sign=False)
    bl = d.Bilinear((2, 3, 3), 2)
    with pytest.raises(Exception, match="hardened"):  # the native garbler refuses it too
        native().Garbler([2, 3, 5, 7, 11, 13, 17], [], SEED, 0).garble(
            d.Circuit([bl]).garble_specs_native(), list(bl.in_dims), 0, -1, True, False, False, False, None, False, False)


def test_native_geometry_validates_the_tables():
    bl = d.Bilinear((1, 3, 3), 2)
    g = native().Garbler([2, 3, 5, 7, 11, 13, 17], [], SEED, 0)
    for key, val, what in [("ny", [0, 1, 5, 1, 3, 0], "weight 5"), ("y1", [1, 1, 1, 2, 2, 3], "outside the input"),
                           ("x0", [0, 0, 0, 1, 1], "one entry per output"), ("by", [9], "fraction bits")]:
        kind, p = bl.garble_spec()
        p = dict(p)
        p[key] = np.asarray(val, dtype=np.int64)
        with pytest.raises(Exception, match=what):
            g.garble(native().GarbleSpecs([(kind, p)]), [1, 3, 3], 0, -1, True, False, False, False, None, True, False)


def test_zoo_refusals(monkeypatch):
    from dash_amd.models import zoo

    archs = {
        "_BL_OUT": [("conv", 2, 1, 1, 0), ("bilinear", 2)],                                       # a pending output
        "_BL_CAT": [("conv", 2, 1, 1, 0), ("relu",), ("skip",), ("bilinear", 2), ("cat",)],       # unequal bits
        "_BL_CLIP": [("conv", 2, 1, 1, 0), ("bilinear", 2), ("relu6",)],                          # a Clip with bits
    }
    for n, ops in archs.items():
        monkeypatch.setitem(zoo.ARCHS, n, {"input": (1, 4, 4), "ops": ops})
    with pytest.raises(NotImplementedError, match=r"output carries a pending 2\^4"):
        zoo.build_circuit("_BL_OUT", Q.ScaleQuant, 5)
    with pytest.raises(NotImplementedError, match=r"\(cat\).*2\^0.*2\^4.*equal bits"):
        zoo.build_circuit("_BL_CAT", Q.ScaleQuant, 5)
    with pytest.raises(NotImplementedError, match=r"\(relu6\).*2\^4"):
        zoo.build_circuit("_BL_CLIP", Q.ScaleQuant, 5)
    for scheme, param in [(Q.SimpleQuant, -1), (Q.ScaleQuantPlus, 32)]:
        with pytest.raises(ValueError, match=r"\(bilinear\).*ScaleQuant only"):
            zoo.build_circuit("_BL_OUT", scheme, param)


# ---------------------------------------------------------------- 5. wire format
def test_serialize_roundtrip():
    rng = np.random.default_rng(10)
    c = conv_bilinear_conv(rng, factors=3, bits=3)
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED, rescale="mrs", relu="joint")
    blob = gc.model.serialize()
    back = native().GarbledModel.deserialize(blob)
    assert bytes(back.serialize()) == bytes(blob)
    assert [back.layer_kind(i) for i in range(5)] == [1, 24, 1, 4, 2]
    bl = c.layers[1]
    p = {k: list(v) for k, v in back.layer_params(1).items()}
    assert p == dict(C=[3], H=[4], W=[5], OH=[12], OW=[15], by=[bl.by], bx=[bl.bx], y0=list(bl.y0), y1=list(bl.y1),
                     ny=list(bl.ny), x0=list(bl.x0), x1=list(bl.x1), nx=list(bl.nx))
    x = rng.integers(-3, 4, c.input_size)
    enc = gc.garble_inputs(x)
    a, b = gc.cpu_evaluate(enc), native().cpu_evaluate(back, enc, 0)
    for (pa, la), (pb, lb) in zip(a, b):
        assert pa == pb
        np.testing.assert_array_equal(la, lb)
    np.testing.assert_array_equal(gc.decode_outputs(b), gc.plain_q_eval(x))


# ---------------------------------------------------------------- 6. ONNX
def _resize_net(tmp_path, rng, node, extra_inits=None, i64=None, opset=11, out_hw=(8, 12)):
    """Conv 3x3 -> AveragePool 2 -> `node` (p -> u) -> Conv 1x1 on a (3, 8, 12) input."""
    from dash_amd.ir import onnx as o

    w1, b1, w2, b2 = _f32(rng, 4, 3, 3, 3), _f32(rng, 4), _f32(rng, 2, 4, 1, 1), _f32(rng, 2)
    inits = dict(w1=w1, b1=b1, w2=w2, b2=b2, **(extra_inits or {}))
    pool = o._attr_ints("kernel_shape", [2, 2]) + o._attr_ints("pads", [0] * 4) + o._attr_ints("strides", [2, 2])
    nodes = [o._node("Conv", ["input", "w1", "b1"], ["c"], "conv", _conv_attrs(3, 1, 1)),
             o._node("AveragePool", ["c"], ["p"], "pool", pool), node,
             o._node("Conv", ["u", "w2", "b2"], ["out"], "head", _conv_attrs(1))]
    path = tmp_path / "rs.onnx"
    _onnx_model(path, nodes, inits, (1, 3, 8, 12), "out", (1, 2) + tuple(out_hw), opset=opset)
    if i64 is not None:
        path.write_bytes(_with_i64_init(nodes, inits, i64[0], i64[1], (1, 3, 8, 12), "out", (1, 2) + tuple(out_hw), opset))
    return path, (w1, b1, w2, b2)


@pytest.mark.parametrize("form,ctm", [("scales", "half_pixel"), ("scales", None), ("scales", "pytorch_half_pixel"),
                                      ("scales", "align_corners"), ("scales", "asymmetric"), ("sizes", "half_pixel"),
                                      ("sizes", "align_corners"), ("frac_scales", "half_pixel"), ("upsample9", None)])
def test_onnx_import(tmp_path, form, ctm):
    """Conv -> AveragePool -> Resize(linear) -> Conv with resize="bilinear": the layer has the tables of the Bilinear
    built directly, its bits reach the second conv (in_scale_bits, Rescale(l + s)), the pending average factor passes
    through, and the float network equals PyTorch's. The default keyword refuses the same file by the node's name."""
    torch = pytest.importorskip("torch")
    from dash_amd.ir import onnx as o
    from dash_amd.ir.onnx import load_onnx_model

    F = torch.nn.functional
    rng = np.random.default_rng(24)
    attrs = _resize_attrs(ctm=ctm, nm=None, mode="linear")
    size, opset, i64, extra = (8, 12), 11, None, {}
    if form == "scales":
        extra["sc"] = np.asarray([1, 1, 2, 2], np.float32)
        node = o._node("Resize", ["p", "", "sc"], ["u"], "up", attrs)
    elif form == "frac_scales":
        extra["sc"] = np.asarray([1, 1, 1.5, 2.5], np.float32)
        size = (6, 15)
        node = o._node("Resize", ["p", "", "sc"], ["u"], "up", attrs)
    elif form == "sizes":
        size, i64 = (7, 9), ("sz", [1, 4, 7, 9])
        node = o._node("Resize", ["p", "", "", "sz"], ["u"], "up", attrs)
    else:
        opset = 9
        extra["sc"] = np.asarray([1, 1, 2, 2], np.float32)
        node = o._node("Upsample", ["p", "sc"], ["u"], "up", o._attr_str("mode", "linear"))
    path, (w1, b1, w2, b2) = _resize_net(tmp_path, rng, node, extra, i64, opset, size)
    with pytest.raises(NotImplementedError, match=r"up: (Resize|Upsample) mode 'linear'.*nearest only"):
        load_onnx_model(path, Q.ScaleQuant, 10)
    c = load_onnx_model(path, Q.ScaleQuant, 10, resize="bilinear")
    assert [l.name for l in c.layers] == ["conv2d", "rescale", "sum_pool", "bilinear", "conv2d", "rescale"]
    bl = c.layers[3]
    mode = "asymmetric" if form == "upsample9" else {None: "half_pixel", "pytorch_half_pixel": "half_pixel"}.get(ctm, ctm)
    ref = d.Bilinear((4, 4, 6), size=size, mode=mode)
    assert bl.mode == mode and bl.out_dims == (4,) + size and (bl.by, bl.bx) == (ref.by, ref.bx)
    for t in ("y0", "y1", "ny", "x0", "x1", "nx"):
        assert np.array_equal(getattr(bl, t), getattr(ref, t)), t
    assert c.layers[4].in_scale_bits == bl.scale_bits and c.layers[5].l == 10 + bl.scale_bits
    assert c.output_dims == (2,) + size
    if mode == "asymmetric":
        return  # PyTorch has no asymmetric bilinear mode: the tables above are the check
    for _ in range(2):
        x = _f32(rng, 3, 8, 12) * 4
        h = F.avg_pool2d(F.conv2d(torch.tensor(x)[None], torch.tensor(w1), torch.tensor(b1), padding=1), 2)
        h = F.interpolate(h, size=size, mode="bilinear", align_corners=mode == "align_corners")
        want = F.conv2d(h, torch.tensor(w2), torch.tensor(b2)).numpy().reshape(-1)
        got = c.plain_eval(x.reshape(-1), track=False)
        # dyadic tables are exact; 1.5 / 2.5 and the sizes 7 x 9 round to 6 bits: the layer is off by at most
        # 2^(1 - 6) max|h| (test_rounded_weights_stay_within_the_bound), which the 1x1 conv multiplies by a row's sum |w|
        tol = 0.0 if 6 not in (bl.by, bl.bx) else 2.0 ** -5 * float(h.abs().max()) * float(np.abs(w2).sum(axis=(1, 2, 3)).max())
        assert np.abs(got - want).max() <= tol + 1e-4 * max(1.0, np.abs(want).max()), (np.abs(got - want).max(), tol)


@pytest.mark.parametrize("case,what", [
    ("cubic", "mode 'cubic'"), ("no_const", "constant scales or sizes"), ("batch", r"scales.*\[1, 1, fh, fw\]"),
    ("channel", r"scales.*\[1, 1, fh, fw\]"), ("crop", "coordinate_transformation_mode"), ("ragged", "whole"),
    ("ones", "unchanged"), ("opset10", "opset"), ("php1", "pytorch_half_pixel")])
def test_onnx_refusals_by_node_name(tmp_path, case, what):
    from dash_amd.ir import onnx as o
    from dash_amd.ir.onnx import load_onnx_model

    sc, attrs, ins, opset = [1, 1, 2, 2], _resize_attrs(ctm="half_pixel", nm=None, mode="linear"), ["input", "", "sc"], 11
    ind, out = (1, 2, 3, 3), (1, 2, 6, 6)
    if case == "cubic":
        attrs = _resize_attrs(ctm="half_pixel", nm=None, mode="cubic")
    elif case == "no_const":
        ins = ["input", "", "dyn"]  # scales computed in the graph: no initializer of that name
    elif case == "batch":
        sc = [2, 1, 2, 2]
    elif case == "channel":
        sc = [1, 2, 2, 2]
    elif case == "crop":
        attrs = _resize_attrs(ctm="tf_crop_and_resize", nm=None, mode="linear")
    elif case == "ragged":
        sc = [1, 1, 1.5, 2]  # 3 * 1.5 is no whole size
    elif case == "ones":
        sc = [1, 1, 1, 1]
    elif case == "opset10":
        opset = 10
    elif case == "php1":
        attrs, sc, ind = _resize_attrs(ctm="pytorch_half_pixel", nm=None, mode="linear"), [1, 1, 0.5, 2], (1, 2, 2, 2)
    path = _onnx_model(tmp_path / "bad.onnx", [o._node("Resize", ins, ["out"], "head_resize", attrs)],
                       dict(sc=np.asarray(sc, np.float32)), ind, "out", out, opset=opset)
    with pytest.raises(NotImplementedError, match=f"head_resize.*{what}"):
        load_onnx_model(path, Q.ScaleQuant, 10, resize="bilinear")
    with pytest.raises(ValueError, match="resize must be"):
        load_onnx_model(path, Q.ScaleQuant, 10, resize="cubic")


def test_onnx_scheme_and_pending_bit_refusals(tmp_path):
    from dash_amd.ir import onnx as o
    from dash_amd.ir.onnx import load_onnx_model

    attrs = _resize_attrs(ctm="half_pixel", nm=None, mode="linear")
    sc = dict(sc=np.asarray([1, 1, 2, 2], np.float32))
    path = _onnx_model(tmp_path / "out.onnx", [o._node("Resize", ["input", "", "sc"], ["out"], "head_resize", attrs)],
                       sc, (1, 2, 3, 3), "out", (1, 2, 6, 6), opset=11)
    for scheme, param in [(Q.SimpleQuant, -1), (Q.ScaleQuantPlus, 32)]:
        with pytest.raises(ValueError, match="head_resize.*ScaleQuant only"):
            load_onnx_model(path, scheme, param, resize="bilinear")
    with pytest.raises(NotImplementedError, match="2\\^4"):  # a graph output with pending bits
        load_onnx_model(path, Q.ScaleQuant, 10, resize="bilinear")
    # Concat of the input (0 bits) with its resized self (4 bits): unequal bits
    nodes = [o._node("Resize", ["input", "", "sc"], ["u"], "up", attrs),
             o._node("Resize", ["input", "", "sc"], ["v"], "near", _resize_attrs()),
             o._node("Concat", ["u", "v"], ["out"], "join", o._attr_int("axis", 1))]
    path = _onnx_model(tmp_path / "cat.onnx", nodes, sc, (1, 2, 3, 3), "out", (1, 4, 6, 6), opset=11)
    with pytest.raises(NotImplementedError, match="join"):
        load_onnx_model(path, Q.ScaleQuant, 10, resize="bilinear")


@pytest.mark.parametrize("name", ["UNET_BILINEAR_CIFAR", "DEEPLAB_HEAD_CIFAR"])
def test_onnx_export_import_roundtrip(tmp_path, name):
    from dash_amd.ir.onnx import load_onnx_model, parse_onnx, save_onnx_model
    from dash_amd.models import build_circuit, quantized_inputs

    c = build_circuit(name, Q.ScaleQuant, 5, seed=0)
    save_onnx_model(tmp_path / "m.onnx", c)
    rs = [n for n in parse_onnx(tmp_path / "m.onnx")["nodes"] if n["op_type"] == "Resize"]
    assert len(rs) == sum(l.name == "bilinear" for l in c.layers) >= 1
    assert all(n["attrs"]["mode"] in ("linear", b"linear") for n in rs)
    with pytest.raises(NotImplementedError, match="bilinear_.*nearest only"):
        load_onnx_model(tmp_path / "m.onnx", Q.ScaleQuant, 5)
    back = load_onnx_model(tmp_path / "m.onnx", Q.ScaleQuant, 5, resize="bilinear")
    assert [l.name for l in back.layers] == [l.name for l in c.layers]
    for a, b in zip(c.layers, back.layers):
        if a.name == "bilinear":
            assert all(np.array_equal(getattr(a, t), getattr(b, t)) for t in ("y0", "y1", "ny", "x0", "x1", "nx"))
            assert (a.by, a.bx, a.mode) == (b.by, b.bx, b.mode)
    for x in quantized_inputs(name, 2, Q.ScaleQuant, 5, seed=1):
        np.testing.assert_array_equal(back.plain_q_eval(x, False), c.plain_q_eval(x, False))


def test_onnx_export_keeps_every_mode(tmp_path):
    from dash_amd.ir.onnx import load_onnx_model, save_onnx_model

    for mode, kw in [("align_corners", dict(size=(7, 8))), ("asymmetric", dict(factors=2)), ("half_pixel", dict(factors=1.5))]:
        rng = np.random.default_rng(3)
        c1 = d.Conv2d(_f32(rng, 2, 2, 1, 1), _f32(rng, 2), 4, 4, 2, 2, 1, 1, 1, 1, 5, Q.ScaleQuant)
        bl = d.Bilinear((2, 4, 4), mode=mode, **kw)
        c2 = d.Conv2d(_f32(rng, 2, 2, 1, 1), _f32(rng, 2), bl.OW, bl.OH, 2, 2, 1, 1, 1, 1, 5, Q.ScaleQuant,
                      in_scale_bits=bl.scale_bits)
        c = d.Circuit([c1, d.Rescale(5, c1.out_dims), bl, c2, d.Rescale(5 + bl.scale_bits, c2.out_dims)])
        save_onnx_model(tmp_path / "m.onnx", c)
        back = load_onnx_model(tmp_path / "m.onnx", Q.ScaleQuant, 5, resize="bilinear")
        b2 = back.layers[2]
        assert (b2.mode, b2.by, b2.bx, b2.out_dims) == (mode, bl.by, bl.bx, bl.out_dims)
        x = rng.integers(-40, 41, c.input_size)
        np.testing.assert_array_equal(back.plain_q_eval(x, False), c.plain_q_eval(x, False))


# ---------------------------------------------------------------- 7. range guard
def test_range_guard_paths_agree():
    pytest.importorskip("torch")
    rng = np.random.default_rng(42)
    c = conv_bilinear_conv(rng, factors=2)
    c.calibrate([rng.integers(-6, 7, c.input_size) for _ in range(4)], M7)
    g = RangeGuard(c, M7, mrs=True, device=None)
    assert g.batched and not g.native_forms and not g._native_ok()
    ys = [rng.integers(-6, 7, c.input_size), np.full(c.input_size, M7 // 64), rng.integers(-6, 7, c.input_size)]
    want = [i for i, y in enumerate(ys) if g.violations_np(y)]
    assert want == [1] and g.submit(ys).bad_indices() == want
    np.testing.assert_array_equal(g.outputs([ys[0], ys[2]]), [c.plain_q_eval(y, False, M7) for y in (ys[0], ys[2])])
    # the bare layer: exact int64 on values that float32 / float64 interpolation would round
    c2 = d.Circuit([d.Bilinear((2, 3, 5), size=(7, 9), mode="align_corners"), d.Relu((2, 7, 9))])
    g2 = RangeGuard(c2, 2 ** 61 - 1, mrs=False, device=None)
    big = [rng.integers(-2 ** 45, 2 ** 45, c2.input_size) for _ in range(2)]
    np.testing.assert_array_equal(g2.outputs(big), [c2.plain_q_eval(y, False) for y in big])


# ---------------------------------------------------------------- 8. zoo, training, command line
def _zoo(name):
    from dash_amd.models import BENCH_CONFIGS, build_circuit, quantized_inputs

    cfg = BENCH_CONFIGS[f"{name}/DASH"]
    assert (cfg["model"], cfg["q_method"], cfg["q_parameter"], cfg["crt"], cfg["mrs"]) == (name, Q.ScaleQuant, 5, 7, 100.0)
    c = build_circuit(name, cfg["q_method"], cfg["q_parameter"], seed=0)
    return cfg, c, quantized_inputs(name, 2, cfg["q_method"], cfg["q_parameter"], seed=7)


def test_zoo_models_build_and_run_plain():
    from dash_amd.ir.quant import quantize_input
    from dash_amd.models import synthetic_inputs

    _, u, _ = _zoo("UNET_BILINEAR_CIFAR")
    names = [l.name for l in u.layers]
    assert u.input_dims == (3, 32, 32) and u.output_dims == (1, 32, 32) and names[-1] == "argmax"
    assert names.count("bilinear") == 2 and names.count("concat") == 2 and "conv_transpose2d" not in names
    for i, l in enumerate(u.layers):
        if l.name == "bilinear":  # the up-conv: the conv absorbs the 4 pending bits, the rescale takes them out
            assert l.scale_bits == 4 and u.layers[i + 1].in_scale_bits == 4 and u.layers[i + 2].l == 5 + 4
            assert [x.name for x in u.layers[i + 1:i + 5]] == ["conv2d", "rescale", "approx_relu", "concat"]
    _, h, _ = _zoo("DEEPLAB_HEAD_CIFAR")
    names = [l.name for l in h.layers]
    assert names[-3:] == ["rescale", "bilinear", "argmax"] and h.output_dims == (1, 32, 32)
    assert h.layers[-2].in_dims == (4, 16, 16) and h.layers[-2].out_dims == (4, 32, 32)
    for name, c in (("UNET_BILINEAR_CIFAR", u), ("DEEPLAB_HEAD_CIFAR", h)):
        agree = []
        for xf in synthetic_inputs(name, 3, seed=3):
            yq = c.plain_q_eval(quantize_input(xf, Q.ScaleQuant, 5, 0.02), False)
            assert set(np.unique(yq)) <= {0, 1, 2, 3}
            agree.append(float(np.mean(yq == c.plain_eval(xf, False))))
        assert min(agree) > 0.8, (name, agree)


@pytest.mark.parametrize("name", ["UNET_BILINEAR_CIFAR", "DEEPLAB_HEAD_CIFAR"])
def test_zoo_models_garbled_on_the_host(name):
    cfg, c, xs = _zoo(name)
    c.calibrate(xs, M7)
    assert c.required_crt_modulus() <= M7
    gc = GarbledCircuit(c, cfg["crt"], cfg["mrs"], seed=SEED, rescale="mrs")
    assert gc.hardened and gc.relu == "joint"
    y = _host_eval(gc, xs[0])
    np.testing.assert_array_equal(y, gc.plain_q_eval(xs[0]))
    assert y.shape == (32 * 32,)


def test_train_mapping():
    torch = pytest.importorskip("torch")
    from dash_amd.models import zoo
    from dash_amd.models.train import build_torch_model, to_circuit

    for mode in ("half_pixel", "align_corners"):
        zoo.ARCHS["_TINY_UPCONV"] = {"input": (2, 4, 4), "ops": [
            ("conv", 3, 3, 1, 1), ("relu",), ("bilinear", 2, mode), ("conv", 2, 3, 1, 1)]}
        try:
            torch.manual_seed(0)
            m = build_torch_model("_TINY_UPCONV")
            assert any(isinstance(x, torch.nn.Upsample) and x.mode == "bilinear" for x in m)
            c = to_circuit(m, "_TINY_UPCONV", Q.ScaleQuant, 10)
            assert [l.name for l in c.layers] == ["conv2d", "rescale", "approx_relu", "bilinear", "conv2d", "rescale"]
            s = c.layers[3].scale_bits
            assert c.layers[3].mode == mode and c.layers[4].in_scale_bits == s and c.layers[5].l == 10 + s
            x = np.random.default_rng(5).uniform(-1, 1, (2, 4, 4)).astype(np.float32)
            with torch.no_grad():
                ref = m(torch.tensor(x)[None]).numpy().reshape(-1)
                h = m[:2](torch.tensor(x)[None])
            # 4 -> 8 with align_corners rounds to 6 bits: the layer is off by at most 2^(1 - 6) max|h|, which the conv
            # multiplies by a filter's sum |w|; half_pixel by 2 is exact
            tol = 1e-5 if mode == "half_pixel" else \
                2.0 ** -5 * float(h.abs().max()) * float(m[3].weight.detach().abs().sum(dim=(1, 2, 3)).max())
            np.testing.assert_allclose(c.plain_eval(x.reshape(-1), track=False), ref, rtol=1e-4, atol=tol + 1e-5)
            ref_c = zoo.build_circuit("_TINY_UPCONV", Q.ScaleQuant, 10)
            assert [l.name for l in ref_c.layers] == [l.name for l in c.layers]
        finally:
            del zoo.ARCHS["_TINY_UPCONV"]


def test_cli_infer_deeplab_head(capsys):
    from dash_amd.__main__ import main

    main(["infer", "--model", "DEEPLAB_HEAD_CIFAR", "--scheme", "DASH", "--backend", "cpu", "--inputs", "1"])
    out = capsys.readouterr().out
    assert "Bilinear" in out and "ArgMax" in out and "garbled==plaintext: True" in out
