"""The Gather layer on the host (docs/GATHER.md): the constructors against numpy, the refusals, the wire image, the
host garbler and evaluator against the plaintext model for every case the GPU suite runs, ONNX import / export, the
zoo's shuffle unit and sub-pixel head, the range guard and the trainer's refusal. Circuits and inputs:
tests/gather_cases.py. The GPU side is tests/test_gpu_gather.py."""
from __future__ import annotations

import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit, RangeGuard
from dash_amd.ir.quant import QuantizationMethod as Q
from dash_amd.native import native
from tests.gather_cases import (BYTE, DWORD, M7, SHAPES, argmax_case, gather_circuit, gather_index, gather_inputs,
                                in_src_case, numpy_pixel_shuffle, numpy_shuffle_unit, repeats_relu_case,
                                shuffle_unit_case)
from tests.test_clip import _conv_attrs, _f32

SEED = bytes(range(16))


def _host_eval(gc, x):
    return gc.decode_outputs(gc.cpu_evaluate(gc.garble_inputs(x)))


def _apply(l, x):
    """The layer on an integer tensor of its input dims, as a tensor of its output dims."""
    return l.plain_q_eval(np.asarray(x).reshape(-1), False).reshape(l.out_dims)


# ---------------------------------------------------------------- 1. the layer and its constructors
def test_semantics():
    idx = np.array([3, 3, 0, 5])
    l = d.Gather((2, 3), idx)
    assert (l.kind, l.name, d.Gather.kind) == (23, "gather", 23)
    assert l.in_dims == (2, 3) and l.out_dims == (4,)
    x = np.array([10, -20, 30, -40, 50, -60])
    out = l.plain_q_eval(x, False)
    assert out.dtype == np.int64
    np.testing.assert_array_equal(out, [-40, -40, 10, -60])
    f = l.plain_eval(x.astype(np.float64), False)
    assert f.dtype == np.float32
    np.testing.assert_array_equal(f, [-40, -40, 10, -60])
    assert d.Gather((2, 3), idx, (2, 2)).out_dims == (2, 2)
    kind, p = l.garble_spec()
    assert kind == 23 and set(p) == {"idx", "od"} and list(p["idx"]) == [3, 3, 0, 5] and list(p["od"]) == [4]
    # value-preserving and range-tracked like any layer
    l.plain_q_eval(x)
    assert (l.get_min_plain_q_val(), l.get_max_plain_q_val()) == (-60, 10)
    assert repr(l) == "Gather(in=(2, 3), out=(4,))"


@pytest.mark.parametrize("dims,perm", [((2, 3, 4), (0, 2, 1)), ((2, 3, 4), (2, 0, 1)), ((5, 7), (1, 0)), ((6,), (0,)),
                                       ((2, 3, 4, 5), (3, 1, 0, 2))])
def test_transpose(dims, perm):
    x = np.random.default_rng(0).integers(-99, 100, dims)
    l = d.Gather.transpose(dims, perm)
    assert l.out_dims == tuple(dims[p] for p in perm)
    np.testing.assert_array_equal(_apply(l, x), np.transpose(x, perm))


@pytest.mark.parametrize("axis,start,stop,step", [(0, 0, 2, 1), (0, 2, 4, 1), (1, 1, 5, 2), (2, -3, -1, 1), (2, -100, 3, 1),
                                                  (1, 2, 2 ** 63 - 1, 1), (-1, 1, 100, 3), (-3, -1, 9, 1), (1, 0, 6, 5)])
def test_slice(axis, start, stop, step):
    dims = (4, 6, 5)
    x = np.random.default_rng(1).integers(-99, 100, dims)
    sl = [slice(None)] * 3
    sl[axis] = slice(start, stop, step)  # Python's slicing has ONNX's negative-index and clamping rules
    want = x[tuple(sl)]
    l = d.Gather.slice(dims, axis, start, stop, step)
    assert l.out_dims == want.shape
    np.testing.assert_array_equal(_apply(l, x), want)


@pytest.mark.parametrize("g", [1, 2, 3, 6])
def test_channel_shuffle(g):
    dims = (6, 2, 3)
    x = np.random.default_rng(2).integers(-99, 100, dims)
    l = d.Gather.channel_shuffle(dims, g)
    assert l.out_dims == dims
    # torch.nn.ChannelShuffle: view (g, C / g, H, W), swap the first two axes, flatten
    np.testing.assert_array_equal(_apply(l, x), x.reshape(g, 6 // g, 2, 3).transpose(1, 0, 2, 3).reshape(dims))
    out = _apply(l, x)
    for c in range(6):  # output channel c = input channel (c % g) (C / g) + c // g
        np.testing.assert_array_equal(out[c], x[(c % g) * (6 // g) + c // g])


@pytest.mark.parametrize("mode", ["DCR", "CRD"])
@pytest.mark.parametrize("r,dims", [(2, (8, 3, 2)), (3, (9, 2, 2)), (1, (3, 2, 2))])
def test_depth_to_space(mode, r, dims):
    C, H, W = dims
    x = np.random.default_rng(3).integers(-99, 100, dims)
    c = C // (r * r)
    if mode == "DCR":  # the ONNX operator's definition, with the batch axis
        t = x.reshape(1, r, r, c, H, W).transpose(0, 3, 4, 1, 5, 2)
    else:
        t = x.reshape(1, c, r, r, H, W).transpose(0, 1, 4, 2, 5, 3)
    want = t.reshape(c, H * r, W * r)
    l = d.Gather.depth_to_space(dims, r, mode)
    assert l.out_dims == (c, H * r, W * r)
    np.testing.assert_array_equal(_apply(l, x), want)
    if mode == "CRD":
        np.testing.assert_array_equal(want, numpy_pixel_shuffle(x, r))


@pytest.mark.parametrize("r,dims", [(2, (3, 4, 6)), (3, (2, 3, 6)), (1, (2, 2, 2))])
def test_space_to_depth_and_back(r, dims):
    C, H, W = dims
    x = np.random.default_rng(4).integers(-99, 100, dims)
    s = d.Gather.space_to_depth(dims, r)
    want = x.reshape(1, C, H // r, r, W // r, r).transpose(0, 3, 5, 1, 2, 4).reshape(C * r * r, H // r, W // r)
    np.testing.assert_array_equal(_apply(s, x), want)
    back = d.Gather.depth_to_space(s.out_dims, r)  # DCR is its inverse
    np.testing.assert_array_equal(_apply(back, _apply(s, x)), x)
    np.testing.assert_array_equal(back.idx[s.idx], np.arange(x.size))


def test_value_errors():
    with pytest.raises(ValueError, match="empty"):
        d.Gather((4,), np.zeros(0, dtype=np.int64))
    with pytest.raises(ValueError, match=r"idx\[2\] = -1.*negative"):
        d.Gather((4,), [0, 1, -1, -2])
    with pytest.raises(ValueError, match=r"idx\[1\] = 4.*4"):
        d.Gather((4,), [3, 4, 9])
    with pytest.raises(ValueError, match=r"idx\[0\] = 6"):
        d.Gather((2, 3), [6])
    with pytest.raises(ValueError, match="out_dims"):
        d.Gather((4,), [0, 1, 2], (2, 2))
    with pytest.raises(ValueError, match="1-D integer"):
        d.Gather((4,), [[0, 1], [2, 3]])
    with pytest.raises(ValueError, match="1-D integer"):
        d.Gather((4,), [0.5, 1.0])
    with pytest.raises(ValueError, match="perm"):
        d.Gather.transpose((2, 3), (0, 0))
    with pytest.raises(ValueError, match="step"):
        d.Gather.slice((4,), 0, 3, 0, -1)
    with pytest.raises(ValueError, match="step"):
        d.Gather.slice((4,), 0, 0, 4, 0)
    with pytest.raises(ValueError, match="axis"):
        d.Gather.slice((4,), 1, 0, 4)
    with pytest.raises(ValueError, match="empty slice"):
        d.Gather.slice((4,), 0, 3, 3)
    with pytest.raises(ValueError, match="groups"):
        d.Gather.channel_shuffle((6, 2, 2), 4)
    with pytest.raises(ValueError, match="depth_to_space"):
        d.Gather.depth_to_space((6, 2, 2), 2)
    with pytest.raises(ValueError, match="mode"):
        d.Gather.depth_to_space((4, 2, 2), 2, "XYZ")
    with pytest.raises(ValueError, match="space_to_depth"):
        d.Gather.space_to_depth((2, 3, 4), 2)


def test_native_garbler_checks_the_map_too():
    """A map that did not pass the layer's constructor: the native garbler names the first offending position."""
    for idx, msg in (([0, 5], "index 5 at position 1"), ([-1, 0], "index -1 at position 0")):
        l = d.Gather((4,), [0, 1])
        l.idx = np.asarray(idx, dtype=np.int64)  # behind the constructor's back
        with pytest.raises(Exception, match=msg):
            GarbledCircuit(d.Circuit([l]), 3, None, seed=SEED)


# ---------------------------------------------------------------- 2. wire image
def test_wire_image_and_serialize_roundtrip():
    c = gather_circuit("odd3")
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED)
    m = gc.model
    assert m.layer_kind(0) == 23 and native().kind_name(23) == "gather"
    p = m.layer_params(0)
    assert set(p) == {"idx", "od"} and list(p["idx"]) == list(gather_index("odd3")) and list(p["od"]) == [3]
    assert not m.layer_arrays(0) and gc.table_bytes == 0  # free: no tables
    blob = m.serialize()
    back = native().GarbledModel.deserialize(blob)
    assert bytes(back.serialize()) == bytes(blob)
    x = gather_inputs("odd3")[0]
    enc = gc.garble_inputs(x)
    for (pa, la), (pb, lb) in zip(gc.cpu_evaluate(enc), native().cpu_evaluate(back, enc, 0)):
        assert pa == pb
        np.testing.assert_array_equal(la, lb)
    # out_dims reach the model's header
    g2 = GarbledCircuit(d.Circuit([d.Gather.transpose((2, 3, 4), (2, 0, 1))]), 7, 100.0, seed=SEED)
    assert list(g2.model.layer_params(0)["od"]) == [4, 2, 3] and tuple(g2.circuit.output_dims) == (4, 2, 3)


# ---------------------------------------------------------------- 3. host garbler and evaluator
@pytest.mark.parametrize("hardened", [True, False], ids=["hardened", "reference"])
@pytest.mark.parametrize("name", DWORD + BYTE)
def test_host_garble_and_evaluate(name, hardened):
    c = gather_circuit(name)
    idx = gather_index(name)
    assert (c.input_size, c.output_size) == SHAPES[name]
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED, hardened=hardened)
    assert gc.hardened == hardened
    for x in gather_inputs(name, rounds=3):
        y = _host_eval(gc, x)
        np.testing.assert_array_equal(y, c.plain_q_eval(x, False, M7))
        np.testing.assert_array_equal(y, x[idx])
    # the zero labels moved: output wire o carries input wire idx[o]'s label, component for component
    enc = gc.garble_inputs(gather_inputs(name)[0])
    for (p, a), (q, b) in zip(enc, gc.cpu_evaluate(enc)):
        assert p == q
        np.testing.assert_array_equal(b, np.asarray(a)[idx])


@pytest.mark.parametrize("hardened", [True, False], ids=["hardened", "reference"])
@pytest.mark.parametrize("case", [in_src_case, repeats_relu_case], ids=["in_src", "repeats_relu"])
def test_host_composites(case, hardened):
    c, xs, want = case()
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED, hardened=hardened)
    for x in xs:
        y = _host_eval(gc, x)
        np.testing.assert_array_equal(y, c.plain_q_eval(x, False, M7))
        np.testing.assert_array_equal(y, want(x))


def test_host_behind_an_argmax():
    c, xs, want = argmax_case()
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED)  # an ArgMax exists in the hardened encoding only
    for x in xs:
        y = _host_eval(gc, x)
        np.testing.assert_array_equal(y, c.plain_q_eval(x, False, M7))
        np.testing.assert_array_equal(y, want(x))


@pytest.mark.parametrize("hardened", [True, False], ids=["hardened", "reference"])
def test_host_shuffle_unit(hardened):
    c, xs = shuffle_unit_case()
    assert [l.name for l in c.layers] == ["gather", "gather", "conv2d", "rescale", "approx_relu", "conv2d", "rescale",
                                          "conv2d", "rescale", "approx_relu", "concat", "gather"]
    assert [l.in_src for l in c.layers[:3]] == [None, -1, None]
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED, hardened=hardened)
    for x in xs[:3]:
        np.testing.assert_array_equal(_host_eval(gc, x), c.plain_q_eval(x, False, M7))


def test_every_copy_has_its_own_gate():
    """Behind a Gather with repeats the ReLU garbles one gate per output element, as behind an Upsample: 12 rows of
    tables for 5 inputs, and the copies of one input (wires 0, 1, 9: input 0) get different tables."""
    c, xs, _ = repeats_relu_case()
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED)
    arrs = gc.model.layer_arrays(1)
    assert arrs and all(np.asarray(a).shape[0] == 12 for a in arrs.values())
    solo = GarbledCircuit(d.Circuit([d.Relu((5,))]), 7, 100.0, seed=SEED).model.layer_arrays(0)
    assert all(np.asarray(a).shape[0] == 5 for a in solo.values())
    for a in arrs.values():
        a = np.asarray(a)
        assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[0], a[9])


# ---------------------------------------------------------------- 4. ONNX
def _model(path, nodes, inits, in_dims, out_name, out_dims, opset=13):
    """tests/test_clip.py's _onnx_model with integer initializers written as int64 tensors."""
    from dash_amd.ir import onnx as o

    def tensor(n, v):
        v = np.asarray(v)
        if v.ndim == 0 and np.issubdtype(v.dtype, np.integer):  # a scalar: a TensorProto without dims
            return o._i(2, 7) + o._s(8, n) + o._ld(9, v.astype(np.int64).tobytes())
        return o._tensor_i64(n, v) if np.issubdtype(v.dtype, np.integer) else o._tensor(n, v)

    graph = b"".join(nodes) + o._s(2, "g") + b"".join(o._ld(5, tensor(n, v)) for n, v in inits.items())
    graph += o._ld(11, o._value_info("input", in_dims)) + o._ld(12, o._value_info(out_name, out_dims))
    path.write_bytes(o._i(1, 7) + o._s(2, "test") + o._s(3, "1") + o._ld(7, graph) + o._ld(8, o._s(1, "") + o._i(2, opset)))
    return path


def _load(path, **kw):
    from dash_amd.ir.onnx import load_onnx_model

    return load_onnx_model(path, Q.ScaleQuant, 5, **kw)


def _conv_front(rng, cin=2, cout=4):
    """A 1x1 conv in front, so that the operator under test reads a produced tensor."""
    from dash_amd.ir import onnx as o

    inits = {"w": _f32(rng, cout, cin, 1, 1), "b": _f32(rng, cout)}
    return [o._node("Conv", ["input", "w", "b"], ["a"], "c0", _conv_attrs(1))], inits


def _conv_ref(inits, x, cin, hw):
    return (inits["w"].reshape(-1, cin) @ x.reshape(cin, hw) + inits["b"][:, None])


def _single(tmp_path, node, extra_inits, out_dims, in_dims=(1, 2, 4, 4), opset=13, **kw):
    rng = np.random.default_rng(8)
    nodes, inits = _conv_front(rng)
    inits.update(extra_inits)
    c = _load(_model(tmp_path / "m.onnx", nodes + [node], inits, in_dims, "y", out_dims, opset), **kw)
    x = rng.uniform(-1, 1, int(np.prod(in_dims))).astype(np.float32)
    a = _conv_ref(inits, x, 2, 16).reshape(4, 4, 4)
    return c, a, c.plain_eval(x, False)


def test_onnx_slice(tmp_path):
    from dash_amd.ir import onnx as o

    # opset >= 10: inputs; two axes at once, a negative start, an end beyond the axis, a step
    node = o._node("Slice", ["a", "st", "en", "ax", "sp"], ["y"], "sl")
    c, a, y = _single(tmp_path, node, {"st": np.array([1, -3]), "en": np.array([2 ** 62, 100]), "ax": np.array([1, 3]),
                                       "sp": np.array([2, 1])}, (1, 2, 4, 3))
    assert [l.name for l in c.layers] == ["conv2d", "rescale", "gather"] and c.output_dims == (2, 4, 3)
    np.testing.assert_allclose(y, a[1::2, :, -3:].reshape(-1), rtol=1e-5, atol=1e-6)
    # without axes and steps: starts / ends cover the leading axes, the batch axis included, which is refused
    with pytest.raises(NotImplementedError, match="sl0.*batch axis"):
        _single(tmp_path, o._node("Slice", ["a", "st", "en"], ["y"], "sl0"), {"st": np.array([0]), "en": np.array([1])},
                (1, 4, 4, 4))
    # opset 1: attributes
    node = o._node("Slice", ["a"], ["y"], "sl1", o._attr_ints("starts", [1]) + o._attr_ints("ends", [3])
                   + o._attr_ints("axes", [2]))
    c, a, y = _single(tmp_path, node, {}, (1, 4, 2, 4), opset=9)
    np.testing.assert_allclose(y, a[:, 1:3].reshape(-1), rtol=1e-5, atol=1e-6)
    # a full slice is an alias, not a layer
    node = o._node("Slice", ["a", "st", "en", "ax"], ["y"], "sl2")
    c, a, y = _single(tmp_path, node, {"st": np.array([0]), "en": np.array([4]), "ax": np.array([1])}, (1, 4, 4, 4))
    assert [l.name for l in c.layers] == ["conv2d", "rescale"]
    # refusals, by node name
    with pytest.raises(NotImplementedError, match="neg.*positive steps"):
        _single(tmp_path, o._node("Slice", ["a", "st", "en", "ax", "sp"], ["y"], "neg"),
                {"st": np.array([3]), "en": np.array([0]), "ax": np.array([1]), "sp": np.array([-1])}, (1, 3, 4, 4))
    with pytest.raises(NotImplementedError, match="dyn.*initializer"):
        _single(tmp_path, o._node("Slice", ["a", "input", "en"], ["y"], "dyn"), {"en": np.array([1])}, (1, 4, 4, 4))
    with pytest.raises(ValueError, match="emp.*empty"):
        _single(tmp_path, o._node("Slice", ["a", "st", "en", "ax"], ["y"], "emp"),
                {"st": np.array([2]), "en": np.array([2]), "ax": np.array([1])}, (1, 0, 4, 4))


def test_onnx_split_branches_concat(tmp_path):
    """Split -> (left: identity, right: Relu) -> Concat, the skeleton of a ShuffleNet unit: each part is its own
    Gather reading the Split's input."""
    from dash_amd.ir import onnx as o

    rng = np.random.default_rng(9)
    for form in ("equal", "attr", "input"):
        nodes, inits = _conv_front(rng)
        attrs = o._attr_int("axis", 1)
        ins = ["a"]
        parts = [2, 2]
        if form == "attr":
            parts = [1, 3]
            attrs += o._attr_ints("split", parts)
        elif form == "input":
            parts = [3, 1]
            inits["sp"] = np.array(parts)
            ins.append("sp")
        nodes += [o._node("Split", ins, ["l", "r"], "split", attrs), o._node("Relu", ["r"], ["rr"], "relu"),
                  o._node("Concat", ["l", "rr"], ["y"], "cat", o._attr_int("axis", 1))]
        c = _load(_model(tmp_path / f"s_{form}.onnx", nodes, inits, (1, 2, 4, 4), "y", (1, 4, 4, 4)))
        assert [l.name for l in c.layers] == ["conv2d", "rescale", "gather", "gather", "approx_relu", "concat"]
        left, right, cat = c.layers[2], c.layers[3], c.layers[5]
        assert (left.in_src, right.in_src) == (None, 1) and list(cat.srcs) == [2, 4]
        assert left.out_dims == (parts[0], 4, 4) and right.out_dims == (parts[1], 4, 4)
        x = rng.uniform(-1, 1, 32).astype(np.float32)
        a = _conv_ref(inits, x, 2, 16).reshape(4, 4, 4)
        want = np.concatenate([a[:parts[0]], np.maximum(a[parts[0]:], 0)])
        np.testing.assert_allclose(c.plain_eval(x, False), want.reshape(-1), rtol=1e-5, atol=1e-6)
    nodes, inits = _conv_front(rng)
    with pytest.raises(NotImplementedError, match="uneven.*equal parts"):
        _load(_model(tmp_path / "u.onnx", nodes + [o._node("Split", ["a"], ["p", "q", "y"], "uneven", o._attr_int("axis", 1))],
                     inits, (1, 2, 4, 4), "y", (1, 1, 4, 4)))
    with pytest.raises(NotImplementedError, match="batch0.*batch axis"):
        _load(_model(tmp_path / "b.onnx", nodes + [o._node("Split", ["a"], ["p", "y"], "batch0")], inits, (1, 2, 4, 4), "y",
                     (1, 4, 4, 4)))
    with pytest.raises(ValueError, match="bad0.*split"):
        _load(_model(tmp_path / "c.onnx", nodes + [o._node("Split", ["a"], ["p", "y"], "bad0", o._attr_int("axis", 1)
                                                           + o._attr_ints("split", [1, 2]))], inits, (1, 2, 4, 4), "y",
                     (1, 2, 4, 4)))


@pytest.mark.parametrize("mode", [None, "DCR", "CRD"])
def test_onnx_depth_to_space(tmp_path, mode):
    from dash_amd.ir import onnx as o

    attrs = o._attr_int("blocksize", 2) + (o._attr_str("mode", mode) if mode else b"")
    c, a, y = _single(tmp_path, o._node("DepthToSpace", ["a"], ["y"], "d2s", attrs), {}, (1, 1, 8, 8))
    assert c.layers[-1].name == "gather" and c.output_dims == (1, 8, 8)
    if mode == "CRD":
        want = numpy_pixel_shuffle(a, 2)
    else:  # DCR, the operator's default
        want = a.reshape(2, 2, 1, 4, 4).transpose(2, 3, 0, 4, 1).reshape(1, 8, 8)
    np.testing.assert_allclose(y, want.reshape(-1), rtol=1e-5, atol=1e-6)


def test_onnx_space_to_depth_and_refusals(tmp_path):
    from dash_amd.ir import onnx as o

    c, a, y = _single(tmp_path, o._node("SpaceToDepth", ["a"], ["y"], "s2d", o._attr_int("blocksize", 2)), {},
                      (1, 16, 2, 2))
    want = a.reshape(4, 2, 2, 2, 2).transpose(2, 4, 0, 1, 3).reshape(16, 2, 2)
    np.testing.assert_allclose(y, want.reshape(-1), rtol=1e-5, atol=1e-6)
    with pytest.raises(NotImplementedError, match="s2d3"):
        _single(tmp_path, o._node("SpaceToDepth", ["a"], ["y"], "s2d3", o._attr_int("blocksize", 3)), {}, (1, 36, 1, 1))
    with pytest.raises(NotImplementedError, match="d2s3"):
        _single(tmp_path, o._node("DepthToSpace", ["a"], ["y"], "d2s3", o._attr_int("blocksize", 3)), {}, (1, 1, 12, 12))


def test_onnx_gather(tmp_path):
    from dash_amd.ir import onnx as o

    # a 1-D index list along the channel axis, with a negative entry
    c, a, y = _single(tmp_path, o._node("Gather", ["a", "ix"], ["y"], "g", o._attr_int("axis", 1)),
                      {"ix": np.array([3, 0, -1, 0])}, (1, 4, 4, 4))
    assert c.layers[-1].name == "gather" and c.output_dims == (4, 4, 4)
    np.testing.assert_allclose(y, a[[3, 0, 3, 0]].reshape(-1), rtol=1e-5, atol=1e-6)
    # a scalar index drops the axis
    c, a, y = _single(tmp_path, o._node("Gather", ["a", "ix"], ["y"], "g", o._attr_int("axis", -1)),
                      {"ix": np.array(2)}, (1, 4, 4))
    assert c.output_dims == (4, 4)
    np.testing.assert_allclose(y, a[:, :, 2].reshape(-1), rtol=1e-5, atol=1e-6)
    with pytest.raises(NotImplementedError, match="g2.*scalar"):
        _single(tmp_path, o._node("Gather", ["a", "ix"], ["y"], "g2", o._attr_int("axis", 1)),
                {"ix": np.array([[0, 1], [2, 3]])}, (1, 2, 2, 4, 4))
    with pytest.raises(NotImplementedError, match="g0.*batch axis"):
        _single(tmp_path, o._node("Gather", ["a", "ix"], ["y"], "g0"), {"ix": np.array([0])}, (1, 4, 4, 4))
    with pytest.raises(NotImplementedError, match="gd.*initializer"):
        _single(tmp_path, o._node("Gather", ["a", "input"], ["y"], "gd", o._attr_int("axis", 1)), {}, (1, 4, 4, 4))
    with pytest.raises(ValueError, match="gr.*outside"):
        _single(tmp_path, o._node("Gather", ["a", "ix"], ["y"], "gr", o._attr_int("axis", 1)), {"ix": np.array([4])},
                (1, 1, 4, 4))


def _shuffle_chain(tmp_path, s5=(1, 2, 2, 4, 4), out=("y", (1, 4, 4, 4)), **kw):
    """What PyTorch exports for a channel shuffle with 2 groups: view (1, 2, 2, 4, 4), transpose(1, 2), view back."""
    from dash_amd.ir import onnx as o

    node = [o._node("Reshape", ["a", "s5"], ["v"], "view5"),
            o._node("Transpose", ["v"], ["t"], "swap", o._attr_ints("perm", [0, 2, 1, 3, 4])),
            o._node("Reshape", ["t", "s4"], ["y"], "view4")]
    rng = np.random.default_rng(10)
    nodes, inits = _conv_front(rng)
    inits.update(s5=np.array(s5), s4=np.array([1, -1, 4, 4]))
    c = _load(_model(tmp_path / "sh.onnx", nodes + node, inits, (1, 2, 4, 4), *out), **kw)
    x = rng.uniform(-1, 1, 32).astype(np.float32)
    return c, _conv_ref(inits, x, 2, 16).reshape(4, 4, 4), c.plain_eval(x, False)


def test_onnx_shuffle_chain_is_opt_in(tmp_path):
    with pytest.raises(NotImplementedError, match="swap.*Transpose is supported only"):
        _shuffle_chain(tmp_path)  # today's refusal
    c, a, y = _shuffle_chain(tmp_path, transpose="gather")
    assert [l.name for l in c.layers] == ["conv2d", "rescale", "gather"]  # one layer with the composed map
    g = c.layers[-1]
    assert g.in_dims == (4, 4, 4) and g.out_dims == (4, 4, 4)
    np.testing.assert_array_equal(g.idx, d.Gather.channel_shuffle((4, 4, 4), 2).idx)
    np.testing.assert_allclose(y, a[[0, 2, 1, 3]].reshape(-1), rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError, match="transpose"):
        _shuffle_chain(tmp_path, transpose="always")
    # the batch axis written as the shape's only -1 is one sample too
    c2, _, y2 = _shuffle_chain(tmp_path, s5=(-1, 2, 2, 4, 4), transpose="gather")
    np.testing.assert_array_equal(c2.layers[-1].idx, g.idx)
    # a shape whose first entry is no batch axis of one sample: refused by the Reshape's name, no numpy error
    with pytest.raises(NotImplementedError, match="view5.*batch axis"):
        _shuffle_chain(tmp_path, s5=(2, 2, 2, 4, 4), transpose="gather")
    # an intermediate that is a graph output is a tensor of its own: no chain, the Transpose is refused by name
    with pytest.raises(NotImplementedError, match="swap"):
        _shuffle_chain(tmp_path, out=("t", (1, 2, 2, 4, 4)), transpose="gather")


def test_onnx_axes_of_a_flat_imported_reshape_are_refused(tmp_path):
    """A Reshape outside the recognised patterns is imported as a Flatten. A Slice, Split or Gather behind it, also
    through an elementwise node, would name an axis of a view that the importer does not track: refused by name.
    Behind a Reshape to [N, K] the axes are the tracked ones."""
    from dash_amd.ir import onnx as o

    def load(nodes, inits_, out_dims):
        rng = np.random.default_rng(13)
        front, inits = _conv_front(rng)
        inits.update(inits_)
        c = _load(_model(tmp_path / "v.onnx", front + nodes, inits, (1, 2, 4, 4), "y", out_dims))
        x = rng.uniform(-1, 1, 32).astype(np.float32)
        return c, _conv_ref(inits, x, 2, 16).reshape(-1), c.plain_eval(x, False)

    view = o._node("Reshape", ["a", "s"], ["v"], "glu_view")
    s3 = {"s": np.array([1, 2, 2, 16])}
    with pytest.raises(NotImplementedError, match="sp.*glu_view"):
        load([view, o._node("Split", ["v"], ["p", "y"], "sp", o._attr_int("axis", 1))], s3, (1, 1, 2, 16))
    with pytest.raises(NotImplementedError, match="sl.*glu_view"):
        load([view, o._node("Relu", ["v"], ["r"], "relu"), o._node("Slice", ["r", "st", "en", "ax"], ["y"], "sl")],
             dict(s3, st=np.array([0]), en=np.array([1]), ax=np.array([1])), (1, 1, 2, 16))
    with pytest.raises(NotImplementedError, match="ga.*glu_view"):
        load([view, o._node("Gather", ["v", "ix"], ["y"], "ga", o._attr_int("axis", 1))], dict(s3, ix=np.array([1])),
             (1, 1, 2, 16))
    c, a, y = load([view, o._node("Slice", ["v", "st", "en", "ax"], ["y"], "sl")],
                   {"s": np.array([1, 64]), "st": np.array([5]), "en": np.array([9]), "ax": np.array([1])}, (1, 4))
    assert [l.name for l in c.layers] == ["conv2d", "rescale", "flatten", "gather"]
    np.testing.assert_allclose(y, a[5:9], rtol=1e-5, atol=1e-6)


def test_onnx_transpose_opt_in(tmp_path):
    from dash_amd.ir import onnx as o

    node = o._node("Transpose", ["a"], ["y"], "perm0", o._attr_ints("perm", [0, 2, 1, 3]))
    with pytest.raises(NotImplementedError, match="perm0"):
        _single(tmp_path, node, {}, (1, 4, 4, 4))
    c, a, y = _single(tmp_path, node, {}, (1, 4, 4, 4), transpose="gather")
    assert c.layers[-1].name == "gather"
    np.testing.assert_allclose(y, a.transpose(1, 0, 2).reshape(-1), rtol=1e-5, atol=1e-6)
    # a perm that moves the batch axis, and a Transpose of a Reshape (whose tracked dims are flat): refused by name
    with pytest.raises(NotImplementedError, match="perm1"):
        _single(tmp_path, o._node("Transpose", ["a"], ["y"], "perm1", o._attr_ints("perm", [1, 0, 2, 3])), {},
                (4, 1, 4, 4), transpose="gather")
    rng = np.random.default_rng(11)
    nodes, inits = _conv_front(rng)
    inits["s316"] = np.array([1, 4, 16])
    nodes += [o._node("Reshape", ["a", "s316"], ["am"], "ra"),
              o._node("Transpose", ["am"], ["y"], "lone1", o._attr_ints("perm", [0, 2, 1]))]
    with pytest.raises(NotImplementedError, match="lone1.*tracked under dims"):
        _load(_model(tmp_path / "l.onnx", nodes, inits, (1, 2, 4, 4), "y", (1, 16, 4)), transpose="gather")
    from tests.test_matmul import _nonlocal_onnx
    from dash_amd.ir.onnx import load_onnx_model

    # a Transpose that folds into a MatMul still folds under the keyword
    path, _ = _nonlocal_onnx(tmp_path)
    assert [l.name for l in load_onnx_model(path, Q.ScaleQuant, 5, transpose="gather").layers] == \
        [l.name for l in load_onnx_model(path, Q.ScaleQuant, 5).layers]


def test_onnx_token_major_view_is_still_refused(tmp_path):
    """tests/test_matmul_heads.py's t_q case under the keyword: a Transpose that moves the head axis of a Reshape
    view next to a MatMul is no Transpose of a produced tensor under its tracked dims."""
    from dash_amd.ir import onnx as o
    from dash_amd.ir.onnx import load_onnx_model
    from tests.test_matmul_heads import _attention_onnx

    swap = {"t_q": o._node("Transpose", ["qh"], ["qt"], "t_q", o._attr_ints("perm", [0, 2, 1, 3]))}
    for kw in ({}, {"transpose": "gather"}):
        with pytest.raises(NotImplementedError, match="t_q"):
            load_onnx_model(_attention_onnx(tmp_path, swap=swap)[0], Q.ScaleQuant, 5, **kw)


def test_onnx_export_import_is_the_identity(tmp_path):
    from dash_amd.ir.onnx import load_onnx_model, parse_onnx, save_onnx_model

    c, xs = shuffle_unit_case()
    extra = d.Gather.depth_to_space((4, 4, 4), 2, "CRD")
    c = d.Circuit(list(c.layers) + [extra, d.Gather((1, 8, 8), np.arange(64)[::-1].copy())])  # a flat out_dims too
    path = tmp_path / "rt.onnx"
    save_onnx_model(path, c)
    ops = [n["op_type"] for n in parse_onnx(path)["nodes"]]
    assert ops.count("Gather") == 5 and ops.count("Flatten") == 5 and ops.count("Reshape") == 4
    back = load_onnx_model(path, Q.ScaleQuant, 5)
    assert [l.name for l in back.layers] == [l.name for l in c.layers]
    assert [l.in_src for l in back.layers] == [l.in_src for l in c.layers]
    for a, b in zip(back.layers, c.layers):
        assert (a.in_dims, a.out_dims) == (b.in_dims, b.out_dims)
        if isinstance(b, d.Gather):
            np.testing.assert_array_equal(a.idx, b.idx)
    for x in xs[:3]:
        np.testing.assert_array_equal(back.plain_q_eval(x, False, M7), c.plain_q_eval(x, False, M7))


def test_onnx_pending_factor_passes_through(tmp_path):
    """Value-preserving: an average's 1/K passes through a Slice to the next Gemm's weights, as through an Upsample."""
    from dash_amd.ir import onnx as o

    rng = np.random.default_rng(12)
    nodes, inits = _conv_front(rng)
    inits.update(st=np.array([1]), en=np.array([3]), ax=np.array([1]), wf=_f32(rng, 3, 2), bf=_f32(rng, 3))
    nodes += [o._node("GlobalAveragePool", ["a"], ["p"], "gap"), o._node("Slice", ["p", "st", "en", "ax"], ["s"], "sl"),
              o._node("Flatten", ["s"], ["f"], "fl", o._attr_int("axis", 1)),
              o._node("Gemm", ["f", "wf", "bf"], ["y"], "fc", o._attr_int("transB", 1))]
    c = _load(_model(tmp_path / "p.onnx", nodes, inits, (1, 2, 4, 4), "y", (1, 3)))
    assert [l.name for l in c.layers] == ["conv2d", "rescale", "sum_pool", "gather", "flatten", "dense", "rescale"]
    x = rng.uniform(-1, 1, 32).astype(np.float32)
    a = _conv_ref(inits, x, 2, 16)
    np.testing.assert_allclose(c.plain_eval(x, False), inits["wf"] @ a.mean(axis=1)[1:3] + inits["bf"], rtol=1e-4,
                               atol=1e-5)


# ---------------------------------------------------------------- 5. zoo, trainer, CLI
def _zoo(name):
    from dash_amd.models import zoo

    c = zoo.build_circuit(name, Q.ScaleQuant, 5, seed=0)
    xs = zoo.quantized_inputs(name, 2, Q.ScaleQuant, 5, seed=7)
    c.calibrate(xs, M7)
    assert c.required_crt_modulus() <= M7
    return c, xs


def test_shufflenet_float_forward_and_host_garbling():
    c, xs = _zoo("SHUFFLENET_V2_CIFAR")
    convs = [l for l in c.layers if isinstance(l, d.Conv2d)]
    gathers = [l for l in c.layers if isinstance(l, d.Gather)]
    assert len(convs) == 2 + 2 * 3 and len(gathers) == 2 * 3
    assert [g.in_src is not None for g in gathers] == [False, True, False] * 2
    x = np.random.default_rng(1).uniform(-1, 1, 3 * 32 * 32).astype(np.float32)
    t = x
    for l in convs[:2]:  # the stem: two strided 3x3 convs + ReLU, to (16, 8, 8)
        t = np.maximum(l.plain_eval(t, False), 0)
    t = t.reshape(16, 8, 8)
    for u in range(2):
        t = numpy_shuffle_unit(t, convs[2 + 3 * u:5 + 3 * u])
    head = c.layers[-2]
    ref = head.weights @ t.sum(axis=(1, 2)) + head.biases
    np.testing.assert_allclose(c.plain_eval(x, False), ref, rtol=1e-4, atol=1e-4)
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED)
    np.testing.assert_array_equal(_host_eval(gc, xs[0]), c.plain_q_eval(xs[0], False, M7))


def test_subpixel_float_forward_and_host_garbling():
    c, xs = _zoo("SUBPIXEL_SEG_CIFAR")
    assert c.output_dims == (1, 32, 32)
    convs = [l for l in c.layers if isinstance(l, d.Conv2d)]
    x = np.random.default_rng(2).uniform(-1, 1, 3 * 32 * 32).astype(np.float32)
    t = np.maximum(convs[0].plain_eval(x, False), 0)
    t = np.maximum(convs[1].plain_eval(t, False), 0)
    scores = numpy_pixel_shuffle(convs[2].plain_eval(t, False).reshape(16, 16, 16), 2)
    assert scores.shape == (4, 32, 32)
    np.testing.assert_array_equal(c.plain_eval(x, False), np.argmax(scores, axis=0).reshape(-1))
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED)
    np.testing.assert_array_equal(_host_eval(gc, xs[0]), c.plain_q_eval(xs[0], False, M7))


def test_trainer_refuses_the_new_ops():
    from dash_amd.models import train, zoo

    with pytest.raises(NotImplementedError, match="shuffle_unit"):
        train.build_torch_model("SHUFFLENET_V2_CIFAR")
    with pytest.raises(NotImplementedError, match="d2s"):
        train.build_torch_model("SUBPIXEL_SEG_CIFAR")
    zoo.ARCHS["_SHUFFLE_ONLY"] = {"input": (4, 2, 2), "ops": [("shuffle", 2)]}
    try:
        with pytest.raises(NotImplementedError, match="shuffle"):
            train.build_torch_model("_SHUFFLE_ONLY")
        c = zoo.build_circuit("_SHUFFLE_ONLY", Q.ScaleQuant, 5)
        np.testing.assert_array_equal(c.layers[0].idx, d.Gather.channel_shuffle((4, 2, 2), 2).idx)
    finally:
        del zoo.ARCHS["_SHUFFLE_ONLY"]
    zoo.ARCHS["_ODD_UNIT"] = {"input": (3, 2, 2), "ops": [("shuffle_unit",)]}
    try:
        with pytest.raises(ValueError, match="even channel"):
            zoo.build_circuit("_ODD_UNIT", Q.ScaleQuant, 5)
    finally:
        del zoo.ARCHS["_ODD_UNIT"]


# ---------------------------------------------------------------- 6. range guard
def test_range_guard_finds_a_violation_behind_a_gather():
    """Gather -> Rescale(1): the Gather sets no limit, the rescale behind it does. An input whose only out-of-range
    value sits on an element the map reads is flagged by the numpy and the torch path alike; the same value on an
    element that no output reads is not."""
    idx = np.array([4, 4, 0, 2])  # elements 1 and 3 go unread
    c = d.Circuit([d.Gather((5,), idx), d.Rescale(1, (4,))])
    lim = c.layers[1].mrs_limit(M7)
    ok = np.array([lim - 1, 0, -5, 0, 7])
    read = np.array([0, 0, 0, 0, lim])
    unread = np.array([0, lim, 0, M7 // 2 - 1, 0])
    xs, want = [ok, read, unread], [False, True, False]
    g = RangeGuard(c, M7, mrs=True)
    assert g.batched and not g.native_forms
    assert [bool(g.violations_np(x)) for x in xs] == want
    assert g.submit(xs).bad_indices() == [1]
    np.testing.assert_array_equal(g.outputs([ok])[0], c.plain_q_eval(ok, False, M7))
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED, rescale="mrs")
    np.testing.assert_array_equal(_host_eval(gc, ok), c.plain_q_eval(ok, False, M7))
