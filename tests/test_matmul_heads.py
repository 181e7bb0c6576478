"""The multi-head MatMul layer on the host (docs/MATMUL.md, Heads): layer semantics against numpy's einsum, the
refusals, the unchanged G = 1 wire image, the host garbler and evaluator against the plaintext model, head
isolation, ONNX import / export, the zoo's ReLU-attention block and the range guard. Circuits and inputs:
tests/matmul_heads_cases.py. The GPU side is tests/test_gpu_matmul_heads.py."""
from __future__ import annotations

import itertools

import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit, RangeGuard
from dash_amd.ir.quant import QuantizationMethod as Q
from tests.matmul_cases import matmul_circuit, tiny_arch
from tests.matmul_heads_cases import (M7, TINY_ATTENTION, expected, gram_heads_circuit, gram_heads_expected,
                                      gram_heads_inputs, guard_heads_case, heads_circuit, heads_inputs, lim_of, operands,
                                      split_circuit)
from tests.test_clip import _conv_attrs, _f32, _onnx_model

SEED = bytes(range(16))
FLAGS = list(itertools.product([False, True], [False, True]))


def _host_eval(gc, x):
    return gc.decode_outputs(gc.cpu_evaluate(gc.garble_inputs(x)))


# ---------------------------------------------------------------- 1. the layer
@pytest.mark.parametrize("ta,tb", FLAGS, ids=["nn", "nt", "tn", "tt"])
def test_plain_q_eval_is_the_einsum(ta, tb):
    G, M, T, N = 3, 5, 3, 7
    c = heads_circuit(G, M, T, N, ta, tb)
    mm = c.layers[1]
    assert (mm.heads, mm.M, mm.T, mm.N) == (G, M, T, N) and mm.out_dims == (G * M, N)
    for x in heads_inputs(G, M, T, N, ta, tb, rounds=3):
        out = c.plain_q_eval(x, False)
        assert out.dtype == np.int64
        a, b = operands(G, M, T, N, x, ta, tb)
        np.testing.assert_array_equal(out, np.einsum("git,gtl->gil", a, b).reshape(-1))
        f = mm.plain_eval(x.astype(np.float32), False, [None, c.layers[0].plain_q_eval(x, False).astype(np.float32)])
        assert f.dtype == np.float32
        np.testing.assert_allclose(f, out)


def test_extremes_sit_on_every_head():
    G, M, T, N = 3, 5, 3, 7
    lim = lim_of(T)
    outs = np.stack([expected(G, M, T, N, x).reshape(G, M * N) for x in heads_inputs(G, M, T, N, rounds=7)])
    assert np.abs(outs).max() == T * lim * lim < M7 // 2
    for g in range(G):  # the first and last output of every head see an extreme in some round
        for e in (0, M * N - 1):
            assert np.abs(outs[:, g, e]).max() == T * lim * lim


def test_spec_repr_and_out_dims():
    l = d.MatMul((6, 4), 0, (12, 5), heads=3)  # 3 slabs (2, 4) and (4, 5)
    assert (l.M, l.T, l.N, l.heads) == (2, 4, 5, 3) and l.out_dims == (6, 5)
    assert l.garble_spec() == (22, {"src": 0, "M": 2, "T": 4, "N": 5, "G": 3})
    assert repr(l).endswith("out_dims=(6, 5), heads=3)")
    # a (C, H, W) operand: the leading axis splits, the slab (C / G, H, W) reads as C / G x H W
    t = d.MatMul((4, 2, 3), 0, (4, 2, 3), trans_a=True, heads=2, out_dims=(2, 6, 6))
    assert (t.M, t.T, t.N) == (6, 2, 6) and t.out_dims == (2, 6, 6)
    assert t.garble_spec() == (22, {"src": 0, "M": 6, "T": 2, "N": 6, "ta": 1, "G": 2})
    one = d.MatMul((2, 3), 0, (3, 5), heads=1)
    assert one.heads == 1 and "G" not in one.garble_spec()[1] and "heads" not in repr(one)


def test_refusals():
    with pytest.raises(ValueError, match=r"\(5, 3\).*3 heads|3 heads.*\(5, 3\)") as ex:
        d.MatMul((5, 3), 0, (9, 4), heads=3)  # 5 % 3 != 0
    assert "(5, 3)" in str(ex.value) and "3" in str(ex.value)
    with pytest.raises(ValueError, match=r"\(7, 4\)"):
        d.MatMul((6, 3), 0, (7, 4), heads=3)  # the operand's leading axis
    with pytest.raises(ValueError, match=r"matmul: x of dims .* and y of dims .*inner sizes"):
        d.MatMul((6, 4), 0, (9, 5), heads=3)  # 2 x 4 against 3 x 5 per head
    with pytest.raises(ValueError, match="out_dims"):
        d.MatMul((6, 4), 0, (12, 5), heads=3, out_dims=(2, 5))  # one head's size, not three
    with pytest.raises(ValueError, match="1-D"):
        d.MatMul((6,), 0, (6,), heads=2)
    with pytest.raises(ValueError, match="1-D"):
        d.MatMul((6, 1), 0, (6,), trans_a=True, heads=2)
    with pytest.raises(ValueError, match="heads"):
        d.MatMul((6, 4), 0, (12, 5), heads=0)


def test_single_head_wire_image_is_unchanged():
    """G = 1 is today's layer: no "G" in the spec, and the serialized garbled model is byte-identical to the one of a
    layer built without the keyword."""
    with_kw = heads_circuit(1, 5, 3, 7, True, False)
    without = heads_circuit(1, 5, 3, 7, True, False, heads=None)
    legacy = matmul_circuit(5, 3, 7, True, False)  # the single-head cases' own builder: the same circuit
    assert "G" not in with_kw.layers[1].garble_spec()[1]
    blobs = [bytes(GarbledCircuit(c, 7, 100.0, seed=SEED).model.serialize()) for c in (with_kw, without, legacy)]
    assert blobs[0] == blobs[1] == blobs[2]
    assert "G" not in GarbledCircuit(with_kw, 7, 100.0, seed=SEED).model.layer_params(1)
    p = GarbledCircuit(heads_circuit(2, 5, 3, 7), 7, 100.0, seed=SEED).model.layer_params(1)
    assert list(p["G"]) == [2] and [list(p[k]) for k in ("M", "T", "N")] == [[5], [3], [7]]


# ---------------------------------------------------------------- 2. host garbler and evaluator
# every shape of the GPU tests, so the host evaluator that is their oracle is itself checked against the plain model
HOST_CASES = [((3, 5, 3, 7), False, False), ((3, 5, 3, 7), True, True), ((2, 13, 4, 20), False, True),
              ((4, 8, 16, 16), False, True), ((2, 16, 16, 16), False, False), ((3, 17, 5, 18), True, False),
              ((2, 16, 17, 15), False, False), ((4, 16, 8, 16), True, False), ((2, 1, 1, 1), False, False)]


@pytest.mark.parametrize("shape,ta,tb", HOST_CASES, ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)[0])
def test_host_garble_and_evaluate(shape, ta, tb):
    G, M, T, N = shape
    c = heads_circuit(*shape, ta, tb)
    gcs = [GarbledCircuit(c, 7, 100.0, seed=bytes([s]) * 16) for s in (1, 2)]
    for gc, x in zip(gcs, heads_inputs(*shape, ta, tb)):
        y = _host_eval(gc, x)
        np.testing.assert_array_equal(y, c.plain_q_eval(x, False, M7))
        np.testing.assert_array_equal(y, expected(*shape, x, ta, tb))
    arrs = gcs[0].model.layer_arrays(1)
    assert set(arrs) == {"g", "e"} and all(np.asarray(a).shape[0] == G * M * N * T for a in arrs.values())


def test_host_gram_with_heads():
    G, M, T = 3, 4, 5
    c = gram_heads_circuit(G, M, T)
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED)
    for x in gram_heads_inputs(G, M, T):
        np.testing.assert_array_equal(_host_eval(gc, x), gram_heads_expected(G, M, T, x))


def test_serialize_roundtrip_with_heads():
    from dash_amd.native import native

    shape = (3, 5, 3, 7)
    gc = GarbledCircuit(heads_circuit(*shape, True, True), 7, 100.0, seed=SEED)
    blob = gc.model.serialize()
    back = native().GarbledModel.deserialize(blob)
    assert bytes(back.serialize()) == bytes(blob)
    x = heads_inputs(*shape, True, True)[0]
    np.testing.assert_array_equal(gc.decode_outputs(native().cpu_evaluate(back, gc.garble_inputs(x), 0)),
                                  expected(*shape, x, True, True))


def test_head_isolation():
    """G = 3: changing only head 1's operand values changes only head 1's decoded outputs, and the garbled output
    equals that of three single-head MatMul circuits on the slabs, value for value."""
    G, M, T, N = 3, 4, 3, 5
    nx, ny = M * T, T * N
    lim = lim_of(T)
    rng = np.random.default_rng(11)
    x, y = rng.integers(-lim, lim + 1, (G, nx)), rng.integers(-lim, lim + 1, (G, ny))
    x2, y2 = x.copy(), y.copy()
    x2[1], y2[1] = rng.integers(1, lim + 1, nx), rng.integers(1, lim + 1, ny)  # all positive: every output moves
    x[1, 0] = -x2[1, 0]
    gc = GarbledCircuit(split_circuit(G, M, T, N), 7, 100.0, seed=SEED)
    one = GarbledCircuit(split_circuit(1, M, T, N), 7, 100.0, seed=bytes([9]) * 16)
    outs = []
    for xv, yv in ((x, y), (x2, y2)):
        out = _host_eval(gc, np.concatenate([xv.reshape(-1), yv.reshape(-1)])).reshape(G, M * N)
        for g in range(G):
            np.testing.assert_array_equal(out[g], _host_eval(one, np.concatenate([xv[g], yv[g]])))
            np.testing.assert_array_equal(out[g], (xv[g].reshape(M, T) @ yv[g].reshape(T, N)).reshape(-1))
        outs.append(out)
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_array_equal(outs[0][2], outs[1][2])
    assert not np.array_equal(outs[0][1], outs[1][1])


# ---------------------------------------------------------------- 3. ONNX
def _attention_onnx(tmp_path, h=2, extra=None, swap=None):
    """The channel-major form: q, k, v 1x1 convs 2 -> 4 on [1, 2, 2, 2]; views (1, h, 4 / h, 4); the scores
    Transpose(q) k of (1, h, 4, 4), a Relu, the mix v Transpose(relu) and a Reshape back to [1, 4, 2, 2]. `swap`
    replaces named nodes."""
    from dash_amd.ir import onnx as o

    rng = np.random.default_rng(3)
    inits = {"wq": _f32(rng, 4, 2, 1, 1), "bq": _f32(rng, 4), "wk": _f32(rng, 4, 2, 1, 1), "bk": _f32(rng, 4),
             "wv": _f32(rng, 4, 2, 1, 1), "bv": _f32(rng, 4), "sh": np.asarray([1, h, 4 // h, 4], np.float32),
             "s422": np.asarray([1, 4, 2, 2], np.float32), "sh1": np.asarray([1, 1, 4, 4], np.float32),
             "s5": np.asarray([1, 1, h, 4 // h, 4], np.float32)}
    nodes = {"q": o._node("Conv", ["input", "wq", "bq"], ["q"], "q", _conv_attrs(1)),
             "k": o._node("Conv", ["input", "wk", "bk"], ["k"], "k", _conv_attrs(1)),
             "v": o._node("Conv", ["input", "wv", "bv"], ["v"], "v", _conv_attrs(1)),
             "r_q": o._node("Reshape", ["q", "sh"], ["qh"], "r_q"),
             "t_q": o._node("Transpose", ["qh"], ["qt"], "t_q", o._attr_ints("perm", [0, 1, 3, 2])),
             "r_k": o._node("Reshape", ["k", "sh"], ["kh"], "r_k"),
             "mm_s": o._node("MatMul", ["qt", "kh"], ["s"], "mm_s"),
             "relu": o._node("Relu", ["s"], ["a"], "relu"),
             "r_v": o._node("Reshape", ["v", "sh"], ["vh"], "r_v"),
             "t_a": o._node("Transpose", ["a"], ["at"], "t_a", o._attr_ints("perm", [0, 1, 3, 2])),
             "mm_o": o._node("MatMul", ["vh", "at"], ["oh"], "mm_o"),
             "r_o": o._node("Reshape", ["oh", "s422"], ["y"], "r_o")}
    nodes.update(swap or {})
    return _onnx_model(tmp_path / "attn.onnx", list(nodes.values()) + (extra or []), inits, (1, 2, 2, 2), "y",
                       (1, 4, 2, 2)), inits


def test_onnx_import_of_the_channel_major_form(tmp_path):
    from dash_amd.ir.onnx import load_onnx_model

    path, inits = _attention_onnx(tmp_path)
    c = load_onnx_model(path, Q.ScaleQuant, 5)
    assert [l.name for l in c.layers] == ["conv2d", "rescale"] * 3 + ["matmul", "rescale", "approx_relu", "matmul",
                                                                     "rescale"]
    s, o = c.layers[6], c.layers[9]
    assert (s.in_dims, s.src_dims, s.trans_a, s.trans_b, s.heads, s.out_dims) == ((4, 4), (4, 4), True, False, 2, (8, 4))
    assert (s.M, s.T, s.N) == (4, 2, 4) and (s.in_src, s.src) == (1, 3)  # q's and k's rescales
    assert (o.in_dims, o.src_dims, o.trans_a, o.trans_b, o.heads, o.out_dims) == ((4, 4), (8, 4), False, True, 2, (4, 2, 2))
    assert (o.M, o.T, o.N) == (2, 4, 4) and (o.in_src, o.src) == (5, 8)  # v's rescale, the Relu of the scores
    assert c.output_dims == (4, 2, 2)
    x = np.random.default_rng(1).uniform(-1, 1, 8).astype(np.float32)

    def conv(w, b):
        return (inits[w].reshape(4, 2) @ x.reshape(2, 4) + inits[b][:, None]).reshape(2, 2, 4)  # [head][dh][token]

    q, k, v = conv("wq", "bq"), conv("wk", "bk"), conv("wv", "bv")
    a = np.maximum(np.einsum("gdi,gdl->gil", q, k), 0)
    ref = np.einsum("gdt,glt->gdl", v, a).reshape(-1)
    np.testing.assert_allclose(c.plain_eval(x, False), ref, rtol=1e-4, atol=1e-5)
    # one head written with a head axis is the single-head layer
    one = load_onnx_model(_attention_onnx(tmp_path, h=1)[0], Q.ScaleQuant, 5)
    assert [l.heads for l in one.layers if isinstance(l, d.MatMul)] == [1, 1]


def test_onnx_refusals_name_their_node(tmp_path):
    from dash_amd.ir import onnx as o
    from dash_amd.ir.onnx import load_onnx_model

    def load(**swap):
        return load_onnx_model(_attention_onnx(tmp_path, swap=swap)[0], Q.ScaleQuant, 5)

    # different head counts: k viewed as one head of (4, 4) against q's two of (2, 4)
    with pytest.raises(NotImplementedError, match="mm_s.*head counts"):
        load(r_k=o._node("Reshape", ["k", "sh1"], ["kh"], "r_k"))
    # a perm that moves the head axis (token-major)
    with pytest.raises(NotImplementedError, match="t_q"):
        load(t_q=o._node("Transpose", ["qh"], ["qt"], "t_q", o._attr_ints("perm", [0, 2, 1, 3])))
    # rank above 3 behind the batch axis
    with pytest.raises(NotImplementedError, match="mm_s.*rank above 3"):
        load(r_q=o._node("Reshape", ["q", "s5"], ["qh"], "r_q"), r_k=o._node("Reshape", ["k", "s5"], ["kh"], "r_k"))
    # a rank-3 operand that is no Reshape alias: the conv's own (C, H, W) output, as before
    with pytest.raises(NotImplementedError, match="mm_s.*batch of more than one matrix"):
        load(mm_s=o._node("MatMul", ["qt", "k"], ["s"], "mm_s"))


def test_onnx_export_import_is_the_identity(tmp_path):
    from dash_amd.ir.onnx import load_onnx_model, parse_onnx, save_onnx_model

    c, xs = tiny_arch("_TINY_ATTENTION_RT", TINY_ATTENTION)
    path = tmp_path / "rt.onnx"
    save_onnx_model(path, c)
    nodes = parse_onnx(path)["nodes"]
    ops = [n["op_type"] for n in nodes]
    # per MatMul: a rank-4 Reshape of each operand and one of the result; one Transpose each
    assert ops.count("MatMul") == 2 and ops.count("Transpose") == 2 and ops.count("Reshape") == 6
    assert all([int(v) for v in n["attrs"]["perm"]] == [0, 1, 3, 2] for n in nodes if n["op_type"] == "Transpose")
    back = load_onnx_model(path, Q.ScaleQuant, 5)
    assert [l.name for l in back.layers] == [l.name for l in c.layers]
    assert [l.in_src for l in back.layers] == [l.in_src for l in c.layers]
    for (ka, pa), (kb, pb) in zip(back.garble_specs(), c.garble_specs()):
        assert ka == kb
        if ka in (d.ir.layers.Kind.MATMUL, d.ir.layers.Kind.RESCALE):
            assert pa == pb
    assert [l.heads for l in back.layers if isinstance(l, d.MatMul)] == [2, 2]
    assert [l.out_dims for l in back.layers] == [l.out_dims for l in c.layers]
    for x in xs:
        np.testing.assert_array_equal(back.plain_q_eval(x, False, M7), c.plain_q_eval(x, False, M7))


# ---------------------------------------------------------------- 4. zoo and trainer
def _relu_attn_cifar():
    from dash_amd.models import zoo

    c = zoo.build_circuit("RELU_ATTN_CIFAR", Q.ScaleQuant, 5, seed=0)
    xs = zoo.quantized_inputs("RELU_ATTN_CIFAR", 2, Q.ScaleQuant, 5, seed=7)
    return c, xs


def test_zoo_model_builds_and_is_refused_where_it_must():
    from dash_amd.models import train, zoo

    c, _ = _relu_attn_cifar()
    sc, mix = [l for l in c.layers if isinstance(l, d.MatMul)]
    assert (sc.heads, sc.M, sc.T, sc.N, sc.trans_a, sc.trans_b, sc.out_dims) == (4, 16, 8, 16, True, False, (64, 16))
    assert (mix.heads, mix.M, mix.T, mix.N, mix.trans_a, mix.trans_b, mix.out_dims) == (4, 8, 16, 16, False, True, (32, 4, 4))
    i = c.layers.index(sc)
    assert isinstance(c.layers[i + 1], d.Rescale) and isinstance(c.layers[i + 2], d.Relu) and mix.src == i + 2
    assert isinstance(c.layers[c.layers.index(mix) + 1], d.Rescale) and mix.in_src is not None
    add = next(l for l in c.layers if isinstance(l, d.Add))
    assert c.layers[add.src].out_dims == (32, 4, 4) and add.src < i  # the block's input
    with pytest.raises(NotImplementedError, match="attention"):
        train.build_torch_model("RELU_ATTN_CIFAR")
    for arch, msg in (({"input": (4, 16, 16), "ops": [("attention", 2)]}, "H W <= 64"),
                      ({"input": (6, 4, 4), "ops": [("attention", 4)]}, "heads divide")):
        zoo.ARCHS["_BAD_ATTENTION"] = arch
        try:
            with pytest.raises(ValueError, match=msg):
                zoo.build_circuit("_BAD_ATTENTION", Q.ScaleQuant, 5)
        finally:
            del zoo.ARCHS["_BAD_ATTENTION"]


def test_zoo_block_is_multi_head_relu_attention():
    """The float model against relu(Q K^T) V per head written out in numpy, with the layers' own weights (q's carry
    the 1 / sqrt(dh), the output conv's the 1 / L)."""
    c, _ = _relu_attn_cifar()
    conv0, conv1, k, v, q, back = [l for l in c.layers if isinstance(l, d.Conv2d)]
    x = np.random.default_rng(1).uniform(-1, 1, 3 * 32 * 32).astype(np.float32)
    a = np.maximum(conv1.plain_eval(np.maximum(conv0.plain_eval(x, False), 0), False), 0)
    a = a.reshape(32, 4, 2, 4, 2).max(axis=(2, 4)).reshape(32, 16).astype(np.float64)  # the 2 x 2 max pool

    def one(l):
        return (l.weights.reshape(32, 32).astype(np.float64) @ a + l.biases[:, None]).reshape(4, 8, 16)

    s = np.maximum(np.einsum("gdi,gdl->gil", one(q), one(k)), 0)  # [head][query][key]
    o = np.einsum("gdt,glt->gdl", one(v), s).reshape(32, 16)
    z = back.weights.reshape(32, 32) @ o + back.biases[:, None] + a
    head = c.layers[-2]
    ref = head.weights @ np.maximum(z, 0).sum(axis=1) + head.biases
    np.testing.assert_allclose(c.plain_eval(x, False), ref, rtol=1e-3, atol=1e-4)


def test_zoo_model_on_the_host():
    c, xs = _relu_attn_cifar()
    c.calibrate(xs, M7)
    assert c.required_crt_modulus() <= M7
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED)
    assert gc.hardened
    for x in xs:
        np.testing.assert_array_equal(_host_eval(gc, x), c.plain_q_eval(x, False, M7))


# ---------------------------------------------------------------- 5. range guard
def test_range_guard_numpy_and_torch_agree_with_the_layer():
    c, xs, want = guard_heads_case()
    mm = c.layers[1]
    for x in xs:  # the layer itself, per head
        np.testing.assert_array_equal(mm.plain_q_eval(x, False, [None, x]), (x.reshape(2, 2) ** 2).sum(axis=1))
    g = RangeGuard(c, M7, mrs=True)
    assert g.batched and not g.native_forms
    assert [bool(g.violations_np(x)) for x in xs] == want
    assert g.submit(xs).bad_indices() == [i for i, w in enumerate(want) if w]
    np.testing.assert_array_equal(g.outputs([xs[0]])[0], c.plain_q_eval(xs[0], False, M7))
    # operands whose T products could reach 2^62: the layer raises, both paths flag the input, nothing wraps
    over = np.array([1 << 31, 1, 1, 1 << 31], dtype=np.int64)  # 2 * 2^31 * 2^31 = 2^63 as a bound; the sums are tiny
    with pytest.raises(OverflowError, match="matmul"):
        mm.plain_q_eval(over, False, [None, over])
    assert bool(g.violations_np(over)) and g.submit([xs[0], over]).bad_indices() == [1]
