"""The MatMul layer on the host (docs/MATMUL.md): layer semantics, the host garbler and evaluator against the
plaintext model, entry counts, the wire round trip, the refusals, the zoo's non-local block, ONNX import / export
and the range guard. Circuits and inputs: tests/matmul_cases.py. The GPU side is tests/test_gpu_matmul.py."""
from __future__ import annotations

import itertools
import math

import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit, RangeGuard
from dash_amd.ir.bases import first_primes
from dash_amd.ir.quant import QuantizationMethod as Q
from dash_amd.native import native
from tests.matmul_cases import (M7, TINY_NONLOCAL, expected, gram_circuit, gram_expected, gram_inputs, guard_case, lim_of,
                                matmul_circuit, matmul_inputs, tiny_arch)
from tests.test_clip import _conv_attrs, _f32, _onnx_model

CRT7 = first_primes(7)
P7 = sum(CRT7)
SEED = bytes(range(16))
FLAGS = list(itertools.product([False, True], [False, True]))


def _host_eval(gc, x):
    return gc.decode_outputs(gc.cpu_evaluate(gc.garble_inputs(x)))


# ---------------------------------------------------------------- 1. the layer
def test_semantics_and_views():
    rng = np.random.default_rng(0)
    x, y = rng.integers(-9, 10, (2, 3, 4)), rng.integers(-9, 10, (12, 5))
    l = d.MatMul((2, 3, 4), 0, (12, 5))  # (2, 3, 4) reads as 2 x 12
    assert (l.M, l.T, l.N) == (2, 12, 5) and l.out_dims == (2, 5) and l.kind == 22 and l.name == "matmul"
    ctx = [None, y.reshape(-1)]
    np.testing.assert_array_equal(l.plain_q_eval(x.reshape(-1), False, ctx), (x.reshape(2, 12) @ y).reshape(-1))
    out = l.plain_eval(x.reshape(-1).astype(np.float32), False, [None, y.reshape(-1).astype(np.float32)])
    assert out.dtype == np.float32
    np.testing.assert_allclose(out, (x.reshape(2, 12) @ y).reshape(-1))
    # a 1-D tensor is 1 x n; its transpose n x 1: an outer product
    o = d.MatMul((4,), 0, (3,), trans_a=True)
    assert (o.M, o.T, o.N) == (4, 1, 3)
    v, w = rng.integers(-9, 10, 4), rng.integers(-9, 10, 3)
    np.testing.assert_array_equal(o.plain_q_eval(v, False, [None, w]), np.outer(v, w).reshape(-1))
    # out_dims of equal size
    assert d.MatMul((2, 16), 0, (16, 16), out_dims=(2, 4, 4)).out_dims == (2, 4, 4)
    assert l.garble_spec() == (22, {"src": 0, "M": 2, "T": 12, "N": 5})
    t = d.MatMul((3, 2), 1, (5, 3), trans_a=True, trans_b=True)
    assert t.garble_spec() == (22, {"src": 1, "M": 2, "T": 3, "N": 5, "ta": 1, "tb": 1})
    assert repr(t) == "MatMul((3, 2), src=1, src_dims=(5, 3), trans_a=True, trans_b=True, out_dims=(2, 5))"


@pytest.mark.parametrize("dims,src_dims,ta,tb", [((2, 3), (4, 5), False, False), ((2, 3), (3, 5), True, False),
                                                 ((2, 3), (3, 5), False, True), ((6,), (6,), False, False)])
def test_refused_shapes(dims, src_dims, ta, tb):
    with pytest.raises(ValueError, match=r"matmul: x of dims .* and y of dims") as ex:
        d.MatMul(dims, 0, src_dims, trans_a=ta, trans_b=tb)
    assert str(dims) in str(ex.value) and str(src_dims) in str(ex.value)


def test_refused_out_dims():
    with pytest.raises(ValueError, match="out_dims"):
        d.MatMul((2, 3), 0, (3, 5), out_dims=(3, 3))


@pytest.mark.parametrize("ta,tb", FLAGS, ids=["nn", "nt", "tn", "tt"])
def test_plain_q_eval_all_flags(ta, tb):
    c = matmul_circuit(5, 3, 7, ta, tb)
    for x in matmul_inputs(5, 3, 7, ta, tb, rounds=3):
        out = c.plain_q_eval(x, False)
        assert out.dtype == np.int64
        np.testing.assert_array_equal(out, expected(5, 3, 7, x, ta, tb))


def test_extremes_are_hit_and_nothing_wraps():
    for M, T, N in [(1, 5, 1), (7, 3, 11), (16, 2, 16), (13, 4, 20)]:
        lim = lim_of(T)
        outs = np.concatenate([expected(M, T, N, x) for x in matmul_inputs(M, T, N, rounds=7)])
        assert np.abs(outs).max() == T * lim * lim < M7 // 2
        assert (outs == T * lim * lim).any() and (outs == 0).any()
        if M > 1:
            assert (outs == -T * lim * lim).any()


def test_overflow_is_an_error():
    l = d.MatMul((1, 4), 0, (4, 1))
    big = np.full(4, 1 << 30, dtype=np.int64)
    with pytest.raises(OverflowError, match="matmul"):
        l.plain_q_eval(big, False, [None, big])  # 4 * 2^30 * 2^30 = 2^62
    small = np.full(4, (1 << 30) - 1, dtype=np.int64)
    assert int(l.plain_q_eval(small, False, [None, big])[0]) == 4 * ((1 << 30) - 1) * (1 << 30)


# ---------------------------------------------------------------- 2. host garbler and evaluator
HOST_SHAPES = [(1, 1, 1), (1, 5, 1), (3, 1, 4), (7, 3, 11), (15, 2, 17), (16, 2, 16), (13, 4, 20), (16, 17, 16)]


@pytest.mark.parametrize("shape", HOST_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_host_garble_and_evaluate(shape):
    c = matmul_circuit(*shape)
    gcs = [GarbledCircuit(c, 7, 100.0, seed=bytes([s]) * 16) for s in (1, 2)]
    for gc, x in zip(gcs, matmul_inputs(*shape)):
        y = _host_eval(gc, x)
        np.testing.assert_array_equal(y, c.plain_q_eval(x, False, M7))
        np.testing.assert_array_equal(y, expected(*shape, x))
    a, b = (g.model.layer_arrays(1) for g in gcs)
    assert set(a) == {"g", "e"}
    for name in a:  # two seeds, different tables
        assert a[name].shape == b[name].shape and not np.array_equal(a[name], b[name])
    assert gcs[0].model.layer_kind(1) == 22 and native().kind_name(22) == "matmul"


@pytest.mark.parametrize("ta,tb", FLAGS, ids=["nn", "nt", "tn", "tt"])
def test_host_transposes(ta, tb):
    c = matmul_circuit(5, 3, 7, ta, tb)
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED)
    for x in matmul_inputs(5, 3, 7, ta, tb):
        np.testing.assert_array_equal(_host_eval(gc, x), expected(5, 3, 7, x, ta, tb))


def test_host_gram_and_out_dims():
    """src = the layer's own input: the general product, no square shortcut (the params keep src and the flags)."""
    c = gram_circuit(6, 5)
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED)
    p = gc.model.layer_params(0)
    assert list(p["src"]) == [-1] and list(p["tb"]) == [1] and "sq" not in p and "ta" not in p
    for x in gram_inputs(6, 5):
        np.testing.assert_array_equal(_host_eval(gc, x), gram_expected(6, 5, x))
    c2 = matmul_circuit(4, 3, 6, out_dims=(2, 3, 4))
    assert c2.output_dims == (2, 3, 4)
    x = matmul_inputs(4, 3, 6)[0]
    np.testing.assert_array_equal(_host_eval(GarbledCircuit(c2, 7, 100.0, seed=SEED), x), expected(4, 3, 6, x))


def test_entry_counts_and_table_bytes():
    n = native()
    for T in (1, 3, 16):
        assert n.matmul_entries(CRT7, T) == 2 * P7 * T
    assert n.matmul_entries(CRT7, 16) == 16 * n.mul_entries(CRT7, False)
    for M, T, N in HOST_SHAPES:
        gc = GarbledCircuit(matmul_circuit(M, T, N), 7, 100.0, seed=SEED)
        arrs = gc.model.layer_arrays(1)
        assert all(np.asarray(a).shape[0] == M * N * T for a in arrs.values())
        nbytes = sum(int(np.asarray(a).nbytes) for a in arrs.values())
        assert nbytes == 16 * M * N * n.matmul_entries(CRT7, T)
    params = GarbledCircuit(matmul_circuit(5, 3, 7, True, False), 7, 100.0, seed=SEED).model.layer_params(1)
    assert [list(params[k]) for k in ("src", "M", "T", "N", "ta")] == [[0], [5], [3], [7], [1]] and "tb" not in params


# ---------------------------------------------------------------- 3. wire format
def test_serialize_roundtrip():
    shape = (5, 3, 7)
    c = matmul_circuit(*shape, True, True)
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED)
    blob = gc.model.serialize()
    back = native().GarbledModel.deserialize(blob)
    assert bytes(back.serialize()) == bytes(blob)
    x = matmul_inputs(*shape, True, True)[0]
    enc = gc.garble_inputs(x)
    a, b = gc.cpu_evaluate(enc), native().cpu_evaluate(back, enc, 0)
    for (pa, la), (pb, lb) in zip(a, b):
        assert pa == pb
        np.testing.assert_array_equal(la, lb)
    np.testing.assert_array_equal(gc.decode_outputs(b), expected(*shape, x, True, True))


# ---------------------------------------------------------------- 4. refusals
def test_hardened_only():
    c = matmul_circuit(2, 2, 2)
    with pytest.raises(ValueError, match=r"layer 1 \(matmul\).*hardened"):
        GarbledCircuit(c, 7, 100.0, seed=SEED, hardened=False)
    with pytest.raises(ValueError, match=r"layer 0 \(matmul\).*hardened"):
        GarbledCircuit(gram_circuit(2, 2), 7, 100.0, seed=SEED, fused_sign=False)


# ---------------------------------------------------------------- 5. zoo and trainer
def test_tiny_nonlocal_on_the_host():
    c, xs = tiny_arch("_TINY_NONLOCAL", TINY_NONLOCAL)
    assert c.required_crt_modulus() <= M7
    mms = [l for l in c.layers if isinstance(l, d.MatMul)]
    assert len(mms) == 2
    f, y = mms
    assert (f.M, f.T, f.N) == (16, 2, 16) and f.trans_a and not f.trans_b and f.out_dims == (16, 16)
    assert (y.M, y.T, y.N) == (2, 16, 16) and y.trans_b and not y.trans_a and y.out_dims == (2, 4, 4)
    assert y.src == c.layers.index(f) + 1 and isinstance(c.layers[y.src], d.Rescale) and y.in_src is not None
    assert isinstance(c.layers[c.layers.index(y) + 1], d.Rescale)
    add = next(l for l in c.layers if isinstance(l, d.Add))
    assert isinstance(c.layers[add.src], d.Relu)  # the block's input
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED)
    assert gc.hardened
    for x in xs:
        np.testing.assert_array_equal(_host_eval(gc, x), c.plain_q_eval(x, False, M7))


def test_nonlocal_block_is_the_dot_product_block():
    """The float model of the tiny architecture against the block written out in numpy."""
    c, _ = tiny_arch("_TINY_NONLOCAL_F", TINY_NONLOCAL)
    conv0, phi, g, theta, back = [l for l in c.layers if isinstance(l, d.Conv2d)]
    x = np.random.default_rng(1).uniform(-1, 1, 64).astype(np.float32)
    a = np.maximum(conv0.plain_eval(x, False), 0)

    def one(l):
        return l.weights.reshape(l.weights.shape[0], -1) @ a.reshape(4, 16) + l.biases[:, None]

    f = one(theta).T @ one(phi)
    yv = one(g) @ f.T
    z = back.weights.reshape(4, 2) @ yv + back.biases[:, None] + a.reshape(4, 16)
    head = c.layers[-2]
    ref = head.weights @ np.maximum(z, 0).sum(axis=1) + head.biases
    np.testing.assert_allclose(c.plain_eval(x, False), ref, rtol=1e-4, atol=1e-5)


def test_zoo_model_and_trainer():
    from dash_amd.models import train, zoo

    c = zoo.build_circuit("NONLOCAL_CIFAR", Q.ScaleQuant, 5, seed=0)
    mms = [l for l in c.layers if isinstance(l, d.MatMul)]
    assert [(l.M, l.T, l.N) for l in mms] == [(64, 16, 64), (16, 64, 64)]
    with pytest.raises(NotImplementedError, match="nonlocal"):
        train.build_torch_model("NONLOCAL_CIFAR")
    zoo.ARCHS["_BIG_NONLOCAL"] = {"input": (2, 16, 16), "ops": [("nonlocal", 2)]}
    try:
        with pytest.raises(ValueError, match="H W <= 64"):
            zoo.build_circuit("_BIG_NONLOCAL", Q.ScaleQuant, 5)
    finally:
        del zoo.ARCHS["_BIG_NONLOCAL"]


# ---------------------------------------------------------------- 6. ONNX
def _nonlocal_onnx(tmp_path, extra=None, gemm=False):
    """theta, phi, g: 1x1 convs 2 -> 3 on [1, 2, 4, 4]; f = Reshape(theta)^T Reshape(phi); y = Reshape(g) f^T,
    reshaped back to [1, 3, 4, 4]."""
    from dash_amd.ir import onnx as o

    rng = np.random.default_rng(3)
    inits = {"wt": _f32(rng, 3, 2, 1, 1), "bt": _f32(rng, 3), "wp": _f32(rng, 3, 2, 1, 1), "bp": _f32(rng, 3),
             "wg": _f32(rng, 3, 2, 1, 1), "bg": _f32(rng, 3), "s316": np.asarray([1, 3, 16], np.float32),
             "s344": np.asarray([1, 3, 4, 4], np.float32)}
    mm = (lambda a, b, out, name: o._node("Gemm", [a, b], [out], name)) if gemm else \
        (lambda a, b, out, name: o._node("MatMul", [a, b], [out], name))
    nodes = [o._node("Conv", ["input", "wt", "bt"], ["th"], "theta", _conv_attrs(1)),
             o._node("Conv", ["input", "wp", "bp"], ["ph"], "phi", _conv_attrs(1)),
             o._node("Conv", ["input", "wg", "bg"], ["g"], "g", _conv_attrs(1)),
             o._node("Reshape", ["th", "s316"], ["thm"], "r_theta"),
             o._node("Transpose", ["thm"], ["tht"], "t_theta", o._attr_ints("perm", [0, 2, 1])),
             o._node("Reshape", ["ph", "s316"], ["phm"], "r_phi"),
             mm("tht", "phm", "f", "mm_f"),
             o._node("Reshape", ["g", "s316"], ["gm"], "r_g"),
             o._node("Transpose", ["f"], ["ft"], "t_f", o._attr_ints("perm", [0, 2, 1])),
             mm("gm", "ft", "ym", "mm_y"),
             o._node("Reshape", ["ym", "s344"], ["y"], "r_y")]
    nodes += extra or []
    return _onnx_model(tmp_path / "nl.onnx", nodes, inits, (1, 2, 4, 4), "y", (1, 3, 4, 4)), inits


@pytest.mark.parametrize("gemm", [False, True], ids=["matmul", "gemm"])
def test_onnx_import(tmp_path, gemm):
    from dash_amd.ir.onnx import load_onnx_model

    path, inits = _nonlocal_onnx(tmp_path, gemm=gemm)
    c = load_onnx_model(path, Q.ScaleQuant, 5)
    assert [l.name for l in c.layers] == ["conv2d", "rescale"] * 3 + ["matmul", "rescale"] * 2
    f, y = c.layers[6], c.layers[8]
    assert (f.in_dims, f.src_dims, f.trans_a, f.trans_b, f.out_dims) == ((3, 16), (3, 16), True, False, (16, 16))
    assert (f.in_src, f.src) == (1, 3)                # theta's and phi's rescales
    assert (y.in_dims, y.src_dims, y.trans_a, y.trans_b, y.out_dims) == ((3, 16), (16, 16), False, True, (3, 4, 4))
    assert (y.in_src, y.src) == (5, 7)                # g's rescale, f's rescale
    assert c.layers[7].l == 5 and c.layers[9].l == 5  # the scheme's rescale behind each, as after a Mul
    assert c.output_dims == (3, 4, 4)
    x = np.random.default_rng(1).uniform(-1, 1, 32).astype(np.float32)

    def conv(w, b):
        return inits[w].reshape(3, 2) @ x.reshape(2, 16) + inits[b][:, None]

    fm = conv("wt", "bt").T @ conv("wp", "bp")
    np.testing.assert_allclose(c.plain_eval(x, False), (conv("wg", "bg") @ fm.T).reshape(-1), rtol=1e-4, atol=1e-5)
    assert [l.name for l in load_onnx_model(path, Q.SimpleQuant).layers] == ["conv2d"] * 3 + ["matmul"] * 2


def test_onnx_gemm_flags(tmp_path):
    from dash_amd.ir import onnx as o
    from dash_amd.ir.onnx import load_onnx_model

    rng = np.random.default_rng(5)
    inits = {"w0": _f32(rng, 6, 6), "b0": _f32(rng, 6), "w1": _f32(rng, 6, 6), "b1": _f32(rng, 6),
             "s23": np.asarray([1, 2, 3], np.float32)}
    nodes = [o._node("Gemm", ["input", "w0", "b0"], ["h0"], "fc0", o._attr_int("transB", 1)),
             o._node("Gemm", ["input", "w1", "b1"], ["h1"], "fc1", o._attr_int("transB", 1)),
             o._node("Reshape", ["h0", "s23"], ["a"], "ra"), o._node("Reshape", ["h1", "s23"], ["b"], "rb"),
             o._node("Gemm", ["a", "b"], ["y"], "gram", o._attr_int("transA", 1))]
    c = load_onnx_model(_onnx_model(tmp_path / "g.onnx", nodes, inits, (1, 6), "y", (1, 3, 3)), Q.ScaleQuant, 5)
    mm = next(l for l in c.layers if isinstance(l, d.MatMul))
    assert (mm.M, mm.T, mm.N, mm.trans_a, mm.trans_b) == (3, 2, 3, True, False)
    x = rng.uniform(-1, 1, 6).astype(np.float32)
    h0, h1 = inits["w0"] @ x + inits["b0"], inits["w1"] @ x + inits["b1"]
    np.testing.assert_allclose(c.plain_eval(x, False), (h0.reshape(2, 3).T @ h1.reshape(2, 3)).reshape(-1), rtol=1e-4,
                               atol=1e-5)


def test_onnx_refusals(tmp_path):
    from dash_amd.ir import onnx as o
    from dash_amd.ir.onnx import load_onnx_model

    rng = np.random.default_rng(6)
    inits = {"w0": _f32(rng, 3, 2, 1, 1), "b0": _f32(rng, 3), "w1": _f32(rng, 3, 2, 1, 1), "b1": _f32(rng, 3),
             "s316": np.asarray([1, 3, 16], np.float32), "s34": np.asarray([1, 3, 4], np.float32)}
    convs = [o._node("Conv", ["input", "w0", "b0"], ["a"], "c0", _conv_attrs(1)),
             o._node("Conv", ["input", "w1", "b1"], ["b"], "c1", _conv_attrs(1))]

    def load(nodes, out_dims=(1, 3, 3)):
        return load_onnx_model(_onnx_model(tmp_path / "r.onnx", convs + nodes, inits, (1, 2, 4, 4), "y", out_dims),
                               Q.ScaleQuant, 5)

    # more than one matrix per operand: (3, 4, 4) behind the batch axis
    with pytest.raises(NotImplementedError, match="heads0.*batch of more than one matrix"):
        load([o._node("MatMul", ["a", "b"], ["y"], "heads0")], (1, 3, 4, 4))
    # a Transpose that does not swap the last two axes, and one that feeds something else
    with pytest.raises(NotImplementedError, match="perm0"):
        load([o._node("Transpose", ["a"], ["y"], "perm0", o._attr_ints("perm", [0, 2, 1, 3]))], (1, 4, 3, 4))
    with pytest.raises(NotImplementedError, match="lone0"):
        load([o._node("Reshape", ["a", "s316"], ["am"], "ra"),
              o._node("Transpose", ["am"], ["at"], "lone0", o._attr_ints("perm", [0, 2, 1])),
              o._node("Relu", ["at"], ["y"], "relu0")], (1, 16, 3))
    # a pending average factor on an operand
    with pytest.raises(NotImplementedError, match="avg0.*pending"):
        load([o._node("AveragePool", ["a"], ["ap"], "ap", o._attr_ints("kernel_shape", [2, 2])
                      + o._attr_ints("strides", [2, 2])),
              o._node("AveragePool", ["b"], ["bp"], "bp", o._attr_ints("kernel_shape", [2, 2])
                      + o._attr_ints("strides", [2, 2])),
              o._node("Reshape", ["ap", "s34"], ["am"], "ra"), o._node("Reshape", ["bp", "s34"], ["bm"], "rb"),
              o._node("Transpose", ["am"], ["at"], "ta", o._attr_ints("perm", [0, 2, 1])),
              o._node("MatMul", ["at", "bm"], ["y"], "avg0")], (1, 4, 4))
    # a Gemm with alpha != 1
    with pytest.raises(NotImplementedError, match="alpha0"):
        load([o._node("Reshape", ["a", "s316"], ["am"], "ra"), o._node("Reshape", ["b", "s316"], ["bm"], "rb"),
              o._node("Gemm", ["am", "bm"], ["y"], "alpha0", o._attr_float("alpha", 0.5) + o._attr_int("transB", 1))])
    # inner sizes that differ: the message names both shapes
    with pytest.raises(ValueError, match=r"shape0.*\(3, 16\).*\(3, 16\)"):
        load([o._node("Reshape", ["a", "s316"], ["am"], "ra"), o._node("Reshape", ["b", "s316"], ["bm"], "rb"),
              o._node("MatMul", ["am", "bm"], ["y"], "shape0")])


def test_onnx_initializer_operand_is_a_dense_as_before(tmp_path):
    from dash_amd.ir import onnx as o
    from dash_amd.ir.onnx import load_onnx_model

    rng = np.random.default_rng(7)
    inits = {"w": _f32(rng, 6, 4)}
    c = load_onnx_model(_onnx_model(tmp_path / "d.onnx", [o._node("MatMul", ["input", "w"], ["y"], "mm")], inits,
                                    (1, 6), "y", (1, 4)), Q.ScaleQuant, 5)
    assert [l.name for l in c.layers] == ["dense", "rescale"]


def test_onnx_export_import_is_the_identity(tmp_path):
    from dash_amd.ir.onnx import load_onnx_model, parse_onnx, save_onnx_model

    c, xs = tiny_arch("_TINY_NONLOCAL_RT", TINY_NONLOCAL)
    path = tmp_path / "rt.onnx"
    save_onnx_model(path, c)
    ops = [n["op_type"] for n in parse_onnx(path)["nodes"]]
    assert ops.count("MatMul") == 2 and ops.count("Transpose") == 2 and ops.count("Reshape") == 4
    back = load_onnx_model(path, Q.ScaleQuant, 5)
    assert [l.name for l in back.layers] == [l.name for l in c.layers]
    assert [l.in_src for l in back.layers] == [l.in_src for l in c.layers]
    for (ka, pa), (kb, pb) in zip(back.garble_specs(), c.garble_specs()):
        assert ka == kb
        if ka in (d.ir.layers.Kind.MATMUL, d.ir.layers.Kind.RESCALE):
            assert pa == pb
    assert [l.out_dims for l in back.layers] == [l.out_dims for l in c.layers]
    for x in xs:
        np.testing.assert_array_equal(back.plain_q_eval(x, False, M7), c.plain_q_eval(x, False, M7))


# ---------------------------------------------------------------- 7. range guard
def test_range_guard_numpy_and_torch_agree():
    c, xs, want = guard_case()
    g = RangeGuard(c, M7, mrs=True)
    assert g.batched and not g.native_forms
    assert [bool(g.violations_np(x)) for x in xs] == want
    assert g.submit(xs).bad_indices() == [i for i, w in enumerate(want) if w]
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED, rescale="mrs")
    np.testing.assert_array_equal(_host_eval(gc, xs[0]), c.plain_q_eval(xs[0], False, M7))


def test_range_guard_torch_path_is_exact_and_flags_overflow():
    """k = 15: M / 2 is about 2^58, beyond float64's integers. The torch path contracts in int64 and gives the
    numpy verdict on both sides of M / 2; operands whose T products could reach 2^62 are refused by both (the numpy
    model's OverflowError), never wrapped."""
    from dash_amd.ir.bases import crt_modulus

    M = crt_modulus(first_primes(15))
    h = M // 2
    assert (1 << 53) < h < (1 << 62)
    sel = d.Dense.from_quantized(np.eye(2, dtype=np.int64)[::-1].copy(), np.zeros(2, dtype=np.int64))
    mm = d.MatMul((1, 2), 0, (2, 1), out_dims=(1,))
    mm.in_src = -1
    c = d.Circuit([sel, mm, d.Relu((1,))])  # out = 2 x0 x1 feeds a sign
    a = (1 << 28) + 3
    b = (h - 1) // (2 * a)
    assert (1 << 53) < 2 * a * b < h <= 2 * a * (b + 1)
    # y is x reversed, so max|x| = max|y| = m and the bound is T m^2 = 2 m^2 against 2^62: the largest m inside it,
    # and the first outside (whose actual sum 2 * 5 (m + 1) is tiny: the bound is on the operands, as for Mul)
    m = math.isqrt((1 << 61) - 1)
    assert 2 * m * m < (1 << 62) <= 2 * (m + 1) * (m + 1)
    xs = [np.array([a, b]), np.array([a, b + 1]), np.array([-a, b + 1]), np.array([-a, b]),
          np.array([m, 5]), np.array([m + 1, 5]), np.array([-(m + 1), 5])]
    g = RangeGuard(c, M, mrs=True)
    verdict = [bool(g.violations_np(x)) for x in xs]
    assert verdict == [False, True, True, False, False, True, True]
    assert g.submit(xs).bad_indices() == [i for i, v in enumerate(verdict) if v]
