"""The Mul layer on the host: semantics, the generalized half gates and the square projection of csrc/gadgets.h
MulPlan through the host garbler and evaluator, table sizes, the wire format, refusals, the per-element gate tweak,
ONNX import and export, the zoo ops and the range guard (docs/MUL.md)."""
from __future__ import annotations

import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit, RangeGuard
from dash_amd.ir.bases import first_primes
from dash_amd.ir.quant import QuantizationMethod as Q
from dash_amd.native import native
from tests.mul_cases import (LIM, M7, TINY_SE, TINY_SQUARE, expected, guard_case, mul_circuit, mul_inputs, tiny_arch)
from tests.test_argmax import GOLDEN, parent_circuit
from tests.test_clip import _conv_attrs, _f32, _onnx_model

SEED = bytes(range(16))
CRT7 = first_primes(7)
P7 = sum(CRT7)  # 58


def _host_eval(gc, x):
    return gc.decode_outputs(gc.cpu_evaluate(gc.garble_inputs(x)))


def _u128(a) -> int:
    """One table entry of a layer array as a Python int."""
    return int.from_bytes(np.ascontiguousarray(a).tobytes(), "little")


# ---------------------------------------------------------------- 1. semantics
@pytest.mark.parametrize("dims,src_dims,bc", [((7,), None, 0), ((3, 4, 5), None, 0), ((3, 4, 5), (3,), 20),
                                               ((3, 4, 5), (3, 1, 1), 20), ((3, 1, 1), (3, 1, 1), 1)])
def test_semantics(dims, src_dims, bc):
    rng = np.random.default_rng(0)
    N, ny = int(np.prod(dims)), int(np.prod(src_dims or dims))
    m = d.Mul(dims, -1, src_dims)
    assert (m.kind, m.name, d.ir.layers.Kind.MUL, m.bc) == (19, "mul", 19, bc)
    assert m.garble_spec() == (19, {"src": -1, "bc": bc} if bc else {"src": -1})
    x, y = rng.integers(-LIM, LIM + 1, N), rng.integers(-LIM, LIM + 1, ny)
    want = (x.reshape(dims[0], -1) * y.reshape(dims[0], 1)).reshape(-1) if bc else x * y
    got = m.plain_q_eval(x, True, [y])
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, want)
    assert m.get_max_plain_q_val() == max(x.max(), y.max(), want.max())
    assert m.get_min_plain_q_val() == min(x.min(), y.min(), want.min())
    f = m.plain_eval(x.astype(np.float32), False, [y.astype(np.float32)])
    assert f.dtype == np.float32
    np.testing.assert_array_equal(f, want.astype(np.float32))


def test_square_forms():
    sq = d.Mul.square((5,))
    assert sq.is_square and sq.garble_spec() == (19, {"sq": 1})
    x = np.array([-LIM, -1, 0, 2, LIM])
    np.testing.assert_array_equal(sq.plain_q_eval(x, False, [x]), x * x)
    np.testing.assert_array_equal(sq.plain_eval(x, False, [x]), (x * x).astype(np.float32))
    # a src that names the layer's own input is the same tensor twice
    same = d.Mul((5,), 0)
    same.in_src = 0
    assert same.is_square and same.garble_spec() == (19, {"sq": 1})
    other = d.Mul((5,), 0)
    other.in_src = -1
    assert not other.is_square and other.garble_spec() == (19, {"src": 0})


def test_square_by_position_in_the_circuit():
    """A sequential Mul whose src is the layer before it (or the circuit input, as layer 0) reads one tensor twice:
    Circuit.garble_specs, which knows the layer's index, garbles it as the square."""
    first = d.Circuit([d.Mul((5,), -1)])
    assert first.garble_specs() == [(19, {"sq": 1})]
    seq = d.Circuit([d.Flatten((5,)), d.Mul((5,), 0)])
    assert seq.garble_specs()[1] == (19, {"sq": 1})
    skip = d.Circuit([d.Flatten((5,)), d.Mul((5,), -1)])  # the input through a Flatten is another layer's output
    assert skip.garble_specs()[1] == (19, {"src": -1})
    bc = d.Circuit([d.Flatten((3, 1, 1)), d.Mul((3, 1, 1), 0, (3, 1, 1))])  # an explicit broadcast stays a product
    assert bc.garble_specs()[1] == (19, {"src": 0, "bc": 1})
    x = np.array([-LIM, -1, 0, 2, LIM])
    for c in (first, seq):
        gc = GarbledCircuit(c, 7, 100.0, seed=SEED)
        assert set(gc.model.layer_arrays(len(c.layers) - 1)) == {"t"}
        np.testing.assert_array_equal(_host_eval(gc, x), x * x)
    with pytest.raises(ValueError, match="mul"):
        d.Mul((3, 4, 5), None, (3,))


@pytest.mark.parametrize("dims,src_dims", [((3, 4, 5), (4,)), ((3, 4, 5), (3, 4, 1)), ((3, 4, 5), (1, 4, 5)),
                                           ((3,), (3, 4, 5)), ((6,), (3,)), ((3, 4, 5), (3, 1))])
def test_bad_shapes(dims, src_dims):
    with pytest.raises(ValueError, match="mul"):
        d.Mul(dims, -1, src_dims)


def test_overflow_is_an_error():
    m = d.Mul((2,), -1)
    big = np.array([1 << 31, 3], dtype=np.int64)
    with pytest.raises(OverflowError, match="mul"):
        m.plain_q_eval(big, False, [np.array([1 << 31, -3], dtype=np.int64)])
    ok = np.array([(1 << 31) - 1, 3], dtype=np.int64)  # (2^31 - 1) 2^31 < 2^62
    np.testing.assert_array_equal(m.plain_q_eval(ok, False, [np.array([1 << 31, 2])]),
                                  [((1 << 31) - 1) << 31, 6])


# ---------------------------------------------------------------- 2. host garbler and evaluator
HOST_CASES = [((1,), "elem"), ((77,), "elem"), ((3, 4, 5), "bc1"), ((3, 4, 5), "bc3"), ((5,), "sq")]


@pytest.mark.parametrize("dims,kind", HOST_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_host_garble_and_evaluate(dims, kind):
    c = mul_circuit(dims, kind)
    li = len(c.layers) - 1
    gcs = [GarbledCircuit(c, 7, 100.0, seed=bytes([s]) * 16) for s in (1, 2)]
    for gc, x in zip(gcs, mul_inputs(dims, kind)):
        y = _host_eval(gc, x)
        np.testing.assert_array_equal(y, c.plain_q_eval(x, False, M7))
        np.testing.assert_array_equal(y, expected(dims, kind, x))
    a, b = (g.model.layer_arrays(li) for g in gcs)
    assert set(a) == ({"t"} if kind == "sq" else {"g", "e"})
    for name in a:  # two seeds, different tables
        assert a[name].shape == b[name].shape and not np.array_equal(a[name], b[name])
    assert gcs[0].model.layer_kind(li) == 19 and native().kind_name(19) == "mul"


def test_entry_counts():
    n = native()
    assert (n.mul_entries(CRT7, False), n.mul_entries(CRT7, True)) == (116, 58) == (2 * P7, P7)
    for dims, kind in HOST_CASES:
        gc = GarbledCircuit(mul_circuit(dims, kind), 7, 100.0, seed=SEED)
        arrs = gc.model.layer_arrays(len(gc.circuit.layers) - 1)
        N = int(np.prod(dims))
        assert sum(int(np.asarray(a).nbytes // 16) for a in arrs.values()) == N * n.mul_entries(CRT7, kind == "sq")
    params = GarbledCircuit(mul_circuit((3, 4, 5), "bc1"), 7, 100.0, seed=SEED).model.layer_params(1)
    assert list(params["bc"]) == [20] and list(params["src"]) == [0] and "sq" not in params
    assert "bc" not in GarbledCircuit(mul_circuit((77,), "elem"), 7, 100.0, seed=SEED).model.layer_params(1)


# ---------------------------------------------------------------- 3. wire format
@pytest.mark.parametrize("dims,kind", [((3, 4, 5), "bc3"), ((5,), "sq")], ids=["bc", "sq"])
def test_serialize_roundtrip(dims, kind):
    c = mul_circuit(dims, kind)
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED)
    blob = gc.model.serialize()
    back = native().GarbledModel.deserialize(blob)
    assert bytes(back.serialize()) == bytes(blob)
    x = mul_inputs(dims, kind)[0]
    enc = gc.garble_inputs(x)
    a, b = gc.cpu_evaluate(enc), native().cpu_evaluate(back, enc, 0)
    for (pa, la), (pb, lb) in zip(a, b):
        assert pa == pb
        np.testing.assert_array_equal(la, lb)
    np.testing.assert_array_equal(gc.decode_outputs(b), expected(dims, kind, x))


def test_circuits_without_mul_keep_their_bytes():
    """The golden file is the offline message of tests.test_argmax.parent_circuit() written before the Mul layer
    existed (k = 7, garbler seed 0..15, rescale="mrs", relu="joint"); the same circuit, which has no Mul, still
    serializes to these bytes."""
    c, _ = parent_circuit()
    assert not any(isinstance(l, d.Mul) for l in c.layers)
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED, rescale="mrs", relu="joint")
    assert bytes(gc.model.serialize()) == GOLDEN.read_bytes()


# ---------------------------------------------------------------- 4. refusals
def test_hardened_only():
    c = mul_circuit((5,), "elem")
    with pytest.raises(ValueError, match=r"layer 1 \(mul\).*hardened"):
        GarbledCircuit(c, 7, 100.0, seed=SEED, hardened=False)
    with pytest.raises(ValueError, match=r"layer 0 \(mul\).*hardened"):
        GarbledCircuit(mul_circuit((5,), "sq"), 7, 100.0, seed=SEED, fused_sign=False)


# ---------------------------------------------------------------- 5. security: the gate tweak
def test_broadcast_rows_of_one_label_have_their_own_pads():
    """One y label of a broadcast keys the e rows of all H W elements of its channel. Each row is masked under its
    own element's gate id: the pads of two elements of a channel differ, each unmasks its own row to the payload
    the evaluator's formula out = E + colour(y) x - G needs, and neither unmasks the other's."""
    n = native()
    dims = (2, 1, 3)
    c = mul_circuit(dims, "bc1")
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED)
    x = mul_inputs(dims, "bc1")[0]
    enc = gc.garble_inputs(x)
    out = gc.cpu_evaluate(enc)
    # y = layer 0's output: evaluate the selection alone to get its active labels
    sel = GarbledCircuit(d.Circuit([c.layers[0]]), 7, 100.0, seed=SEED)
    ylab = sel.cpu_evaluate(sel.garble_inputs(x))
    arrs = gc.model.layer_arrays(1)
    L, TW_MMG, TW_GME = 2, 5, 12
    prefix = np.concatenate([[0], np.cumsum(CRT7)[:-1]])
    for j in (1, 6):  # p = 3 and p = 17
        p = CRT7[j]
        for ch in range(2):
            K = n.compress(ylab[j][1][ch], p)
            coly = int(ylab[j][1][ch][0]) % p
            pads = {}
            for e in (3 * ch, 3 * ch + 2):
                gate = n.stream_id(L, 1, e)
                pads[e] = n.hard_pads(K, gate, (TW_GME << 16) | j, 0)[0]
                xl = np.asarray(enc[j][1][e], dtype=np.int64)
                colx = int(xl[0]) % p
                Hx = n.hard_pads(n.compress(enc[j][1][e], p), gate, (TW_MMG << 16) | j, 0)[0]
                G = n.decompress((_u128(arrs["g"][e, prefix[j] + colx]) - Hx) % (1 << 128), p).astype(np.int64)
                E = n.decompress((_u128(arrs["e"][e, prefix[j] + coly]) - pads[e]) % (1 << 128), p).astype(np.int64)
                np.testing.assert_array_equal((E + coly * xl - G) % p, np.asarray(out[j][1][e], dtype=np.int64) % p)
            e1, e2 = sorted(pads)
            assert pads[e1] != pads[e2]
            wrong = n.decompress((_u128(arrs["e"][e1, prefix[j] + coly]) - pads[e2]) % (1 << 128), p)
            right = n.decompress((_u128(arrs["e"][e1, prefix[j] + coly]) - pads[e1]) % (1 << 128), p)
            assert not np.array_equal(wrong, right)


# ---------------------------------------------------------------- 6. ONNX
def _se_like_onnx(tmp_path, order, gate_shape4=True):
    """Conv(2 -> 3, 1x1) -> x [1, 3, 4, 4]; GlobalAveragePool(x) -> Conv(3 -> 3, 1x1) -> gate [1, 3, 1, 1] (or
    Flatten to [1, 3]); Mul(x, gate) or Mul(gate, x)."""
    from dash_amd.ir import onnx as o

    rng = np.random.default_rng(3)
    inits = {"w0": _f32(rng, 3, 2, 1, 1), "b0": _f32(rng, 3), "w1": _f32(rng, 3, 3, 1, 1), "b1": _f32(rng, 3)}
    nodes = [o._node("Conv", ["input", "w0", "b0"], ["x"], "c0", _conv_attrs(1)),
             o._node("GlobalAveragePool", ["x"], ["gp"], "gp"),
             o._node("Conv", ["gp", "w1", "b1"], ["g4"], "c1", _conv_attrs(1))]
    gate = "g4"
    if not gate_shape4:
        nodes.append(o._node("Flatten", ["g4"], ["g2"], "fl", o._attr_int("axis", 1)))
        gate = "g2"
    nodes.append(o._node("Mul", ["x", gate] if order == "xg" else [gate, "x"], ["y"], "mul0"))
    return _onnx_model(tmp_path / "se.onnx", nodes, inits, (1, 2, 4, 4), "y", (1, 3, 4, 4)), inits


@pytest.mark.parametrize("order", ["xg", "gx"])
@pytest.mark.parametrize("shape4", [True, False], ids=["NC11", "NC"])
def test_onnx_broadcast_import_both_orders(tmp_path, order, shape4):
    from dash_amd.ir.onnx import load_onnx_model

    path, inits = _se_like_onnx(tmp_path, order, shape4)
    c = load_onnx_model(path, Q.ScaleQuant, 5)
    mul = next(l for l in c.layers if isinstance(l, d.Mul))
    i = c.layers.index(mul)
    assert mul.in_dims == (3, 4, 4) and mul.bc == 16 and mul.src_dims == ((3, 1, 1) if shape4 else (3,))
    assert mul.in_src == 1 and mul.src == i - 1  # x: the first conv's rescale; the gate: the layer before the Mul
    assert isinstance(c.layers[i + 1], d.Rescale) and c.layers[i + 1].l == 5
    x = np.random.default_rng(1).uniform(-1, 1, 32).astype(np.float32)
    xin = x.reshape(2, 16)
    a = inits["w0"].reshape(3, 2) @ xin + inits["b0"][:, None]
    g = inits["w1"].reshape(3, 3) @ a.mean(axis=1) + inits["b1"]
    np.testing.assert_allclose(c.plain_eval(x, False), (a * g[:, None]).reshape(-1), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("form", ["mul_xx", "pow_init", "pow_const"])
def test_onnx_square_forms(tmp_path, form):
    from dash_amd.ir import onnx as o
    from dash_amd.ir.onnx import load_onnx_model
    from tests.test_clip import _const_node

    rng = np.random.default_rng(4)
    inits = {"w0": _f32(rng, 4, 6), "b0": _f32(rng, 4)}
    nodes = [o._node("Gemm", ["input", "w0", "b0"], ["h"], "fc", o._attr_int("transB", 1))]
    if form == "mul_xx":
        nodes.append(o._node("Mul", ["h", "h"], ["y"], "sq"))
    elif form == "pow_init":
        inits["two"] = np.asarray(2.0, np.float32)
        nodes.append(o._node("Pow", ["h", "two"], ["y"], "sq"))
    else:
        nodes += [_const_node("two", 2.0), o._node("Pow", ["h", "two"], ["y"], "sq")]
    c = load_onnx_model(_onnx_model(tmp_path / "sq.onnx", nodes, inits, (1, 6), "y", (1, 4)), Q.ScaleQuantPlus, 32)
    assert [l.name for l in c.layers] == ["dense", "rescale", "mul", "rescale"]
    assert c.layers[2].is_square and c.layers[3].s == [32]
    x = rng.uniform(-1, 1, 6).astype(np.float32)
    np.testing.assert_allclose(c.plain_eval(x, False), (inits["w0"] @ x + inits["b0"]) ** 2, rtol=1e-4, atol=1e-5)


def test_onnx_rescale_per_scheme_and_refusals(tmp_path):
    from dash_amd.ir import onnx as o
    from dash_amd.ir.onnx import load_onnx_model

    rng = np.random.default_rng(5)
    inits = {"w0": _f32(rng, 4, 6), "b0": _f32(rng, 4)}
    fc = o._node("Gemm", ["input", "w0", "b0"], ["h"], "fc", o._attr_int("transB", 1))
    path = _onnx_model(tmp_path / "m.onnx", [fc, o._node("Mul", ["h", "h"], ["y"], "sq")], inits, (1, 6), "y", (1, 4))
    assert [l.name for l in load_onnx_model(path, Q.SimpleQuant).layers] == ["dense", "mul"]
    assert [l.name for l in load_onnx_model(path, Q.ScaleQuant, 5).layers] == ["dense", "rescale", "mul", "rescale"]
    assert load_onnx_model(path, Q.ScaleQuant, 5).layers[3].l == 5
    # an initializer operand
    inits2 = dict(inits, s=_f32(rng, 4))
    path = _onnx_model(tmp_path / "c.onnx", [fc, o._node("Mul", ["h", "s"], ["y"], "scale0")], inits2, (1, 6), "y", (1, 4))
    with pytest.raises(NotImplementedError, match="scale0"):
        load_onnx_model(path, Q.ScaleQuant, 5)
    # another exponent
    inits3 = dict(inits, three=np.asarray(3.0, np.float32))
    path = _onnx_model(tmp_path / "p.onnx", [fc, o._node("Pow", ["h", "three"], ["y"], "cube0")], inits3, (1, 6), "y", (1, 4))
    with pytest.raises(NotImplementedError, match="cube0"):
        load_onnx_model(path, Q.ScaleQuant, 5)
    # another broadcast: [1, 4] against [1, 6]-derived [1, 2] has no channel form
    inits4 = dict(inits, w1=_f32(rng, 2, 6), b1=_f32(rng, 2))
    nodes = [fc, o._node("Gemm", ["input", "w1", "b1"], ["h2"], "fc2", o._attr_int("transB", 1)),
             o._node("Mul", ["h", "h2"], ["y"], "bad0")]
    with pytest.raises(NotImplementedError, match="bad0"):
        load_onnx_model(_onnx_model(tmp_path / "b.onnx", nodes, inits4, (1, 6), "y", (1, 4)), Q.ScaleQuant, 5)


@pytest.mark.parametrize("arch", ["se", "square"])
def test_onnx_export_import_is_the_identity(tmp_path, arch):
    from dash_amd.ir.onnx import load_onnx_model, save_onnx_model

    c, xs = tiny_arch("_TINY_MUL_RT", TINY_SE if arch == "se" else TINY_SQUARE)
    path = tmp_path / "rt.onnx"
    save_onnx_model(path, c)
    back = load_onnx_model(path, Q.ScaleQuant, 5)
    assert [repr(l) for l in back.layers] == [repr(l) for l in c.layers]
    assert [l.in_src for l in back.layers] == [l.in_src for l in c.layers]
    assert [k for k, _ in back.garble_specs()] == [k for k, _ in c.garble_specs()]
    for (ka, pa), (_, pb) in zip(back.garble_specs(), c.garble_specs()):
        if ka in (d.ir.layers.Kind.MUL, d.ir.layers.Kind.RESCALE):
            assert pa == pb
    for x in xs:
        np.testing.assert_array_equal(back.plain_q_eval(x, False, M7), c.plain_q_eval(x, False, M7))


# ---------------------------------------------------------------- 7. zoo and trainer
@pytest.mark.parametrize("arch", ["se", "square"])
def test_tiny_arch_on_the_host(arch):
    c, xs = tiny_arch("_TINY_MUL", TINY_SE if arch == "se" else TINY_SQUARE)
    muls = [l for l in c.layers if isinstance(l, d.Mul)]
    assert len(muls) == (1 if arch == "se" else 2)
    if arch == "se":
        m = muls[0]
        assert m.bc == 36 and m.src_dims == (4, 1, 1) and m.in_src is not None and isinstance(c.layers[m.src], d.Clip)
        assert isinstance(c.layers[c.layers.index(m) + 1], d.Rescale)
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED)
    for x in xs:
        np.testing.assert_array_equal(_host_eval(gc, x), c.plain_q_eval(x, False, M7))


def test_zoo_models_and_trainer():
    from dash_amd.models import train, zoo

    cn = zoo.build_circuit("CRYPTONETS_MNIST", Q.ScaleQuant, 5, seed=0)
    assert [l.name for l in cn.layers if l.name != "rescale"] == ["conv2d", "mul", "flatten", "dense", "mul", "dense"]
    assert all(l.is_square for l in cn.layers if isinstance(l, d.Mul))
    se = zoo.build_circuit("SE_MOBILENET_CIFAR", Q.ScaleQuant, 5, seed=0)
    assert sum(isinstance(l, d.Mul) for l in se.layers) == 3 and all(l.bc for l in se.layers if isinstance(l, d.Mul))
    x = zoo.quantized_inputs("SE_MOBILENET_CIFAR", 1, Q.ScaleQuant, 5, seed=3)[0]
    assert se.plain_q_eval(x, False).shape == (10,)
    with pytest.raises(ValueError, match="se"):
        zoo.build_circuit("SE_MOBILENET_CIFAR", Q.SimpleQuant, -1)
    model = train.build_torch_model("CRYPTONETS_MNIST")
    c = train.to_circuit(model, "CRYPTONETS_MNIST", Q.ScaleQuant, 5)
    assert [l.name for l in c.layers] == [l.name for l in cn.layers]
    with pytest.raises(NotImplementedError, match="se"):
        train.build_torch_model("SE_MOBILENET_CIFAR")


# ---------------------------------------------------------------- 8. range guard
def test_range_guard_numpy_and_torch_agree():
    c, xs, want = guard_case()
    g = RangeGuard(c, M7, mrs=True)
    assert g.batched and not g.native_forms
    assert [bool(g.violations_np(x)) for x in xs] == want
    assert g.submit(xs).bad_indices() == [i for i, w in enumerate(want) if w]
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED, rescale="mrs")
    np.testing.assert_array_equal(_host_eval(gc, xs[0]), c.plain_q_eval(xs[0], False, M7))


def test_range_guard_torch_path_is_exact_above_2_53():
    """k = 15: M / 2 is about 2^58, so products next to it are not representable in float64. The torch path
    multiplies in int64 and gives the numpy verdict on both sides of M / 2; operands whose product would leave
    int64 are refused by both (the numpy model's OverflowError), never wrapped."""
    from dash_amd.ir.bases import crt_modulus

    M = crt_modulus(first_primes(15))
    h = M // 2
    assert (1 << 53) < h < (1 << 62)
    a = (1 << 29) + 3
    b = (h - 1) // a
    assert (1 << 53) < a * b < h <= a * (b + 1)
    c = d.Circuit(mul_circuit((2,), "elem").layers + [d.Relu((2,))])  # the products a b, b a feed a sign
    xs = [np.array([a, b]), np.array([a, b + 1]), np.array([-a, b + 1]), np.array([-a, b]), np.array([1 << 31, 1 << 31]),
          np.array([(1 << 31) - 1, 5])]  # the last two: max|x| max|y| = 2^62 exactly, and just below it
    g = RangeGuard(c, M, mrs=True)
    verdict = [bool(g.violations_np(x)) for x in xs]
    assert verdict == [False, True, True, False, True, False]
    assert g.submit(xs).bad_indices() == [i for i, v in enumerate(verdict) if v]
