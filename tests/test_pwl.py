"""The PiecewiseLinear layer on the host (docs/PWL.md): the exact integer semantics against a per-segment model,
continuity, the constructor's refusals, the accuracy of the sigmoid / tanh interpolants and of their quantized form,
the host garbler and evaluator under every sign construction, the wire format, gate ids and table cost from the
plan, ONNX import / export with the pending scale bits, the range guard, the zoo models and the kernel's digit
formula. Layers and inputs: tests/pwl_cases.py."""
from __future__ import annotations

import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit, RangeGuard
from dash_amd.ir.bases import crt_modulus, first_primes
from dash_amd.ir.quant import QuantizationMethod as Q
from dash_amd.native import native
from tests.pwl_cases import (M7, SHAPES, cardinal, conv_chain, conv_chain_inputs, expected, lim, modq, pwl_circuit,
                             pwl_inputs, pwl_layer, shape_for)
from tests.test_clip import _conv_attrs, _f32, _onnx_model

SEED = bytes(range(16))
CONSTRUCTIONS = {"approx": dict(rescale="mrs", relu="approx"), "mrs": dict(rescale="mrs", relu="mrs"),
                 "joint": dict(rescale="mrs", relu="joint")}
PWL = d.PiecewiseLinear


def _host_eval(gc, x):
    return gc.decode_outputs(gc.cpu_evaluate(gc.garble_inputs(x)))


def _mrs_arg(k):
    return 100.0 if 4 <= k <= 11 else None


# ---------------------------------------------------------------- 1. / 2. semantics
@pytest.mark.parametrize("name", ["m1", "m2", "m8", "drop"])
def test_plain_q_eval_against_segment_model(name):
    T, A, V, s = SHAPES[name]
    l = pwl_layer((40,), name)
    assert (l.kind, l.name, d.ir.layers.Kind.PWL, PWL.MAX_BREAKS) == (21, "pwl", 21, 8)
    assert l.garble_spec() == (21, {"s": s, "T": T, "A": A, "V": V, "fn": 0})
    L = lim(l, 7)
    x = np.array(cardinal(l, 7) + list(np.random.default_rng(0).integers(-L, L + 1, 200)), dtype=np.int64)
    for t in T:
        assert {t - 1, t, t + 1} <= set(x.tolist())
    assert {-L, L} <= set(x.tolist())
    got = l.plain_q_eval(x)
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, expected(x, T, A, V))
    # range tracking: x, y and every sign input x - T_i
    assert l.get_min_plain_q_val() == min(x.min() - T[-1], got.min())
    assert l.get_max_plain_q_val() == max(x.max() - T[0], got.max())
    # the float function with the same (dyadic) slopes at scale 2^s
    f = l.plain_eval(x.astype(np.float64), False)
    np.testing.assert_allclose(f, got / float(1 << s), rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("name", ["m1", "m2", "m8", "drop"])
def test_continuity(name):
    """At every breakpoint the left segment's line gives the value the right segment starts from."""
    T, A, V, s = SHAPES[name]
    l = pwl_layer((1,), name)
    for i, t in enumerate(T):
        at = int(l.plain_q_eval(np.array([t]), False)[0])
        left = int(l.plain_q_eval(np.array([t - 1]), False)[0]) + A[i]
        right = int(l.plain_q_eval(np.array([t + 1]), False)[0]) - A[i + 1]
        assert left == at == right


# ---------------------------------------------------------------- 3. refusals
def test_constructor_refusals():
    with pytest.raises(ValueError, match="increase strictly"):
        PWL((4,), [0.1, 0.2], [0, 1, 0], 0.0, 8, 1)  # both round to 0 at l = 1
    with pytest.raises(ValueError, match="increase strictly"):
        PWL.tanh((4,), 8, 0)  # the knots +-0.5 and +-1 collide at l = 0
    with pytest.raises(ValueError, match="between 1 and 8 breakpoints"):
        PWL((4,), np.arange(9.0), np.zeros(10), 0.0)
    with pytest.raises(ValueError, match="between 1 and 8 breakpoints"):
        PWL.from_quantized((4,), list(range(9)), [0] * 9 + [1], 0, 8)
    with pytest.raises(ValueError, match=r"\|a\| <= 2"):
        PWL((4,), [0.0], [0.0, 2.5], 0.0)
    with pytest.raises(ValueError, match=r"\|A\| <= 512"):
        PWL.from_quantized((4,), [0], [0, 513], 0, 8)
    assert PWL((4,), [0.0], [0.0, -2.0], 0.0).A.tolist() == [0, -512]
    for bits in (0, 9, 2.5):
        with pytest.raises(ValueError, match="slope_bits"):
            PWL((4,), [0.0], [0.0, 1.0], 0.0, bits)
    with pytest.raises(ValueError, match="no breakpoint is left"):
        PWL((4,), [0.0, 1.0], [0.5, 0.5, 0.5], 0.0)
    with pytest.raises(ValueError, match="no breakpoint is left"):
        PWL((4,), [0.0], [0.0, 0.1], 0.0, 2)  # 0.1 * 4 rounds to 0
    for qm, qp in ((Q.SimpleQuant, -1), (Q.ScaleQuantPlus, 32)):
        with pytest.raises(ValueError, match="pwl.*ScaleQuant only"):
            PWL.sigmoid((4,), 8, qp, qm)
    c = pwl_circuit((4,), "m2")
    with pytest.raises(ValueError, match=r"layer 0 \(pwl\).*hardened encoding only"):
        GarbledCircuit(c, 7, 100.0, seed=SEED, hardened=False)
    with pytest.raises(ValueError, match=r"layer 0 \(pwl\).*cannot be hardened"):
        GarbledCircuit(c, 7, 100.0, seed=SEED, fused_sign=False)


def test_dropped_breakpoint_and_tags():
    l = pwl_layer((4,), "drop")
    assert l.D.tolist() == [130, 0, -356] and l.kept == [0, 2]
    p = native().pwl_plan(first_primes(7), 7, [-40, 10, 33], [-30, 100, 100, -256], 1234, 147)
    assert p["T"] == [-40, 33] and p["D"] == [130, -356] and p["C"] == 1234 - 30 * 40
    # the device table [residue][m + 1]: A_0 mod p, D_i mod p, negatives included
    assert p["table"] == [v for q in first_primes(7) for v in ((-30) % q, 130 % q, (-356) % q)]
    s = PWL.sigmoid((4,))
    assert (s.fn, PWL.tanh((4,)).fn, s.slope_bits, s.q_parameter) == ("sigmoid", "tanh", 8, 5)
    h = PWL.hard_sigmoid((4,), 0.2, 0.5)
    assert h.fn == "hard_sigmoid" and h.fn_params == {"alpha": 0.2, "beta": 0.5}
    assert h.T.tolist() == [-80, 80] and h.A.tolist() == [0, 51, 0] and h.V == 0
    assert s.garble_spec()[1]["fn"] == 1 and h.garble_spec()[1]["fn"] == 3
    i = PWL.interpolate((4,), [-1.0, 0.0, 2.0], [0.0, 1.0, 0.0], 4, 3)
    assert i.fn is None and i.T.tolist() == [-8, 0, 16] and i.A.tolist() == [0, 16, -8, 0] and i.V == 0


# ---------------------------------------------------------------- 4. / 5. accuracy
GRID = np.linspace(-10.0, 10.0, 20001)


def test_interpolant_accuracy():
    """The float interpolants on the 20001-point grid: 0.0116 (sigmoid) and 0.0233 (tanh) computed, with room for
    the grid."""
    es = np.abs(PWL.sigmoid((1,)).plain_eval(GRID, False) - 1.0 / (1.0 + np.exp(-GRID))).max()
    et = np.abs(PWL.tanh((1,)).plain_eval(GRID, False) - np.tanh(GRID)).max()
    print(f"sigmoid {es:.5f} tanh {et:.5f}")
    assert es <= 0.0125 and et <= 0.025


@pytest.mark.parametrize("fn", ["sigmoid", "tanh", "hard_sigmoid"])
@pytest.mark.parametrize("l,s", [(5, 8), (5, 6), (8, 8), (3, 4)])
def test_quantization_error_bound(fn, l, s):
    """|y_q / 2^(l + s) - plain_eval| on every quantized input of [-10, 10] stays within the bound derived from the
    layer's own floats: slope rounding (t_m - t_1) 2^-(s + 1), knot rounding sum_i |a_i - a_(i-1)| 2^-(l + 1),
    value rounding 2^-(l + s + 1)."""
    lay = getattr(PWL, fn)((1,), slope_bits=s, q_parameter=l)
    xq = np.arange(-10 * (1 << l), 10 * (1 << l) + 1, dtype=np.int64)
    yq = lay.plain_q_eval(xq, False) / float(1 << (l + s))
    yf = lay.plain_eval(xq / float(1 << l), False).astype(np.float64)
    bound = ((lay.t[-1] - lay.t[0]) * 2.0 ** -(s + 1) + np.abs(np.diff(lay.a)).sum() * 2.0 ** -(l + 1)
             + 2.0 ** -(l + s + 1))
    err = np.abs(yq - yf).max()
    print(f"{fn} l={l} s={s}: error {err:.6f} bound {bound:.6f}")
    assert err <= bound


# ---------------------------------------------------------------- 6. host garbler and evaluator
# exact sign: k = 7 and the smallest and largest k of the Leaky host test; the approximate sign needs an MRS base
# (4 <= k <= 11) and is exact on uniform inputs up to k = 9 at accuracy 100: k = 4, 7, 9, the Leaky test's rule
HOST_CASES = [(k, cons) for cons in CONSTRUCTIONS for k in ((4, 7, 9) if cons == "approx" else (2, 7, 12))]


@pytest.mark.parametrize("k,cons", HOST_CASES)
def test_host_garble_evaluate(k, cons):
    N = 60
    name = shape_for(k, "m8")
    c = pwl_circuit((N,), name)
    lay = c.layers[0]
    gc = GarbledCircuit(c, k, _mrs_arg(k), seed=SEED, **CONSTRUCTIONS[cons])
    assert gc.model.layer_params(0)["smode"] == [0 if cons == "approx" else 1]
    for x in pwl_inputs((N,), lay, k):
        want = expected(x, lay.T, lay.A, lay.V)
        np.testing.assert_array_equal(gc.plain_q_eval(x), want)
        np.testing.assert_array_equal(_host_eval(gc, x), want)


@pytest.mark.parametrize("name", ["m1", "m2", "drop"])
@pytest.mark.parametrize("cons", ["approx", "mrs"])
def test_host_shapes_behind_a_rescale(name, cons):
    c = conv_chain(name)
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED, **CONSTRUCTIONS[cons])
    for x in conv_chain_inputs():
        np.testing.assert_array_equal(_host_eval(gc, x), c.plain_q_eval(x, False, M7))


# ---------------------------------------------------------------- 7. wire format
def test_serialize_load_evaluate():
    c = conv_chain("drop")
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED, rescale="mrs", relu="mrs")
    blob = bytes(gc.model.serialize())
    m2 = native().GarbledModel.deserialize(blob)
    assert m2.layer_kind(2) == 21 and native().kind_name(21) == "pwl"
    p = m2.layer_params(2)
    assert (p["s"], p["T"], p["A"], p["V"], p["fn"], p["smode"]) == ([7], [-40, 10, 33], [-30, 100, 100, -256], [1234],
                                                                      [0], [1])
    assert sorted(m2.layer_arrays(2)) == ["b0.mm.e", "b0.mm.g", "b0.mrs", "b1.mm.e", "b1.mm.g", "b1.mrs"]
    assert bytes(m2.serialize()) == blob
    x = conv_chain_inputs()[0]
    enc = gc.garble_inputs(x)
    a, b = gc.cpu_evaluate(enc), native().cpu_evaluate(m2, enc, 0)
    for (pa, la), (pb, lb) in zip(a, b):
        assert pa == pb
        np.testing.assert_array_equal(la, lb)
    np.testing.assert_array_equal(gc.decode_outputs(b), c.plain_q_eval(x, False, M7))


# ---------------------------------------------------------------- 8. / 9. gate ids and table cost from the plan
def test_gate_ids_are_pairwise_distinct():
    """The 2m gadgets of a layer read the same labels, so their pads differ only through the gate id
    stream_id(L, slot, e): the plan's slots are pairwise distinct, fit the 8-bit slot field and stay below the
    ArgMax's 20, hence distinct gate ids for every layer and element."""
    n = native()
    T, A, V, s = SHAPES["m8"]
    slots = n.pwl_plan(first_primes(7), s, T, A, V, 147)["slots"]
    assert slots == [(1 + 2 * i, 2 + 2 * i) for i in range(8)]
    flat = [v for pair in slots for v in pair]
    assert len(set(flat)) == 16 and max(flat) < 20 and max(flat) < 256
    for L in (1, 2, 977):
        for e in (0, 1, 271, (1 << 32) - 1):
            ids = [n.stream_id(L, v, e) for v in flat]
            assert len(set(ids)) == 16
            assert all(i == (L << 44) ^ (v << 36) ^ e for i, v in zip(ids, flat))
    # another layer's or another element's gates never collide with them either
    assert len({n.stream_id(L, v, e) for L in (1, 2) for v in flat for e in (0, 1)}) == 64


@pytest.mark.parametrize("cons", ["approx", "mrs"])
@pytest.mark.parametrize("name,m", [("m1", 1), ("m2", 2), ("m8", 8), ("drop", 2)])
def test_table_cost(name, m, cons):
    """m (n_sign + P + 3k) entries per element: m times a ReLU's tables of the same sign construction; 226 m at
    k = 7 with the exact sign."""
    N, k = 5, 7
    kw = CONSTRUCTIONS[cons]
    gc = GarbledCircuit(pwl_circuit((N,), name), k, 100.0, seed=SEED, **kw)
    relu = GarbledCircuit(d.Circuit([d.Relu((N,))]), k, 100.0, seed=SEED, **kw)
    assert gc.table_bytes == m * relu.table_bytes
    per_elem = gc.table_bytes // (16 * N)
    P = sum(first_primes(k))
    n_sign = relu.table_bytes // (16 * N) - P - 3 * k
    T, A, V, s = SHAPES[name]
    assert per_elem == native().pwl_plan(first_primes(k), s, T, A, V, n_sign)["entries"] == m * (n_sign + P + 3 * k)
    if cons == "mrs":
        assert n_sign == 147 and per_elem == 226 * m


# ---------------------------------------------------------------- 10. / 11. ONNX
def gate_onnx(tmp_path, act="Sigmoid", attrs=b"", name="gate.onnx"):
    """Conv(2 -> 4, 1x1) = f; Conv(4 -> 4, 4x4 on the 4x4 plane) -> act = g (4, 1, 1); Mul(f, g); Conv(4 -> 2, 1x1)."""
    from dash_amd.ir import onnx as o

    rng = np.random.default_rng(11)
    inits = {"w0": _f32(rng, 4, 2, 1, 1), "b0": _f32(rng, 4), "wg": _f32(rng, 4, 4, 4, 4), "bg": _f32(rng, 4),
             "w2": _f32(rng, 2, 4, 1, 1), "b2": _f32(rng, 2)}
    nodes = [o._node("Conv", ["input", "w0", "b0"], ["f"], "conv0", _conv_attrs(1)),
             o._node("Conv", ["f", "wg", "bg"], ["h"], "convg", _conv_attrs(4)),
             o._node(act, ["h"], ["g"], "gate", attrs),
             o._node("Mul", ["f", "g"], ["m"], "mul"),
             o._node("Conv", ["m", "w2", "b2"], ["y"], "conv2", _conv_attrs(1))]
    return _onnx_model(tmp_path / name, nodes, inits, (1, 2, 4, 4), "y", (1, 2, 4, 4))


def test_scale_rule_through_the_gate(tmp_path):
    """conv -> Rescale -> sigmoid -> Mul (channel gate) -> conv: the sigmoid's e = s leaves at the Mul's
    Rescale(l + s); the garbled result equals the plaintext quantized model, which tracks the float network."""
    from dash_amd.ir.onnx import load_onnx_model

    l, s = 4, 6  # l + s <= 10: the mixed-radix rescale's power-of-two label modulus 2^(l + s + 1) must stay below 4096
    c = load_onnx_model(gate_onnx(tmp_path), Q.ScaleQuant, l, pwl_bits=s)
    assert [x.name for x in c.layers] == ["conv2d", "rescale", "conv2d", "rescale", "pwl", "mul", "rescale", "conv2d",
                                          "rescale"]
    assert [x.l for x in c.layers if x.name == "rescale"] == [l, l, l + s, l]
    pw = c.layers[4]
    assert (pw.fn, pw.slope_bits, pw.q_parameter, pw.in_dims) == ("sigmoid", s, l, (4, 1, 1))
    assert c.layers[7].in_scale_bits == 0
    rng = np.random.default_rng(3)
    xf = rng.uniform(-1, 1, 32).astype(np.float32)
    xs = [np.round(xf * (1 << l)).astype(np.int64), np.round(-xf * (1 << l)).astype(np.int64)]
    k = c.infer_crt_base_size(xs)
    M = crt_modulus(first_primes(k))
    gc = GarbledCircuit(c, k, _mrs_arg(k), seed=SEED, rescale="mrs", relu="mrs")
    for x in xs:
        np.testing.assert_array_equal(_host_eval(gc, x), c.plain_q_eval(x, False, M))
    np.testing.assert_allclose(c.plain_q_eval(xs[0], False) / float(1 << l), c.plain_eval(xf, False), atol=0.2)


def test_onnx_import_forms(tmp_path):
    from dash_amd.ir import onnx as o
    from dash_amd.ir.onnx import load_onnx_model

    c = load_onnx_model(gate_onnx(tmp_path), Q.ScaleQuant, 5)
    assert c.layers[4].fn == "sigmoid" and c.layers[4].slope_bits == 8 and c.layers[6].l == 13
    hs = load_onnx_model(gate_onnx(tmp_path, "HardSigmoid", name="hs.onnx"), Q.ScaleQuant, 5).layers[4]
    assert hs.fn == "hard_sigmoid" and hs.fn_params == {"alpha": 0.2, "beta": 0.5} and hs.T.tolist() == [-80, 80]
    attrs = o._attr_float("alpha", 0.25) + o._attr_float("beta", 0.25)
    hs = load_onnx_model(gate_onnx(tmp_path, "HardSigmoid", attrs, "hs2.onnx"), Q.ScaleQuant, 5).layers[4]
    assert hs.T.tolist() == [-32, 96] and hs.A.tolist() == [0, 64, 0]
    # Tanh: today's Sign by default, byte for byte; the layer only with tanh="pwl"
    path = gate_onnx(tmp_path, "Tanh", name="tanh.onnx")
    sign = load_onnx_model(path, Q.ScaleQuant, 5)
    assert [x.name for x in sign.layers][4] == "sign" and sign.layers[6].l == 5
    assert sign.garble_specs()[4] == (3, {}) == load_onnx_model(path, Q.ScaleQuant, 5, tanh="sign").garble_specs()[4]
    tl = load_onnx_model(path, Q.ScaleQuant, 5, tanh="pwl", pwl_bits=4)
    assert tl.layers[4].fn == "tanh" and tl.layers[4].slope_bits == 4 and tl.layers[6].l == 9
    with pytest.raises(ValueError, match="tanh must be"):
        load_onnx_model(path, Q.ScaleQuant, 5, tanh="spline")
    for qm, qp in ((Q.SimpleQuant, -1), (Q.ScaleQuantPlus, 32)):
        with pytest.raises(ValueError, match="gate.*ScaleQuant"):
            load_onnx_model(gate_onnx(tmp_path), qm, qp)


def test_onnx_refuses_pending_scale_and_factor(tmp_path):
    from dash_amd.ir import onnx as o
    from dash_amd.ir.onnx import load_onnx_model

    rng = np.random.default_rng(5)
    inits = {"w0": _f32(rng, 4, 2, 1, 1), "b0": _f32(rng, 4)}
    conv = o._node("Conv", ["input", "w0", "b0"], ["f"], "conv0", _conv_attrs(1))

    def model(mid, name):
        nodes = [conv, mid, o._node("Sigmoid", ["a"], ["y"], "gate")]
        return _onnx_model(tmp_path / name, nodes, inits, (1, 2, 4, 4), "y", (1, 4, 4, 4))

    leaky = o._node("LeakyRelu", ["f"], ["a"], "act", o._attr_float("alpha", 0.25))
    with pytest.raises(NotImplementedError, match=r"gate: a pending 2\^4 scale reaches this Sigmoid"):
        load_onnx_model(model(leaky, "bits.onnx"), Q.ScaleQuant, 5)
    sig = o._node("Sigmoid", ["f"], ["a"], "first")
    with pytest.raises(NotImplementedError, match=r"gate: a pending 2\^8 scale reaches this Sigmoid"):
        load_onnx_model(model(sig, "twice.onnx"), Q.ScaleQuant, 5)
    gap = o._node("GlobalAveragePool", ["f"], ["a"], "gap")
    with pytest.raises(NotImplementedError, match="gate: an average's 1/K factor reaches this Sigmoid"):
        load_onnx_model(model(gap, "fac.onnx"), Q.ScaleQuant, 5)
    # a graph output with the layer's pending bits is refused as a LeakyRelu's is
    nodes = [conv, o._node("Sigmoid", ["f"], ["y"], "gate")]
    with pytest.raises(NotImplementedError, match="graph output 'y'"):
        load_onnx_model(_onnx_model(tmp_path / "out.onnx", nodes, inits, (1, 2, 4, 4), "y", (1, 4, 4, 4)), Q.ScaleQuant, 5)


@pytest.mark.parametrize("act", ["Sigmoid", "Tanh", "HardSigmoid"])
def test_onnx_export_round_trip(tmp_path, act):
    from dash_amd.ir import onnx as o
    from dash_amd.ir.onnx import load_onnx_model, save_onnx_model

    attrs = o._attr_float("alpha", 0.25) + o._attr_float("beta", 0.375) if act == "HardSigmoid" else b""
    kw = dict(tanh="pwl", pwl_bits=6)
    c = load_onnx_model(gate_onnx(tmp_path, act, attrs), Q.ScaleQuant, 5, **kw)
    save_onnx_model(tmp_path / "out.onnx", c)
    assert [n["op_type"] for n in o.parse_onnx(tmp_path / "out.onnx")["nodes"]] == ["Conv", "Conv", act, "Mul", "Conv"]
    c2 = load_onnx_model(tmp_path / "out.onnx", Q.ScaleQuant, 5, **kw)
    assert len(c2.layers) == len(c.layers)
    for a, b in zip(c.garble_specs(), c2.garble_specs()):
        assert a[0] == b[0] and sorted(a[1]) == sorted(b[1])
        for key in a[1]:
            np.testing.assert_array_equal(np.asarray(a[1][key]), np.asarray(b[1][key]))
    with pytest.raises(NotImplementedError, match="untagged piecewise-linear"):
        save_onnx_model(tmp_path / "raw.onnx", pwl_circuit((4,), "m2"))


# ---------------------------------------------------------------- 12. range guard
def test_range_guard_refuses_sign_inputs_outside_the_range():
    """The domain is every x - T_i in [-M/2, M/2): with T = (-50, 70) an input above M/2 - 1 - 50 or below
    -M/2 + 70 is refused on the numpy and on the torch path, the ends themselves pass."""
    c = pwl_circuit((4,), "m2")
    g = RangeGuard(c, M7)
    assert g.batched and not g.native_forms
    h = M7 // 2
    top, bot = (M7 - h) - 1 - 50, -h + 70
    xs = [np.array([top, bot, 0, -1]), np.array([top + 1, 0, 1, 2]), np.array([3, bot - 1, 1, 2]),
          np.array([-50, 70, 69, -51])]
    want = [False, True, True, False]
    assert [bool(g.violations_np(x)) for x in xs] == want
    assert g.submit(xs).bad_indices() == [i for i, w in enumerate(want) if w]
    lay = c.layers[0]
    np.testing.assert_array_equal(g.outputs(xs[3:])[0], expected(xs[3], lay.T, lay.A, lay.V))
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED)
    assert gc.guard_enabled
    with pytest.raises(Exception):
        gc.check_inputs([xs[1]])
    gc.check_inputs([xs[0], xs[3]])


# ---------------------------------------------------------------- 13. zoo
@pytest.mark.parametrize("name,kinds", [("LENET5_TANH_MNIST", ("tanh", 4)), ("SE_SIGMOID_CIFAR", ("sigmoid", 2))])
def test_zoo_models(name, kinds):
    from dash_amd.models import zoo

    l, s = 5, 4
    c = zoo.build_circuit(name, Q.ScaleQuant, l, seed=2, pwl_bits=s)
    pw = [x for x in c.layers if x.name == "pwl"]
    assert len(pw) == kinds[1] and all(x.fn == kinds[0] and x.slope_bits == s for x in pw)
    if name == "SE_SIGMOID_CIFAR":  # the gate's 2^s leaves with the Mul's rescale
        assert [c.layers[i + 1].l for i, x in enumerate(c.layers) if x.name == "mul"] == [l + s, l + s]
    else:  # every linear layer behind a tanh absorbs it
        assert [x.l for x in c.layers if x.name == "rescale"] == [l, l + s, l + s, l + s, l + s]
    xs = zoo.quantized_inputs(name, 2, Q.ScaleQuant, l, seed=5)
    k = c.infer_crt_base_size(xs)
    M = crt_modulus(first_primes(k))
    c.calibrate(xs, M)
    assert c.required_crt_modulus() <= M
    gc = GarbledCircuit(c, k, _mrs_arg(k), seed=SEED, rescale="mrs", relu="mrs")
    for x in xs:
        np.testing.assert_array_equal(_host_eval(gc, x), c.plain_q_eval(x, False, M))
    for qm, qp in ((Q.SimpleQuant, -1), (Q.ScaleQuantPlus, 32)):
        with pytest.raises(ValueError, match="ScaleQuant only"):
            zoo.build_circuit(name, qm, qp)


def test_zoo_se_default_gate_is_unchanged():
    from dash_amd.models import zoo

    c = zoo.build_circuit("SE_MOBILENET_CIFAR", Q.ScaleQuant, 5, seed=2)
    assert not any(x.name == "pwl" for x in c.layers) and sum(x.name == "mul" for x in c.layers) == 3
    assert all(c.layers[i + 1].l == 5 for i, x in enumerate(c.layers) if x.name == "mul")


def test_trainer_maps_sigmoid_and_keeps_tanh():
    torch = pytest.importorskip("torch")
    from dash_amd.models import train as tr

    nn = torch.nn
    for mod, fn in ((nn.Sigmoid(), "sigmoid"), (nn.Hardsigmoid(), "hard_sigmoid")):
        m = nn.Sequential(nn.Flatten(), nn.Linear(784, 6), mod, nn.Linear(6, 3))
        c = tr.to_circuit(m, "MODEL_A", Q.ScaleQuant, 5, pwl_bits=6)
        assert [x.name for x in c.layers] == ["flatten", "dense", "rescale", "pwl", "dense", "rescale"]
        assert c.layers[3].fn == fn and c.layers[4].in_scale_bits == 6 and c.layers[5].l == 11
    m = nn.Sequential(nn.Flatten(), nn.Linear(784, 6), nn.Tanh(), nn.Linear(6, 3))
    assert [x.name for x in tr.to_circuit(m, "MODEL_A", Q.ScaleQuant, 5).layers][3] == "sign"


def test_config_and_cli_options():
    import argparse

    from dash_amd.config import DashConfig

    assert (DashConfig().pwl_bits, DashConfig().tanh) == (8, "sign")
    ap = argparse.ArgumentParser()
    DashConfig.add_arguments(ap)
    cfg = DashConfig.from_args(ap.parse_args(["--pwl-bits", "6", "--tanh", "pwl"]))
    assert (cfg.pwl_bits, cfg.tanh) == (6, "pwl")


# ---------------------------------------------------------------- 14. the kernel's digit formula
def _shipped_primes():
    return sorted({p for k in range(2, 13) for p in first_primes(k)})


@pytest.mark.parametrize("p", [p for p in _shipped_primes() if p > 2])
def test_modq_range_of_the_pwl_digit(p):
    """gadget_walks.h pwl_digit with dev.h modq's arithmetic (reciprocal floor(2^32 / p), one correction).
    (a) modq is exact on the whole range the accumulator can reach with m <= 8: [0, (p - 1)^2 + 8 (p - 1)(2p - 1)],
    which contains the 9 (p - 1)^2 of reduced ReLU digits; every value is tried. (b) One breakpoint's term for ALL
    operand values: with u = ev + p - g in [1, 2p - 1], modq(yl x + d u) with yl = modq(a0 + d ypr) equals
    (a0 x + d t) mod p, t = (ev + ypr x - g) mod p. (c) Eight terms at the operands' extremes and at random."""
    P = np.uint64(p)
    top = (p - 1) ** 2 + 8 * (p - 1) * (2 * p - 1)
    assert 9 * (p - 1) ** 2 <= top < 1 << 32 and (p != 37 or top == 22320)
    allv = np.arange(top + 1, dtype=np.uint64)
    np.testing.assert_array_equal(modq(allv, p), allv % P)
    r = np.arange(p, dtype=np.uint64)
    dd, ypr, x, u = np.meshgrid(r, r, r, np.arange(1, 2 * p, dtype=np.uint64), indexing="ij", sparse=True)
    t = (u + ypr * x) % P
    for a0 in range(p):
        pre = np.uint64(a0) + dd * ypr
        yl = modq(pre, p)
        np.testing.assert_array_equal(yl, pre % P)
        arg = yl * x + dd * u
        assert int(arg.max()) <= (p - 1) ** 2 + (p - 1) * (2 * p - 1)
        got = modq(arg, p)
        np.testing.assert_array_equal(got, np.broadcast_to((np.uint64(a0) * x + dd * t) % P, got.shape))
    rng = np.random.default_rng(p)
    for trial in range(200):
        ext = trial < 2
        m = 8 if ext else int(rng.integers(1, 9))
        pick = (lambda hi: np.full(m, hi - 1, dtype=np.uint64)) if ext else (lambda hi: rng.integers(0, hi, m).astype(np.uint64))
        dv, yv, ev = pick(p), pick(p), pick(p)
        gv = np.zeros(m, dtype=np.uint64) if ext else pick(p)
        a0 = np.uint64(p - 1 if ext else rng.integers(0, p))
        xv = np.uint64(p - 1 if ext else rng.integers(0, p))
        yl = modq(a0 + (dv * yv).sum(), p)
        acc = yl * xv + (dv * (ev + P - gv)).sum()
        assert int(acc) <= top
        tv = (ev + yv * xv + P - gv) % P
        assert int(modq(acc, p)) == int((a0 * xv + (dv * tv).sum()) % P)


def test_p2_bit_logic_of_the_pwl_digit():
    """p = 2: out = (a0 & x) ^ XOR_i (d_i & t_i), t_i = e_i ^ g_i ^ (ypr_i & x), equals W ^ (yl & x) with
    W = XOR_i (d_i & (e_i ^ g_i)) and yl = (a0 + sum_i d_i ypr_i) mod 2, for every operand combination of two
    breakpoints."""
    import itertools

    for a0, x, d0, d1, b0, b1, y0, y1 in itertools.product((0, 1), repeat=8):
        t0, t1 = b0 ^ (y0 & x), b1 ^ (y1 & x)
        W = (d0 & b0) ^ (d1 & b1)
        yl = (a0 + d0 * y0 + d1 * y1) % 2
        assert W ^ (yl & x) == (a0 * x + d0 * t0 + d1 * t1) % 2
