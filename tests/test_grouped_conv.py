"""Grouped and depthwise convolution (Conv2d(groups=g)) on the host: plaintext IR, garbling and the host
evaluator, serialization, ONNX import / export, the range guard and the torch-to-circuit conversion.

Group q holds filters [q*F/g, (q+1)*F/g) and reads channels [q*C/g, (q+1)*C/g); weights are [F][C/g][kh][kw].
The zero-expanded block-diagonal dense Conv2d computes the same values (it is not wire-equivalent: every
expanded zero weight adds a Z_p term), so it serves as a plaintext oracle only.
"""
from __future__ import annotations

import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit, RangeGuard
from dash_amd.ir.bases import crt_modulus, first_primes
from dash_amd.native import native

CASES = [(4, 4, 4), (4, 8, 4), (6, 4, 2), (8, 12, 2)]  # (C, F, g)
VARIANTS = [(1, 0), (2, 0), (1, 1), (2, 1)]  # (stride, pad)
H, W, KS = 7, 9, 3


def _weights(rng, C, F, g, k=KS):
    """Weights with zeros and multiples of 2, 3 and 5 (zero mod a CRT prime: the Z_p quirk)."""
    w = rng.integers(-6, 7, (F, C // g, k, k))
    flat = w.reshape(-1)
    flat[::5] = 0
    flat[1::7] = 2 * 3 * 5
    flat[2::11] = -6
    flat[3::13] = 10
    return w, rng.integers(-9, 10, F)


def _grouped(w, b, C, F, g, s=1, p=0, h=H, wd=W):
    k = w.shape[-1]
    return d.Conv2d.from_quantized(w, b, wd, h, C, F, k, k, s, s, pad_width=p, pad_height=p, groups=g)


def _expanded(w, b, C, F, g, s=1, p=0, h=H, wd=W):
    """The same layer as a dense conv with block-diagonal zero-expanded weights."""
    k = w.shape[-1]
    Cg, Fg = C // g, F // g
    we = np.zeros((F, C, k, k), dtype=np.int64)
    for f in range(F):
        q = f // Fg
        we[f, q * Cg:(q + 1) * Cg] = w[f]
    return d.Conv2d.from_quantized(we, b, wd, h, C, F, k, k, s, s, pad_width=p, pad_height=p)


def _six_loops(x, w, b, C, F, g, s, p, h=H, wd=W):
    k = w.shape[-1]
    Cg, Fg = C // g, F // g
    OH, OW = (h + 2 * p - k) // s + 1, (wd + 2 * p - k) // s + 1
    x = np.asarray(x, dtype=np.int64).reshape(C, h, wd)
    y = np.zeros((F, OH, OW), dtype=np.int64)
    for f in range(F):
        for oy in range(OH):
            for ox in range(OW):
                acc = int(b[f])
                for c in range(Cg):
                    for dy in range(k):
                        for dx in range(k):
                            iy, ix = oy * s - p + dy, ox * s - p + dx
                            if 0 <= iy < h and 0 <= ix < wd:
                                acc += int(w[f, c, dy, dx]) * int(x[(f // Fg) * Cg + c, iy, ix])
                y[f, oy, ox] = acc
    return y.reshape(-1)


@pytest.mark.parametrize("s,p", VARIANTS)
@pytest.mark.parametrize("C,F,g", CASES)
def test_plain_q_eval_against_both_oracles(C, F, g, s, p):
    rng = np.random.default_rng(C * 100 + F * 10 + g + s + 3 * p)
    w, b = _weights(rng, C, F, g)
    x = rng.integers(-20, 21, C * H * W)
    grp, exp = _grouped(w, b, C, F, g, s, p), _expanded(w, b, C, F, g, s, p)
    assert grp.groups == g and grp.q_weights.shape == (F, C // g, KS, KS)
    y = grp.plain_q_eval(x)
    np.testing.assert_array_equal(y, _six_loops(x, w, b, C, F, g, s, p))
    np.testing.assert_array_equal(y, exp.plain_q_eval(x))
    # the float evaluation takes the same per-group path
    np.testing.assert_allclose(grp.plain_eval(x.astype(np.float32)), y.astype(np.float32), rtol=0, atol=1e-2)
    # range tracking runs over the group's own C/g*kh*kw terms: never more CRT primes than the expanded layer
    kg = d.Circuit([grp]).infer_crt_base_size([x])
    ke = d.Circuit([exp]).infer_crt_base_size([x])
    assert kg <= ke
    assert grp.min_q >= exp.min_q and grp.max_q <= exp.max_q


def test_bad_groups_raise():
    w, b = np.zeros((4, 1, 3, 3)), np.zeros(4)
    for g in (0, 3, 8):
        with pytest.raises(ValueError):
            d.Conv2d.from_quantized(w, b, W, H, 4, 4, 3, 3, groups=g)
        with pytest.raises(ValueError):
            d.Conv2d(w, b, W, H, 4, 4, 3, 3, groups=g)
    with pytest.raises(ValueError):  # groups divides C but not F
        d.Conv2d.from_quantized(np.zeros((6, 1, 3, 3)), np.zeros(6), W, H, 4, 6, 3, 3, groups=4)


@pytest.mark.parametrize("hardened", [True, False], ids=["hardened", "reference"])
@pytest.mark.parametrize("C,F,g,s,p", [(4, 4, 4, 1, 1), (4, 8, 4, 2, 1), (6, 4, 2, 1, 0), (8, 12, 2, 2, 1)])
def test_garble_cpu_evaluate_decode(C, F, g, s, p, hardened):
    rng = np.random.default_rng(C + F + g)
    w, b = _weights(rng, C, F, g)
    c = d.Circuit([_grouped(w, b, C, F, g, s, p)])
    gc = GarbledCircuit(c, 7, None, seed=bytes(range(16)), hardened=hardened)
    for i in range(2):
        x = rng.integers(-20, 21, C * H * W)
        y = gc.decode_outputs(gc.cpu_evaluate(gc.garble_inputs(x)))
        np.testing.assert_array_equal(y, gc.plain_q_eval(x))
        np.testing.assert_array_equal(y, _six_loops(x, w, b, C, F, g, s, p))


def test_serialize_roundtrip_and_wire_param():
    rng = np.random.default_rng(5)
    w, b = _weights(rng, 6, 6, 3)
    grp = _grouped(w, b, 6, 6, 3, 1, 1)
    kind, spec = grp.garble_spec()
    assert spec["g"] == 3
    wd, bd = _weights(rng, 6, 6, 1)
    _, dense_spec = _grouped(wd, bd, 6, 6, 1, 1, 1).garble_spec()
    assert "g" not in dense_spec  # groups == 1 keeps the dense wire bytes
    c = d.Circuit([grp, d.Relu(grp.out_dims)])
    gc = GarbledCircuit(c, 7, 100.0, seed=b"g" * 16)
    blob = gc.model.serialize()
    m2 = native().GarbledModel.deserialize(blob)
    assert m2.serialize() == blob
    x = rng.integers(-20, 21, c.input_size)
    enc = gc.garble_inputs(x)
    a, b2 = gc.cpu_evaluate(enc), native().cpu_evaluate(m2, enc, 0)
    for (p1, x1), (p2, x2) in zip(a, b2):
        assert p1 == p2
        np.testing.assert_array_equal(x1, x2)
    np.testing.assert_array_equal(gc.decode_outputs(b2), gc.plain_q_eval(x))


def _dwsep_circuit(rng, q_const=1.0):
    """dense 3x3 stem, depthwise 3x3 (stride 2), 1x1: float weights on an integer grid."""
    from dash_amd.ir.quant import QuantizationMethod as Q

    def conv(F, C, k, g, h, wd, s, p):
        wt = rng.integers(-4, 5, (F, C // g, k, k)).astype(np.float32)
        bs = rng.integers(-4, 5, F).astype(np.float32)
        return d.Conv2d(wt, bs, wd, h, C, F, k, k, s, s, -1, Q.SimpleQuant, q_const, pad_width=p, pad_height=p,
                        groups=g)

    l0 = conv(4, 2, 3, 1, 8, 8, 1, 1)
    l1 = conv(8, 4, 3, 4, 8, 8, 2, 1)  # depthwise, channel multiplier 2
    l2 = conv(6, 8, 1, 2, 4, 4, 1, 0)  # grouped 1x1
    return d.Circuit([l0, d.Relu(l0.out_dims), l1, d.Relu(l1.out_dims), l2])


def test_onnx_roundtrip(tmp_path):
    from dash_amd.ir.onnx import load_onnx_model, save_onnx_model
    from dash_amd.ir.quant import QuantizationMethod as Q

    rng = np.random.default_rng(8)
    c = _dwsep_circuit(rng)
    p = tmp_path / "dw.onnx"
    save_onnx_model(p, c)
    c2 = load_onnx_model(p, Q.SimpleQuant, -1, 1.0)
    convs = [l for l in c.layers if isinstance(l, d.Conv2d)]
    convs2 = [l for l in c2.layers if isinstance(l, d.Conv2d)]
    assert [l.groups for l in convs2] == [1, 4, 2]
    for a, b in zip(convs, convs2):
        np.testing.assert_array_equal(a.q_weights, b.q_weights)
        np.testing.assert_array_equal(a.q_biases, b.q_biases)
    x = rng.integers(-10, 11, c.input_size)
    np.testing.assert_array_equal(c.plain_q_eval(x), c2.plain_q_eval(x))


def _onnx_conv_bn_relu(path, w, b, group, C, H_, W_, bn):
    """Conv (group) -> BatchNormalization (per filter) -> Relu, written with the exporter's own encoders."""
    from dash_amd.ir import onnx as o

    F = w.shape[0]
    inits = [o._tensor("w", w), o._tensor("b", b)] + [o._tensor(n, v) for n, v in bn.items()]
    attrs = (o._attr_ints("dilations", [1, 1]) + o._attr_int("group", group) + o._attr_ints("kernel_shape", [3, 3])
             + o._attr_ints("pads", [1, 1, 1, 1]) + o._attr_ints("strides", [1, 1]))
    nodes = [o._node("Conv", ["input", "w", "b"], ["t0"], "conv", attrs),
             o._node("BatchNormalization", ["t0", "scale", "shift", "mean", "var"], ["t1"], "bn",
                     o._attr_float("epsilon", 0.0)),
             o._node("Relu", ["t1"], ["t2"], "relu")]
    graph = b"".join(nodes) + o._s(2, "g") + b"".join(o._ld(5, t) for t in inits)
    graph += o._ld(11, o._value_info("input", (1, C, H_, W_)))
    graph += o._ld(12, o._value_info("t2", (1, F, H_, W_)))
    model = o._i(1, 7) + o._s(2, "test") + o._s(3, "1") + o._ld(7, graph) + o._ld(8, o._s(1, "") + o._i(2, 13))
    path.write_bytes(model)


def test_onnx_depthwise_batchnorm_fold_and_bad_group(tmp_path):
    from dash_amd.ir.onnx import load_onnx_model
    from dash_amd.ir.quant import QuantizationMethod as Q

    rng = np.random.default_rng(9)
    C = 4
    w = rng.integers(-3, 4, (C, 1, 3, 3)).astype(np.float32)
    b = rng.integers(-3, 4, C).astype(np.float32)
    # integer-valued fold: scale / sqrt(var) in {1, 2, 3}, integer mean and shift
    bn = {"scale": np.array([2, 3, 4, 6], np.float32), "shift": np.array([1, -2, 0, 5], np.float32),
          "mean": np.array([3, 0, -1, 2], np.float32), "var": np.array([4, 1, 4, 4], np.float32)}
    p = tmp_path / "dwbn.onnx"
    _onnx_conv_bn_relu(p, w, b, C, C, 5, 6, bn)
    c = load_onnx_model(p, Q.SimpleQuant, -1, 1.0)
    conv = c.layers[0]
    assert isinstance(conv, d.Conv2d) and conv.groups == C and conv.q_weights.shape == (C, 1, 3, 3)
    g = bn["scale"] / np.sqrt(bn["var"])
    np.testing.assert_array_equal(conv.q_weights, (w * g[:, None, None, None]).astype(np.int64))
    np.testing.assert_array_equal(conv.q_biases, ((b - bn["mean"]) * g + bn["shift"]).astype(np.int64))
    x = rng.integers(-10, 11, C * 5 * 6)
    ref = _six_loops(x, conv.q_weights, conv.q_biases, C, C, C, 1, 1, h=5, wd=6)
    np.testing.assert_array_equal(c.plain_q_eval(x), np.maximum(ref, 0))
    # a group that does not divide the input channels is refused
    bad = tmp_path / "bad.onnx"
    _onnx_conv_bn_relu(bad, rng.integers(-3, 4, (6, 2, 3, 3)).astype(np.float32), np.zeros(6, np.float32), 3, C, 5, 6,
                       {k: np.ones(6, np.float32) for k in bn})
    with pytest.raises(ValueError, match="group"):
        load_onnx_model(bad, Q.SimpleQuant, -1, 1.0)


K_GUARD = 6
M_GUARD = crt_modulus(first_primes(K_GUARD))


def guard_circuit():
    """Depthwise 3x3 identity (center tap 1) -> Rescale(5) -> ReLU: the rescale sees the plaintext input itself,
    so one element at Rescale.mrs_limit(M) sits on the first value of the wrap band."""
    C, h, wd = 3, 4, 4
    w = np.zeros((C, 1, 3, 3), dtype=np.int64)
    w[:, 0, 1, 1] = 1
    conv = d.Conv2d.from_quantized(w, np.zeros(C, np.int64), wd, h, C, C, 3, 3, pad_width=1, pad_height=1, groups=C)
    c = d.Circuit([conv, d.Rescale(5, conv.out_dims), d.Relu(conv.out_dims)])
    rng = np.random.default_rng(0)
    c.calibrate([rng.integers(-50, 51, size=c.input_size) for _ in range(8)], M_GUARD)
    return c


def guard_inputs(c):
    """In-range inputs, the last in-range value, and one input pushed into the band (index 3)."""
    lim = c.layers[1].mrs_limit(M_GUARD)
    assert lim < M_GUARD // 2
    rng = np.random.default_rng(1)
    xs = [rng.integers(-50, 51, size=c.input_size) for _ in range(3)]
    band, ok = xs[0].copy(), xs[1].copy()
    band[17] = lim
    ok[17] = lim - 1
    return xs + [band, ok]


def test_range_guard_depthwise_torch_matches_numpy():
    c = guard_circuit()
    xs = guard_inputs(c)
    g = RangeGuard(c, M_GUARD, mrs=True)
    assert g.batched
    ref = [i for i, x in enumerate(xs) if g.violations_np(x)]
    assert ref == [3]
    assert sorted(g.submit(xs).bad_indices()) == ref
    # the native description carries the group count
    assert g.native_spec()["layers"][0]["g"] == 3
    # a grouped layer with more than one channel per group through the torch path: same outputs as numpy
    rng = np.random.default_rng(2)
    w, b = _weights(rng, 6, 4, 2)
    c2 = d.Circuit([_grouped(w, b, 6, 4, 2, 2, 1)])
    x2 = [rng.integers(-20, 21, c2.input_size) for _ in range(3)]
    c2.calibrate(x2, M_GUARD)
    import torch

    bad, out = RangeGuard(c2, M_GUARD, mrs=True)._bad_batch(torch.tensor(np.stack(x2)), want_out=True)
    assert not bool(bad.any())
    np.testing.assert_array_equal(out.cpu().numpy(), np.stack([c2.plain_q_eval(x, track=False) for x in x2]))
    assert RangeGuard(c2, M_GUARD, mrs=True).submit(x2).bad_indices() == []


def test_torch_module_with_groups_to_circuit():
    torch = pytest.importorskip("torch")
    from dash_amd.ir.quant import QuantizationMethod as Q
    from dash_amd.models.train import build_torch_model, to_circuit

    torch.manual_seed(0)
    nn = torch.nn
    model = nn.Sequential(nn.Conv2d(3, 6, 3, padding=1, groups=3), nn.ReLU(),
                          nn.Conv2d(6, 6, 3, stride=2, padding=1, groups=6), nn.ReLU(), nn.Flatten(),
                          nn.Linear(6 * 16 * 16, 5))
    c = to_circuit(model, "MODEL_DWSEP_CIFAR", Q.ScaleQuant, 4)
    convs = [l for l in c.layers if isinstance(l, d.Conv2d)]
    assert [l.groups for l in convs] == [3, 6]
    x = np.random.default_rng(3).standard_normal((1, 3, 32, 32)).astype(np.float32)
    with torch.no_grad():
        ref = model(torch.from_numpy(x)).numpy()[0]
    np.testing.assert_allclose(c.plain_eval(x.reshape(-1)), ref, rtol=1e-4, atol=1e-4)
    # the zoo's depthwise-separable model builds the same way: every dwconv op becomes groups == channels
    tm = build_torch_model("MODEL_DWSEP_CIFAR")
    tm.fq.c = 0.0
    dw = [m for m in tm if isinstance(m, nn.Conv2d) and m.groups > 1]
    assert len(dw) == 3 and all(m.groups == m.in_channels == m.out_channels for m in dw)
    cz = to_circuit(tm, "MODEL_DWSEP_CIFAR", Q.ScaleQuant, 5)
    with torch.no_grad():
        refz = tm(torch.from_numpy(x)).numpy()[0]
    # the circuit's sumpool is the module's average pool times 16 (a sum), ahead of a linear layer
    fc = [m for m in tm if isinstance(m, nn.Linear)][0]
    scaled = refz - fc.bias.detach().numpy()
    np.testing.assert_allclose(cz.plain_eval(x.reshape(-1)) - fc.bias.detach().numpy(), 16 * scaled, rtol=1e-3,
                               atol=1e-3)


def test_zoo_model_builds_and_matches_plain():
    from dash_amd.ir.quant import QuantizationMethod as Q
    from dash_amd.models import BENCH_CONFIGS, build_circuit, quantized_inputs

    cfg = BENCH_CONFIGS["MODEL_DWSEP_CIFAR/DASH"]
    c = build_circuit(cfg["model"], Q(cfg["q_method"]), cfg["q_parameter"], seed=0)
    dw = [l for l in c.layers if isinstance(l, d.Conv2d) and l.groups > 1]
    assert len(dw) == 3 and all(l.groups == l.C == l.F for l in dw)
    assert [l.sh for l in dw] == [2, 2, 1]
    x = quantized_inputs(cfg["model"], 1, Q(cfg["q_method"]), cfg["q_parameter"], seed=1)[0]
    assert c.infer_crt_base_size([x]) <= cfg["crt"]
    assert c.plain_q_eval(x).shape == (10,)
