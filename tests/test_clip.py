"""The Clip layer (ONNX Clip, ReLU6, Hardtanh) on the host: semantics, the garbled construction of
csrc/gadgets.h ClipPlan through the host garbler and evaluator, refusals, the wire format, ONNX import and
export, the range guard and the MobileNet-style zoo model (docs/CLIP.md).

The helpers below (inputs, the cut-down MobileNet) are shared with tests/test_gpu_clip.py.
"""
from __future__ import annotations

import hashlib

import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit, RangeGuard, RangeGuardError
from dash_amd.ir.bases import crt_modulus, first_primes
from dash_amd.ir.quant import QuantizationMethod as Q

M7 = crt_modulus(first_primes(7))
SEED = bytes(range(16))
BOUNDARY_AT = (0, 15, 16, 63, 64, 255, 256, 511, 512, -1)


# ---------------------------------------------------------------- shared helpers
def clip_values(lo: int, hi: int, M: int) -> list:
    """Every value in [lo - 3, hi + 3] and both ends of the domain [-M/2 + hi, M/2 + lo) on which both sign
    inputs x - lo and x - hi are signed CRT values."""
    return list(range(lo - 3, hi + 4)) + [-(M // 2) + hi, M - M // 2 + lo - 1]


def clip_inputs(N: int, lo: int, hi: int, M: int, seed: int = 1, max_rounds: int = 0) -> list:
    """An even number of input vectors of N values that together hold clip_values() (the six values around the
    bounds first), filled up with random values of the domain. In the first vector the values around the bounds
    also sit on the element indices BOUNDARY_AT, where they exist. max_rounds > 0 caps the number of vectors."""
    rng = np.random.default_rng(seed)
    edge = [lo - 1, lo, lo + 1, hi - 1, hi, hi + 1]
    queue = edge + [v for v in clip_values(lo, hi, M) if v not in edge]
    dom_lo, dom_hi = -(M // 2) + hi, M - M // 2 + lo
    pinned = {i % N: edge[n % len(edge)] for n, i in enumerate(BOUNDARY_AT) if -N <= i < N} if N > 1 else {}
    out = []
    while queue or len(out) % 2:
        x = rng.integers(dom_lo, dom_hi, N)
        for i in range(N):
            if not out and i in pinned:
                x[i] = pinned[i]
            elif queue:
                x[i] = queue.pop(0)
        out.append(x)
        if max_rounds and len(out) == max_rounds:
            break
    return out


TINY_MOBILENET = {"input": (3, 8, 8), "ops": [
    ("conv", 4, 3, 1, 1), ("relu6",), ("dwconv", 3, 2, 1), ("relu6",), ("conv", 8, 1, 1, 0), ("relu6",),
    ("dwconv", 3, 1, 1), ("clip", -0.25, 0.25), ("conv", 8, 1, 1, 0), ("relu6",), ("gap",), ("flatten",), ("fc", 10)]}


def tiny_mobilenet(n_inputs: int = 2):
    """MOBILENET_CIFAR's ops (dense stem, depthwise / pointwise blocks, ReLU6, global-average head) on 3x8x8,
    ScaleQuant l = 5, calibrated. The synthetic inputs are scaled up so that the inputs of the narrow Clip
    pass both of its bounds."""
    from dash_amd.models import zoo

    zoo.ARCHS["_TINY_MOBILENET"] = TINY_MOBILENET
    try:
        c = zoo.build_circuit("_TINY_MOBILENET", Q.ScaleQuant, 5, seed=2)
        xs = [4 * x for x in zoo.quantized_inputs("_TINY_MOBILENET", n_inputs, Q.ScaleQuant, 5, seed=5)]
    finally:
        del zoo.ARCHS["_TINY_MOBILENET"]
    k = c.infer_crt_base_size(xs)
    c.calibrate(xs, crt_modulus(first_primes(max(k, 7))))
    return c, xs, k


def _host_eval(gc, x):
    return gc.decode_outputs(gc.cpu_evaluate(gc.garble_inputs(x)))


# ---------------------------------------------------------------- 1. semantics
@pytest.mark.parametrize("lo,hi", [(0.0, 6.0), (-1.0, 1.0), (-1000.0, 3000.0)])
def test_semantics(lo, hi):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(0)
    c = d.Clip((4, 5, 5), lo, hi, 5, Q.ScaleQuant)
    assert (c.kind, c.name, d.Clip.kind) == (15, "clip", 15)
    assert (c.q_lo, c.q_hi) == (int(lo * 32), int(hi * 32)) and c.q_lo < c.q_hi
    x = (rng.standard_normal(100) * max(abs(lo), abs(hi)) * 2).astype(np.float32)
    np.testing.assert_array_equal(c.plain_eval(x, track=False), torch.clamp(torch.tensor(x), lo, hi).numpy())
    xq = rng.integers(c.q_lo - 50, c.q_hi + 50, 100)
    xq[:4] = [c.q_lo, c.q_hi, c.q_lo - 1, c.q_hi + 1]
    np.testing.assert_array_equal(c.plain_q_eval(xq, track=False), np.clip(xq, c.q_lo, c.q_hi))
    assert c.garble_spec() == (15, {"lo": c.q_lo, "hi": c.q_hi})
    # ScaleQuantPlus: the activation scale is s
    assert d.Clip((3,), lo, hi, 32, Q.ScaleQuantPlus).q_hi == int(hi * 32)


def test_bounds_and_scheme_refusals():
    for lo, hi in ((1.0, 1.0), (2.0, -2.0), (0.0, float("inf")), (float("nan"), 1.0)):
        with pytest.raises(ValueError, match="clip"):
            d.Clip((3,), lo, hi)
    with pytest.raises(ValueError, match="q_lo < q_hi"):
        d.Clip.from_quantized((3,), 5, 5)
    with pytest.raises(ValueError, match="q_lo < q_hi"):
        d.Clip((3,), 0.001, 0.002, 5, Q.ScaleQuant)  # both bounds round to 0
    with pytest.raises(ValueError, match="clip.*SimpleQuant"):
        d.Clip((3,), 0.0, 6.0, -1, Q.SimpleQuant)
    from dash_amd.models import build_circuit

    with pytest.raises(ValueError, match="relu6.*SimpleQuant"):
        build_circuit("MOBILENET_CIFAR", Q.SimpleQuant, -1)


def test_range_tracking_sizes_both_sign_inputs():
    c = d.Clip.from_quantized((4,), -37, 41)
    c.plain_q_eval(np.array([-100, 0, 50, 90]))
    assert c.get_min_plain_q_val() == -100 - 41 and c.get_max_plain_q_val() == 90 + 37
    c.quantize(0.5)  # SimpleQuant re-quantization only resets the ranges
    assert (c.q_lo, c.q_hi) == (-37, 41) and c.max_q < c.min_q
    k = d.Circuit([d.Clip.from_quantized((1,), 0, 192)]).infer_crt_base_size([np.array([14000])])
    assert crt_modulus(first_primes(k)) // 2 > 14000 and crt_modulus(first_primes(k - 1)) // 2 <= 14000


# ---------------------------------------------------------------- 2. garbled end to end on the host
@pytest.mark.parametrize("relu", ["approx", "mrs"])
@pytest.mark.parametrize("lo,hi", [(0, 192), (-37, 41)])
def test_garbled_single_layer(relu, lo, hi):
    """N = 75: every value in [q_lo - 3, q_hi + 3], both ends of the domain and random values in between
    decode to plain_q_eval exactly (the approximate sign at accuracy 100.0 included)."""
    N = 75
    gc = GarbledCircuit(d.Circuit([d.Clip.from_quantized((N,), lo, hi)]), 7, 100.0, seed=SEED, relu=relu)
    assert gc.hardened
    for x in clip_inputs(N, lo, hi, M7):
        np.testing.assert_array_equal(_host_eval(gc, x), gc.plain_q_eval(x))
        np.testing.assert_array_equal(gc.plain_q_eval(x), np.clip(x, lo, hi))


@pytest.mark.parametrize("relu", ["approx", "mrs"])
def test_garbled_dense_clip_dense(relu):
    rng = np.random.default_rng(3)
    c = dense_clip_dense(rng)
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED, relu=relu)
    for i in range(3):
        x = rng.integers(-20, 21, 30)
        np.testing.assert_array_equal(_host_eval(gc, x), gc.plain_q_eval(x))


def dense_clip_dense(rng):
    a = d.Dense.from_quantized(rng.integers(-4, 5, (24, 30)), rng.integers(-6, 6, 24))
    b = d.Dense.from_quantized(rng.integers(-4, 5, (6, 24)), rng.integers(-6, 6, 6))
    return d.Circuit([a, d.Clip.from_quantized((24,), -20, 60), b])


def test_table_entries_match_the_plan():
    """ClipPlan's comment: 2 n_sign + sum p_j + 3 k + 2 k entries per element (exact sign at k = 7: 387),
    against 2 n_sign + 2 sum p_j + 6 k of the two ReLUs it replaces."""
    crt, N = first_primes(7), 10
    k, P = len(crt), sum(crt)
    n_mrs = sum(crt[i + 1] * (k - 1 - i) for i in range(k - 1))
    clip = GarbledCircuit(d.Circuit([d.Clip.from_quantized((N,), 0, 192)]), 7, 100.0, seed=SEED, relu="mrs")
    relu = GarbledCircuit(d.Circuit([d.Relu((N,))]), 7, 100.0, seed=SEED, relu="mrs")
    assert clip.table_bytes == 16 * N * (2 * n_mrs + P + 5 * k) == 16 * N * 387
    assert 2 * relu.table_bytes == 16 * N * (2 * n_mrs + 2 * P + 6 * k)
    approx = GarbledCircuit(d.Circuit([d.Clip.from_quantized((N,), 0, 192)]), 7, 100.0, seed=SEED, relu="approx")
    arelu = GarbledCircuit(d.Circuit([d.Relu((N,))]), 7, 100.0, seed=SEED, relu="approx", hardened=True)
    n_approx = arelu.table_bytes // (16 * N) - P - 3 * k
    assert approx.table_bytes == 16 * N * (2 * n_approx + P + 5 * k)


# ---------------------------------------------------------------- 3. refusals
def test_reference_encoding_refused():
    c = d.Circuit([d.Clip.from_quantized((5,), 0, 192)])
    with pytest.raises(ValueError, match=r"layer 0 \(clip\).*hardened"):
        GarbledCircuit(c, 7, 100.0, seed=SEED, hardened=False)
    with pytest.raises(ValueError, match=r"layer 0 \(clip\).*hardened"):
        GarbledCircuit(c, 7, 100.0, seed=SEED, hardened=False, relu="mrs")
    with pytest.raises(ValueError, match=r"layer 0 \(clip\).*hardened"):
        GarbledCircuit(c, 7, 100.0, seed=SEED, fused_sign=False)  # the reference casts cannot be hardened
    # a legacy rescale cannot be hardened either
    c2 = d.Circuit([d.Rescale(2, (5,)), d.Clip.from_quantized((5,), 0, 192)])
    with pytest.raises(ValueError, match=r"layer 1 \(clip\).*hardened"):
        GarbledCircuit(c2, 7, 100.0, seed=SEED, rescale="legacy")


def test_joint_clip_uses_the_exact_sign_and_no_rescale_sign():
    c = d.Circuit([d.Rescale(3, (40,)), d.Clip.from_quantized((40,), -10, 25)])
    rng = np.random.default_rng(5)
    xs = [rng.integers(-400, 401, 40) for _ in range(2)]
    c.calibrate(xs, M7)
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED, rescale="mrs", relu="joint")
    m = gc.model
    resc, clip = m.layer_params(0), m.layer_params(1)
    assert "sign_out" not in resc or list(resc["sign_out"]) == [0]
    assert list(clip["smode"]) == [1]
    assert {"lo.mrs", "hi.mrs", "mm.g", "mm.e", "cap"} == set(m.layer_arrays(1))
    for x in xs:
        np.testing.assert_array_equal(_host_eval(gc, x), gc.plain_q_eval(x))


# ---------------------------------------------------------------- 4. wire format
def test_serialize_roundtrip():
    from dash_amd.native import native

    rng = np.random.default_rng(7)
    gc = GarbledCircuit(dense_clip_dense(rng), 7, 100.0, seed=SEED, relu="mrs")
    blob = gc.model.serialize()
    back = native().GarbledModel.deserialize(blob)
    assert bytes(back.serialize()) == bytes(blob)
    x = rng.integers(-20, 21, 30)
    enc = gc.garble_inputs(x)
    a, b = gc.cpu_evaluate(enc), native().cpu_evaluate(back, enc, 0)
    for (pa, la), (pb, lb) in zip(a, b):
        assert pa == pb
        np.testing.assert_array_equal(la, lb)


# sha256 of MODEL_A's offline message (ScaleQuant l = 5, seed 0, garbler seed 0..15, k = 7, accuracy 100.0),
# computed on the commit before the Clip layer: models without a Clip keep their bytes
MODEL_A_DIGESTS = {
    ("legacy", "approx", False): "20522046648ce9b9fd9461094f9f92262af6e3d4a99cc35b8b07468e871906f9",
    ("mrs", "joint", True): "c09caf634647f1da3278c2de479398eeabd76915c1feb8cae790b48447112d4e",
    ("mrs", "mrs", True): "d5d49129e947257a3a9860c6304f29e37dd38d742e69adf4b84ef64fd8eca469",
}


@pytest.mark.parametrize("rescale,relu,hardened", list(MODEL_A_DIGESTS))
def test_models_without_clip_keep_their_bytes(rescale, relu, hardened):
    from dash_amd.models import build_circuit

    c = build_circuit("MODEL_A", Q.ScaleQuant, 5, seed=0)
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED, rescale=rescale, relu=relu, hardened=hardened)
    assert hashlib.sha256(bytes(gc.model.serialize())).hexdigest() == MODEL_A_DIGESTS[(rescale, relu, hardened)]


# ---------------------------------------------------------------- 5. ONNX
def _onnx_model(path, nodes, inits, in_dims, out_name, out_dims, opset=11):
    from dash_amd.ir import onnx as o

    graph = b"".join(nodes) + o._s(2, "g") + b"".join(o._ld(5, o._tensor(n, v)) for n, v in inits.items())
    graph += o._ld(11, o._value_info("input", in_dims))
    graph += o._ld(12, o._value_info(out_name, out_dims))
    path.write_bytes(o._i(1, 7) + o._s(2, "test") + o._s(3, "1") + o._ld(7, graph) + o._ld(8, o._s(1, "") + o._i(2, opset)))
    return path


def _const_node(out, value):
    from dash_amd.ir import onnx as o

    # AttributeProto{name "value", t = TensorProto (field 5), type TENSOR (4)}
    attr = o._ld(5, o._s(1, "value") + o._ld(5, o._tensor("", np.float32(value))) + o._i(20, 4))
    return o._node("Constant", [], [out], f"const_{out}", attr)


def _conv_attrs(k, s=1, p=0):
    from dash_amd.ir import onnx as o

    return (o._attr_ints("dilations", [1, 1]) + o._attr_int("group", 1) + o._attr_ints("kernel_shape", [k, k])
            + o._attr_ints("pads", [p] * 4) + o._attr_ints("strides", [s, s]))


def _load(path, l=10):
    from dash_amd.ir.onnx import load_onnx_model

    return load_onnx_model(path, Q.ScaleQuant, l)


def _f32(rng, *shape):
    return rng.uniform(-0.5, 0.5, shape).astype(np.float32)


def _close(c, x, ref):
    np.testing.assert_allclose(c.plain_eval(x.reshape(-1), track=False), ref.detach().numpy().reshape(-1),
                               rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("form", ["init11", "const11", "attr6"])
def test_onnx_clip_forms(tmp_path, form):
    """Conv -> Clip(-0.25, 0.5) -> Conv with the bounds as opset-11 initializers, as opset-11 scalar Constant
    nodes and as opset-6 attributes, against the same network in PyTorch on 8 random inputs."""
    torch = pytest.importorskip("torch")
    from dash_amd.ir import onnx as o

    F = torch.nn.functional
    rng = np.random.default_rng(21)
    w1, b1, w2, b2 = _f32(rng, 4, 3, 3, 3), _f32(rng, 4), _f32(rng, 2, 4, 1, 1), _f32(rng, 2)
    inits = {"w1": w1, "b1": b1, "w2": w2, "b2": b2}
    pre = []
    if form == "init11":
        inits.update(lo=np.float32(-0.25), hi=np.float32(0.5))
        clip = o._node("Clip", ["c1", "lo", "hi"], ["a1"], "act")
    elif form == "const11":
        pre = [_const_node("lo", -0.25), _const_node("hi", 0.5)]
        clip = o._node("Clip", ["c1", "lo", "hi"], ["a1"], "act")
    else:
        clip = o._node("Clip", ["c1"], ["a1"], "act", o._attr_float("min", -0.25) + o._attr_float("max", 0.5))
    nodes = pre + [o._node("Conv", ["input", "w1", "b1"], ["c1"], "conv1", _conv_attrs(3, 1, 1)), clip,
                   o._node("Conv", ["a1", "w2", "b2"], ["out"], "conv2", _conv_attrs(1))]
    c = _load(_onnx_model(tmp_path / "clip.onnx", nodes, inits, (1, 3, 6, 6), "out", (1, 2, 6, 6),
                          opset=6 if form == "attr6" else 11))
    assert [l.name for l in c.layers] == ["conv2d", "rescale", "clip", "conv2d", "rescale"]
    assert (c.layers[2].q_lo, c.layers[2].q_hi) == (-256, 512)
    t = [torch.tensor(v) for v in (w1, b1, w2, b2)]
    for _ in range(8):
        x = _f32(rng, 3, 6, 6) * 4
        ref = F.conv2d(torch.clamp(F.conv2d(torch.tensor(x)[None], t[0], t[1], padding=1), -0.25, 0.5), t[2], t[3])
        _close(c, x, ref)


def test_onnx_min0_is_relu_and_open_bounds_are_refused(tmp_path):
    torch = pytest.importorskip("torch")
    from dash_amd.ir import onnx as o

    rng = np.random.default_rng(22)
    w = _f32(rng, 5, 12)
    b = _f32(rng, 5)
    gemm = o._attr_float("alpha", 1.0) + o._attr_float("beta", 1.0) + o._attr_int("transB", 1)

    def build(clip, inits=None, opset=11):
        nodes = [o._node("Gemm", ["input", "w", "b"], ["g"], "fc", gemm), clip]
        return _onnx_model(tmp_path / "m.onnx", nodes, dict({"w": w, "b": b}, **(inits or {})), (1, 12), "out", (1, 5),
                           opset=opset)

    c = _load(build(o._node("Clip", ["g", "zero"], ["out"], "relu_as_clip"), {"zero": np.float32(0.0)}))
    assert [l.name for l in c.layers] == ["dense", "rescale", "approx_relu"]
    for _ in range(8):
        x = _f32(rng, 12) * 4
        _close(c, x, torch.relu(torch.tensor(x) @ torch.tensor(w).T + torch.tensor(b)))
    c6 = _load(build(o._node("Clip", ["g"], ["out"], "relu6_as_attr", o._attr_float("min", 0.0)), opset=6))
    assert c6.layers[-1].name == "approx_relu"
    for clip, inits in [
        (o._node("Clip", ["g", "lo", "hi"], ["out"], "open_top"), {"lo": np.float32(0.5), "hi": np.float32(np.inf)}),
        (o._node("Clip", ["g", "lo"], ["out"], "open_top"), {"lo": np.float32(0.5)}),
        (o._node("Clip", ["g", "", "hi"], ["out"], "open_top"), {"hi": np.float32(6.0)}),
        (o._node("Clip", ["g", "lo", "hi"], ["out"], "open_top"), {"lo": np.float32(-np.inf), "hi": np.float32(6.0)}),
    ]:
        with pytest.raises(NotImplementedError, match="open_top"):
            _load(build(clip, inits))
    from dash_amd.ir.onnx import load_onnx_model

    p = build(o._node("Clip", ["g", "lo", "hi"], ["out"], "act6"), {"lo": np.float32(0.0), "hi": np.float32(6.0)})
    with pytest.raises(ValueError, match="act6.*SimpleQuant"):
        load_onnx_model(p, Q.SimpleQuant, -1, 0.02)


def test_onnx_average_factor_rescales_the_bounds(tmp_path):
    """AveragePool 2x2 (a sum pool and a pending 1/4) -> Clip(-0.25, 0.5) -> Conv: the Clip clamps the sum to
    (-1, 2) and the factor moves on into the conv's weights."""
    torch = pytest.importorskip("torch")
    from dash_amd.ir import onnx as o

    F = torch.nn.functional
    rng = np.random.default_rng(23)
    w, b = _f32(rng, 3, 2, 1, 1), _f32(rng, 3)
    pool = o._attr_ints("kernel_shape", [2, 2]) + o._attr_ints("pads", [0] * 4) + o._attr_ints("strides", [2, 2])
    nodes = [o._node("AveragePool", ["input"], ["p"], "pool", pool),
             o._node("Clip", ["p", "lo", "hi"], ["a"], "act"),
             o._node("Conv", ["a", "w", "b"], ["out"], "conv", _conv_attrs(1))]
    inits = {"w": w, "b": b, "lo": np.float32(-0.25), "hi": np.float32(0.5)}
    c = _load(_onnx_model(tmp_path / "avg.onnx", nodes, inits, (1, 2, 6, 6), "out", (1, 3, 3, 3)))
    assert [l.name for l in c.layers] == ["sum_pool", "clip", "conv2d", "rescale"]
    assert (c.layers[1].lo, c.layers[1].hi) == (-1.0, 2.0) and (c.layers[1].q_lo, c.layers[1].q_hi) == (-1024, 2048)
    for _ in range(8):
        x = _f32(rng, 2, 6, 6) * 4
        ref = F.conv2d(torch.clamp(F.avg_pool2d(torch.tensor(x)[None], 2), -0.25, 0.5), torch.tensor(w), torch.tensor(b))
        _close(c, x, ref)


def test_onnx_export_import_roundtrip(tmp_path):
    from dash_amd.ir.onnx import load_onnx_model, parse_onnx, save_onnx_model

    c, xs, _ = tiny_mobilenet()
    save_onnx_model(tmp_path / "tiny.onnx", c)
    m = parse_onnx(tmp_path / "tiny.onnx")
    clips = [n for n in m["nodes"] if n["op_type"] == "Clip"]
    assert len(clips) == 5 and all(len(n["inputs"]) == 3 and not n["attrs"] for n in clips)
    back = load_onnx_model(tmp_path / "tiny.onnx", Q.ScaleQuant, 5)
    assert [l.name for l in back.layers] == [l.name for l in c.layers]
    for a, b in zip(c.layers, back.layers):
        if a.name == "clip":
            assert (a.q_lo, a.q_hi) == (b.q_lo, b.q_hi)
    for x in xs:
        np.testing.assert_array_equal(back.plain_q_eval(x, False, M7), c.plain_q_eval(x, False, M7))


# ---------------------------------------------------------------- 6. range guard
def guard_case():
    """A circuit with a Clip and three inputs: in range, x - q_hi just below -M/2, x - q_lo just at M/2."""
    c = d.Circuit([d.Clip.from_quantized((6,), -37, 41)])
    h = M7 // 2
    ok = np.array([-h + 41, M7 - h - 37 - 1, 0, -37, 41, 5])
    low, high = ok.copy(), ok.copy()
    low[0] -= 1    # x - q_hi = -M/2 - 1
    high[1] += 1   # x - q_lo = M/2
    return c, [ok, low, high], [False, True, True]


def test_range_guard_flags_both_sign_inputs():
    pytest.importorskip("torch")
    c, xs, want = guard_case()
    g = RangeGuard(c, M7, mrs=True, device=None)
    assert g.batched and not g.native_forms and not g._native_ok()
    assert [bool(g.violations_np(x)) for x in xs] == want
    assert g.submit(xs).bad_indices() == [i for i, w in enumerate(want) if w]  # the torch path, CPU device
    with pytest.raises(RangeGuardError):
        g.check(xs)
    # range_guard="auto" is on for a circuit with a Clip: an input outside the domain is refused, not mis-decoded
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED, relu="mrs")
    assert gc.guard_enabled
    gc.garble_inputs(xs[0])
    for x in xs[1:]:
        with pytest.raises(RangeGuardError):
            gc.garble_inputs(x)


# ---------------------------------------------------------------- 7. zoo
def test_mobilenet_cifar_builds_and_sizes():
    from dash_amd.models import BENCH_CONFIGS, build_circuit, quantized_inputs

    cfg = BENCH_CONFIGS["MOBILENET_CIFAR/DASH"]
    assert (cfg["q_method"], cfg["q_parameter"], cfg["crt"]) == (Q.ScaleQuant, 5, 7)
    c = build_circuit("MOBILENET_CIFAR", cfg["q_method"], cfg["q_parameter"], seed=0)
    clips = [l for l in c.layers if l.name == "clip"]
    assert len(clips) == 7 and all((l.q_lo, l.q_hi) == (0, 192) for l in clips)
    assert not any(l.name == "approx_relu" for l in c.layers) and c.output_dims == (10,)
    xs = quantized_inputs("MOBILENET_CIFAR", 2, cfg["q_method"], cfg["q_parameter"], seed=1)
    assert c.infer_crt_base_size(xs) <= 8


def test_tiny_mobilenet_garbled_matches_plain():
    c, xs, k = tiny_mobilenet()
    assert k <= 8
    # both bounds of some Clip are reached, so the cap and the pass-through both run
    acts = [xs[0]]
    for l in c.layers:
        acts.append(l.plain_q_eval(acts[-1], False, None, M7))
    ins = [a for l, a in zip(c.layers, acts) if l.name == "clip"]
    assert any((a > l.q_hi).any() for l, a in zip([l for l in c.layers if l.name == "clip"], ins))
    assert any((a < l.q_lo).any() for l, a in zip([l for l in c.layers if l.name == "clip"], ins))
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED, rescale="mrs", relu="joint", hardened=True)
    for x in xs:
        np.testing.assert_array_equal(_host_eval(gc, x), gc.plain_q_eval(x))


def test_trainer_maps_relu6_and_clip():
    """models/train.py: relu6 / clip ops become nn.ReLU6 / nn.Hardtanh and come back as Clip layers."""
    torch = pytest.importorskip("torch")
    from dash_amd.models import train, zoo

    zoo.ARCHS["_TINY_CLIP_SEQ"] = {"input": (1, 6, 6), "ops": [
        ("conv", 2, 3, 1, 1), ("relu6",), ("flatten",), ("fc", 5), ("clip", -0.5, 0.25), ("fc", 3)]}
    try:
        model = train.build_torch_model("_TINY_CLIP_SEQ")
        acts = [m for m in model if isinstance(m, torch.nn.Hardtanh)]
        assert [type(m) for m in acts] == [torch.nn.ReLU6, torch.nn.Hardtanh]
        assert (acts[1].min_val, acts[1].max_val) == (-0.5, 0.25)
        c = train.to_circuit(model, "_TINY_CLIP_SEQ", Q.ScaleQuant, 5)
    finally:
        del zoo.ARCHS["_TINY_CLIP_SEQ"]
    clips = [l for l in c.layers if l.name == "clip"]
    assert [(l.q_lo, l.q_hi) for l in clips] == [(0, 192), (-16, 8)]
    x = np.random.default_rng(0).standard_normal(36).astype(np.float32)
    model.fq.c = 0  # the float network
    with torch.no_grad():
        ref = model(torch.tensor(x).view(1, 1, 6, 6)).numpy().reshape(-1)
    np.testing.assert_allclose(c.plain_eval(x, track=False), ref, rtol=1e-4, atol=1e-5)
