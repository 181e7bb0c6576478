"""Branching graphs and general pooling geometry on the host: padded / ceil-mode MaxPool2d and SumPool2d, the
Concat layer, garbling and the host evaluator, serialization, graph-aware ONNX import / export, the range
guard's torch path and the SqueezeNet-style zoo model.

Pooling rules (docs/BRANCHING_GRAPHS.md): output sizes follow PyTorch / ONNX; a sum-pool tap outside the image
is skipped, a max-pool tap outside the image reads the clamped coordinate (a member of the same window, so the
max is unchanged and every window keeps kh*kw values).
"""
from __future__ import annotations

import itertools

import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit, RangeGuard
from dash_amd.ir.bases import crt_modulus, first_primes
from dash_amd.native import native

M7 = crt_modulus(first_primes(7))


# ---------------------------------------------------------------- shared circuits (also used by the GPU tests)
def _conv(rng, C, F, k, h, w, pad=0):
    wt = rng.integers(-4, 5, (F, C, k, k))
    wt.reshape(-1)[::5] = 0  # zero weights take the Z_p quirk
    return d.Conv2d.from_quantized(wt, rng.integers(-5, 6, F), w, h, C, F, k, k, pad_width=pad, pad_height=pad)


def fire_circuit(seed=3):
    """Fire-like module on 2x6x6: 1x1 squeeze, then a 1x1 and a padded 3x3 expand that both read the squeeze
    output (Rescale + ReLU in every branch), then Concat; calibrated for the mixed-radix constructions."""
    rng = np.random.default_rng(seed)
    sq = _conv(rng, 2, 3, 1, 6, 6)
    e1 = _conv(rng, 3, 2, 1, 6, 6)
    e3 = _conv(rng, 3, 3, 3, 6, 6, pad=1)
    e3.in_src = 2
    layers = [sq, d.Rescale(1, sq.out_dims), d.Relu(sq.out_dims),
              e1, d.Rescale(2, e1.out_dims), d.Relu(e1.out_dims),
              e3, d.Rescale(2, e3.out_dims), d.Relu(e3.out_dims),
              d.Concat([e1.out_dims, e3.out_dims], [5, 8])]
    c = d.Circuit(layers)
    xs = [rng.integers(-20, 21, c.input_size) for _ in range(4)]
    c.calibrate(xs, M7)
    return c, xs


def pools_circuit(seed=4):
    """Padded 3x3/s2 ceil-mode max pool on 3x7x7, then a padded 3x3/s1 sum pool."""
    rng = np.random.default_rng(seed)
    mp = d.MaxPool2d(7, 7, 3, 3, 3, 2, 2, pad_width=1, pad_height=1, ceil_mode=True)
    C, H, W = mp.out_dims
    sp = d.SumPool2d(W, H, C, 3, 3, 1, 1, pad_width=1, pad_height=1)
    c = d.Circuit([mp, sp])
    xs = [rng.integers(-30, 31, c.input_size) for _ in range(4)]
    c.calibrate(xs, M7)
    return c, xs


def concat_circuit(rng, order=(0, 1, -1), n_in=12, n0=75, n1=50):
    """Two dense layers on the circuit input (the second through in_src) and a Concat of 1-D operands."""
    a = d.Dense.from_quantized(rng.integers(-3, 4, (n0, n_in)), rng.integers(-5, 6, n0))
    b = d.Dense.from_quantized(rng.integers(-3, 4, (n1, n_in)), rng.integers(-5, 6, n1))
    b.in_src = -1
    dims = {-1: (n_in,), 0: (n0,), 1: (n1,)}
    return d.Circuit([a, b, d.Concat([dims[s] for s in order], list(order))])


# ---------------------------------------------------------------- 1. pool semantics
SHAPES = [(5, 7), (6, 6), (9, 4), (13, 13)]
KERNELS = [(2, 2), (3, 3), (3, 2), None]  # None: the full plane
STRIDES = [(1, 1), (2, 2), (2, 1), (3, 3)]
PADS = [(0, 0), (1, 1), (1, 0)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_pool_semantics_match_torch(H, W):
    torch = pytest.importorskip("torch")
    F = torch.nn.functional
    C = 2
    rng = np.random.default_rng(H * 31 + W)
    x = rng.integers(-50, 51, (C, H, W))
    xt = torch.tensor(x, dtype=torch.float64)[None]
    n = 0
    for k, (sh, sw), (ph, pw), ceil in itertools.product(KERNELS, STRIDES, PADS, (False, True)):
        kh, kw = k or (H, W)
        mp = d.MaxPool2d(W, H, C, kw, kh, sw, sh, pad_width=pw, pad_height=ph, ceil_mode=ceil)
        sp = d.SumPool2d(W, H, C, kw, kh, sw, sh, pad_width=pw, pad_height=ph, ceil_mode=ceil)
        rm = F.max_pool2d(xt, (kh, kw), (sh, sw), (ph, pw), ceil_mode=ceil)[0]
        rs = F.avg_pool2d(xt, (kh, kw), (sh, sw), (ph, pw), ceil_mode=ceil, count_include_pad=True,
                          divisor_override=1)[0]
        assert mp.out_dims == tuple(rm.shape) and sp.out_dims == tuple(rs.shape), (k, sh, sw, ph, pw, ceil)
        np.testing.assert_array_equal(mp.plain_q_eval(x.reshape(-1), track=False), rm.numpy().reshape(-1).astype(np.int64))
        np.testing.assert_array_equal(sp.plain_q_eval(x.reshape(-1), track=False), rs.numpy().reshape(-1).astype(np.int64))
        # every max window keeps kh*kw values (duplicates at the border), all of them members of the window
        assert len(mp._windows(x)) == kh * kw
        n += 1
    assert n == 96  # 4 kernels x 4 strides x 3 pads x 2 modes, per shape: 384 in all


def test_pool_pads_above_half_kernel_raise():
    with pytest.raises(ValueError, match="half the kernel"):
        d.MaxPool2d(8, 8, 1, 3, 3, 1, 1, pad_width=2, pad_height=2)
    with pytest.raises(ValueError, match="half the kernel"):
        d.SumPool2d(8, 8, 1, 2, 3, 1, 1, pad_width=2, pad_height=1)
    d.MaxPool2d(8, 8, 1, 2, 2, 2, 2, pad_width=1, pad_height=1)  # exactly half is fine


# ---------------------------------------------------------------- 2. concat
def test_concat_semantics():
    rng = np.random.default_rng(0)
    x = rng.integers(-9, 10, 12)
    c = concat_circuit(rng)
    a, b = c.layers[0], c.layers[1]
    ya, yb = a.plain_q_eval(x, False), b.plain_q_eval(x, False)
    assert ya.size == 75 and yb.size == 50
    y = c.plain_q_eval(x)
    assert c.output_dims == (137,)
    np.testing.assert_array_equal(y, np.concatenate([ya, yb, x]))
    # order is respected; the same source may appear twice
    c.layers[2] = d.Concat([(50,), (12,), (75,)], [1, -1, 0])
    np.testing.assert_array_equal(c.plain_q_eval(x), np.concatenate([yb, x, ya]))
    c.layers[2] = d.Concat([(75,), (75,)], [0, 0])
    np.testing.assert_array_equal(c.plain_q_eval(x), np.concatenate([ya, ya]))
    np.testing.assert_array_equal(c.plain_eval(x.astype(np.float32)), np.concatenate([ya, ya]).astype(np.float32))
    # images concatenate along channels
    cat = d.Concat([(3, 5, 5), (2, 5, 5)], [0, 1])
    assert cat.out_dims == (5, 5, 5)
    assert cat.garble_spec() == (14, {"srcs": [0, 1]})
    with pytest.raises(ValueError):
        d.Concat([(3, 5, 5), (2, 5, 4)], [0, 1])
    with pytest.raises(ValueError):
        d.Concat([(3, 5, 5), (50,)], [0, 1])


# ---------------------------------------------------------------- 3. garble, CPU-evaluate, decode
def _garble_eval(c, xs, hardened, **kw):
    for i, x in enumerate(xs):
        gc = GarbledCircuit(c, 7, 100.0, seed=bytes([i + 9]) * 16, hardened=hardened, **kw)
        y = gc.decode_outputs(gc.cpu_evaluate(gc.garble_inputs(x)))
        np.testing.assert_array_equal(y, gc.plain_q_eval(x))


@pytest.mark.parametrize("hardened", [True, False], ids=["hardened", "reference"])
@pytest.mark.parametrize("name", ["fire", "pools", "concat"])
def test_garbled_matches_plain(name, hardened):
    if name == "fire":
        c, xs = fire_circuit()
        # the hardened encoding has no legacy rescale: it runs the mixed-radix constructions
        kw = dict(rescale="mrs", relu="joint") if hardened else dict(rescale="legacy", relu="approx")
        _garble_eval(c, xs[:2], hardened, **kw)
    elif name == "pools":
        c, xs = pools_circuit()
        _garble_eval(c, xs[:2], hardened)
    else:
        rng = np.random.default_rng(1)
        c = concat_circuit(rng, order=(1, -1, 0, 1))
        _garble_eval(c, [rng.integers(-9, 10, 12)], hardened)


# ---------------------------------------------------------------- 4. serialization
@pytest.mark.parametrize("name", ["fire", "pools"])
def test_serialize_roundtrip(name):
    c, xs = fire_circuit() if name == "fire" else pools_circuit()
    gc = GarbledCircuit(c, 7, 100.0, seed=b"b" * 16, rescale="legacy", relu="approx")
    blob = gc.model.serialize()
    m2 = native().GarbledModel.deserialize(blob)
    assert m2.serialize() == blob
    enc = gc.garble_inputs(xs[0])
    for (p1, x1), (p2, x2) in zip(gc.cpu_evaluate(enc), native().cpu_evaluate(m2, enc, 0)):
        assert p1 == p2
        np.testing.assert_array_equal(x1, x2)
    if name == "fire":
        assert m2.layer_kind(9) == 14 and list(m2.layer_params(9)["srcs"]) == [5, 8]
    else:
        p = m2.layer_params(0)
        assert (list(p["ph"]), list(p["pw"]), list(p["ceil"])) == ([1], [1], [1])
        assert "ceil" not in m2.layer_params(1)


def test_unpadded_pools_keep_their_wire_params():
    """ph / pw / ceil are emitted only when set: pools without padding serialize to the bytes they always had."""
    for cls in (d.MaxPool2d, d.SumPool2d):
        kind, spec = cls(8, 6, 3, 2, 3).garble_spec()
        assert sorted(spec) == ["C", "H", "W", "kh", "kw", "sh", "sw"]
        _, spec = cls(8, 6, 3, 2, 3, pad_width=1).garble_spec()
        assert spec["pw"] == 1 and "ph" not in spec and "ceil" not in spec
        _, spec = cls(8, 6, 3, 2, 3, ceil_mode=True).garble_spec()
        assert spec["ceil"] == 1 and "ph" not in spec and "pw" not in spec
    c = d.Circuit([d.MaxPool2d(8, 8, 2, 2, 2), d.SumPool2d(4, 4, 2, 2, 2)])
    gc = GarbledCircuit(c, 7, 100.0, seed=b"u" * 16)
    for i in range(2):
        assert not {"ph", "pw", "ceil"} & set(gc.model.layer_params(i))


# ---------------------------------------------------------------- 5. ONNX import of hand-built graphs
def _onnx_model(path, nodes, inits, in_dims, out_name, out_dims, producer="test"):
    from dash_amd.ir import onnx as o

    graph = b"".join(nodes) + o._s(2, "g") + b"".join(o._ld(5, o._tensor(n, v)) for n, v in inits.items())
    graph += o._ld(11, o._value_info("input", in_dims))
    graph += o._ld(12, o._value_info(out_name, out_dims))
    path.write_bytes(o._i(1, 7) + o._s(2, producer) + o._s(3, "1") + o._ld(7, graph) + o._ld(8, o._s(1, "") + o._i(2, 13)))
    return path


def _conv_attrs(k, s=1, p=0):
    from dash_amd.ir import onnx as o

    return (o._attr_ints("dilations", [1, 1]) + o._attr_int("group", 1) + o._attr_ints("kernel_shape", [k, k])
            + o._attr_ints("pads", [p] * 4) + o._attr_ints("strides", [s, s]))


def _pool_attrs(k, s, p=0, ceil=0, extra=b""):
    from dash_amd.ir import onnx as o

    a = o._attr_ints("kernel_shape", [k, k]) + o._attr_ints("pads", [p] * 4) + o._attr_ints("strides", [s, s])
    return a + (o._attr_int("ceil_mode", 1) if ceil else b"") + extra


def _load(path):
    from dash_amd.ir.onnx import load_onnx_model
    from dash_amd.ir.quant import QuantizationMethod as Q

    return load_onnx_model(path, Q.SimpleQuant, -1, 2.0 ** -10)


def _f32(rng, *shape):
    return rng.uniform(-0.5, 0.5, shape).astype(np.float32)


def _bn(rng, n):
    return {"scale": rng.uniform(0.5, 1.5, n).astype(np.float32), "shift": _f32(rng, n), "mean": _f32(rng, n),
            "var": rng.uniform(0.5, 2.0, n).astype(np.float32)}


def _close(c, x, ref):
    np.testing.assert_allclose(c.plain_eval(x.reshape(-1), track=False), ref.detach().numpy().reshape(-1),
                               rtol=1e-4, atol=1e-5)


def test_onnx_projection_shortcut(tmp_path):
    """(a) a torchvision-style ResNet block: conv-bn-relu-conv-bn on the main path, a 1x1 stride-2 conv + bn
    that reads the block input, then Add of the two earlier tensors and Relu."""
    torch = pytest.importorskip("torch")
    from dash_amd.ir import onnx as o
    F = torch.nn.functional
    rng = np.random.default_rng(10)
    w1, b1, w2, b2, wd, bd = _f32(rng, 8, 4, 3, 3), _f32(rng, 8), _f32(rng, 8, 8, 3, 3), _f32(rng, 8), \
        _f32(rng, 8, 4, 1, 1), _f32(rng, 8)
    bns = [_bn(rng, 8) for _ in range(3)]
    inits = {"w1": w1, "b1": b1, "w2": w2, "b2": b2, "wd": wd, "bd": bd}
    for i, bn in enumerate(bns):
        inits.update({f"{k}{i}": v for k, v in bn.items()})

    def bn_node(i, src, out):
        return o._node("BatchNormalization", [src, f"scale{i}", f"shift{i}", f"mean{i}", f"var{i}"], [out], f"bn{i}",
                       o._attr_float("epsilon", 1e-5))

    nodes = [o._node("Conv", ["input", "w1", "b1"], ["c1"], "conv1", _conv_attrs(3, 2, 1)), bn_node(0, "c1", "n1"),
             o._node("Relu", ["n1"], ["r1"], "relu1"),
             o._node("Conv", ["r1", "w2", "b2"], ["c2"], "conv2", _conv_attrs(3, 1, 1)), bn_node(1, "c2", "n2"),
             o._node("Conv", ["input", "wd", "bd"], ["cd"], "down", _conv_attrs(1, 2, 0)), bn_node(2, "cd", "nd"),
             o._node("Add", ["n2", "nd"], ["sum"], "add"), o._node("Relu", ["sum"], ["out"], "relu2")]
    c = _load(_onnx_model(tmp_path / "block.onnx", nodes, inits, (1, 4, 8, 8), "out", (1, 8, 4, 4)))
    assert [type(l).__name__ for l in c.layers] == ["Conv2d", "Relu", "Conv2d", "Conv2d", "Add", "Relu"]
    assert c.layers[3].in_src == -1 and c.layers[4].src == 2

    def tbn(y, bn):
        t = {k: torch.tensor(v) for k, v in bn.items()}
        return F.batch_norm(y, t["mean"], t["var"], t["scale"], t["shift"], False, 0.0, 1e-5)

    x = _f32(rng, 1, 4, 8, 8)
    xt = torch.tensor(x)
    main = torch.relu(tbn(F.conv2d(xt, torch.tensor(w1), torch.tensor(b1), 2, 1), bns[0]))
    main = tbn(F.conv2d(main, torch.tensor(w2), torch.tensor(b2), 1, 1), bns[1])
    ref = torch.relu(main + tbn(F.conv2d(xt, torch.tensor(wd), torch.tensor(bd), 2, 0), bns[2]))
    _close(c, x, ref)


def test_onnx_padded_maxpool_and_global_average_fold(tmp_path):
    """(b) stem + MaxPool(3, 2, pad 1) + GlobalAveragePool + Flatten + Gemm: the 1/K of the average goes into
    the Gemm's weights, not its bias."""
    torch = pytest.importorskip("torch")
    from dash_amd.ir import onnx as o
    F = torch.nn.functional
    rng = np.random.default_rng(11)
    w, b, fw, fb = _f32(rng, 6, 3, 3, 3), _f32(rng, 6), _f32(rng, 5, 6), _f32(rng, 5)
    nodes = [o._node("Conv", ["input", "w", "b"], ["c"], "stem", _conv_attrs(3, 1, 1)),
             o._node("Relu", ["c"], ["r"], "relu"),
             o._node("MaxPool", ["r"], ["m"], "pool", _pool_attrs(3, 2, 1)),
             o._node("GlobalAveragePool", ["m"], ["g"], "gap"),
             o._node("Flatten", ["g"], ["f"], "flat", o._attr_int("axis", 1)),
             o._node("Gemm", ["f", "fw", "fb"], ["out"], "fc",
                     o._attr_float("alpha", 1.0) + o._attr_float("beta", 1.0) + o._attr_int("transB", 1))]
    c = _load(_onnx_model(tmp_path / "gap.onnx", nodes, {"w": w, "b": b, "fw": fw, "fb": fb}, (1, 3, 9, 9), "out",
                          (1, 5)))
    assert [type(l).__name__ for l in c.layers] == ["Conv2d", "Relu", "MaxPool2d", "SumPool2d", "Flatten", "Dense"]
    mp, sp, fc = c.layers[2], c.layers[3], c.layers[5]
    assert (mp.ph, mp.pw, mp.out_dims) == (1, 1, (6, 5, 5)) and sp.out_dims == (6, 1, 1)
    np.testing.assert_array_equal(fc.weights, fw * np.float32(1 / 25))
    np.testing.assert_array_equal(fc.biases, fb)
    x = _f32(rng, 1, 3, 9, 9)
    y = F.max_pool2d(torch.relu(F.conv2d(torch.tensor(x), torch.tensor(w), torch.tensor(b), 1, 1)), 3, 2, 1)
    ref = F.linear(F.adaptive_avg_pool2d(y, 1).flatten(1), torch.tensor(fw), torch.tensor(fb))
    _close(c, x, ref)


def test_onnx_fire_module_concat_ceil_maxpool(tmp_path):
    """(c) a fire module (both expands read the squeeze output) with Concat and a ceil_mode max pool."""
    torch = pytest.importorskip("torch")
    from dash_amd.ir import onnx as o
    F = torch.nn.functional
    rng = np.random.default_rng(12)
    ws, bs, w1, b1, w3, b3 = _f32(rng, 3, 4, 1, 1), _f32(rng, 3), _f32(rng, 5, 3, 1, 1), _f32(rng, 5), \
        _f32(rng, 2, 3, 3, 3), _f32(rng, 2)
    nodes = [o._node("Conv", ["input", "ws", "bs"], ["s"], "squeeze", _conv_attrs(1)),
             o._node("Relu", ["s"], ["sr"], "relu_s"),
             o._node("Conv", ["sr", "w1", "b1"], ["e1"], "expand1", _conv_attrs(1)),
             o._node("Relu", ["e1"], ["e1r"], "relu_1"),
             o._node("Conv", ["sr", "w3", "b3"], ["e3"], "expand3", _conv_attrs(3, 1, 1)),
             o._node("Relu", ["e3"], ["e3r"], "relu_3"),
             o._node("Concat", ["e1r", "e3r"], ["cat"], "cat", o._attr_int("axis", 1)),
             o._node("MaxPool", ["cat"], ["out"], "pool", _pool_attrs(3, 2, 0, ceil=1))]
    inits = {"ws": ws, "bs": bs, "w1": w1, "b1": b1, "w3": w3, "b3": b3}
    c = _load(_onnx_model(tmp_path / "fire.onnx", nodes, inits, (1, 4, 6, 6), "out", (1, 7, 3, 3)))
    assert [type(l).__name__ for l in c.layers] == ["Conv2d", "Relu", "Conv2d", "Relu", "Conv2d", "Relu", "Concat",
                                                    "MaxPool2d"]
    assert c.layers[4].in_src == 1 and c.layers[6].srcs == [3, 5] and c.layers[2].in_src is None
    assert c.layers[7].ceil_mode and c.output_dims == (7, 3, 3)
    x = _f32(rng, 1, 4, 6, 6)
    s = torch.relu(F.conv2d(torch.tensor(x), torch.tensor(ws), torch.tensor(bs)))
    cat = torch.cat([torch.relu(F.conv2d(s, torch.tensor(w1), torch.tensor(b1))),
                     torch.relu(F.conv2d(s, torch.tensor(w3), torch.tensor(b3), 1, 1))], 1)
    _close(c, x, F.max_pool2d(cat, 3, 2, 0, ceil_mode=True))


@pytest.mark.parametrize("keepdims", [0, 1])
def test_onnx_reduce_mean(tmp_path, keepdims):
    """(d) ReduceMean over (2, 3), with either keepdims, then a Gemm that absorbs the 1/K."""
    torch = pytest.importorskip("torch")
    from dash_amd.ir import onnx as o
    F = torch.nn.functional
    rng = np.random.default_rng(13)
    w, b, fw, fb = _f32(rng, 4, 2, 3, 3), _f32(rng, 4), _f32(rng, 3, 4), _f32(rng, 3)
    gemm = o._attr_float("alpha", 1.0) + o._attr_float("beta", 1.0) + o._attr_int("transB", 1)
    nodes = [o._node("Conv", ["input", "w", "b"], ["c"], "conv", _conv_attrs(3)),
             o._node("ReduceMean", ["c"], ["m"], "mean", o._attr_ints("axes", [2, 3]) + o._attr_int("keepdims", keepdims))]
    if keepdims:
        nodes += [o._node("Flatten", ["m"], ["f"], "flat", o._attr_int("axis", 1)),
                  o._node("Gemm", ["f", "fw", "fb"], ["out"], "fc", gemm)]
    else:
        nodes += [o._node("Gemm", ["m", "fw", "fb"], ["out"], "fc", gemm)]
    c = _load(_onnx_model(tmp_path / "mean.onnx", nodes, {"w": w, "b": b, "fw": fw, "fb": fb}, (1, 2, 7, 6), "out",
                          (1, 3)))
    assert [type(l).__name__ for l in c.layers] == ["Conv2d", "SumPool2d", "Flatten", "Dense"]
    np.testing.assert_array_equal(c.layers[3].biases, fb)
    x = _f32(rng, 1, 2, 7, 6)
    y = F.conv2d(torch.tensor(x), torch.tensor(w), torch.tensor(b))
    _close(c, x, F.linear(y.mean((2, 3)), torch.tensor(fw), torch.tensor(fb)))
    # other axes are refused
    nodes[1] = o._node("ReduceMean", ["c"], ["m"], "mean", o._attr_ints("axes", [1, 2]) + o._attr_int("keepdims", keepdims))
    with pytest.raises(NotImplementedError, match="ReduceMean"):
        _load(_onnx_model(tmp_path / "bad.onnx", nodes, {"w": w, "b": b, "fw": fw, "fb": fb}, (1, 2, 7, 6), "out",
                          (1, 3)))


def test_onnx_refusals(tmp_path):
    from dash_amd.ir import onnx as o

    rng = np.random.default_rng(14)
    w, b = _f32(rng, 4, 4, 1, 1), _f32(rng, 4)
    conv = o._node("Conv", ["input", "w", "b"], ["c"], "conv", _conv_attrs(1))
    inits = {"w": w, "b": b}
    # AveragePool with pads and count_include_pad = 0: the divisor varies per position
    nodes = [conv, o._node("AveragePool", ["c"], ["a"], "avg_pad", _pool_attrs(3, 1, 1)),
             o._node("Conv", ["a", "w", "b"], ["out"], "conv2", _conv_attrs(1))]
    with pytest.raises(NotImplementedError, match="count_include_pad"):
        _load(_onnx_model(tmp_path / "a.onnx", nodes, inits, (1, 4, 6, 6), "out", (1, 4, 6, 6)))
    # ... with count_include_pad = 1 it imports, the 1/9 in the next conv's weights
    nodes[1] = o._node("AveragePool", ["c"], ["a"], "avg_pad", _pool_attrs(3, 1, 1, extra=o._attr_int("count_include_pad", 1)))
    c = _load(_onnx_model(tmp_path / "a1.onnx", nodes, inits, (1, 4, 6, 6), "out", (1, 4, 6, 6)))
    assert isinstance(c.layers[1], d.SumPool2d) and c.layers[1].ph == 1
    np.testing.assert_array_equal(c.layers[2].weights, w * np.float32(1 / 9))
    # Concat on another axis
    nodes = [conv, o._node("Relu", ["c"], ["r"], "relu"), o._node("Concat", ["c", "r"], ["out"], "cat_h", o._attr_int("axis", 2))]
    with pytest.raises(NotImplementedError, match="cat_h"):
        _load(_onnx_model(tmp_path / "b.onnx", nodes, inits, (1, 4, 6, 6), "out", (1, 4, 12, 6)))
    # an average whose factor reaches an Add
    nodes = [conv, o._node("AveragePool", ["c"], ["a"], "avg", _pool_attrs(1, 1)),
             o._node("AveragePool", ["c"], ["a2"], "avg2", _pool_attrs(3, 1, 1, extra=o._attr_int("count_include_pad", 1))),
             o._node("Add", ["a", "a2"], ["out"], "add_avg")]
    with pytest.raises(NotImplementedError, match="add_avg"):
        _load(_onnx_model(tmp_path / "c.onnx", nodes, inits, (1, 4, 6, 6), "out", (1, 4, 6, 6)))
    # ... a Concat, and a graph output
    nodes[3] = o._node("Concat", ["c", "a2"], ["out"], "cat_avg", o._attr_int("axis", 1))
    with pytest.raises(NotImplementedError, match="cat_avg"):
        _load(_onnx_model(tmp_path / "d.onnx", nodes, inits, (1, 4, 6, 6), "out", (1, 8, 6, 6)))
    with pytest.raises(NotImplementedError, match="graph output"):
        _load(_onnx_model(tmp_path / "e.onnx", nodes[:3], inits, (1, 4, 6, 6), "a2", (1, 4, 6, 6)))
    # asymmetric max-pool pads
    nodes = [conv, o._node("MaxPool", ["c"], ["out"], "mp_asym",
                           o._attr_ints("kernel_shape", [3, 3]) + o._attr_ints("pads", [0, 0, 1, 1]))]
    with pytest.raises(NotImplementedError, match="mp_asym"):
        _load(_onnx_model(tmp_path / "f.onnx", nodes, inits, (1, 4, 6, 6), "out", (1, 4, 5, 5)))


# ---------------------------------------------------------------- 6. export round trip
@pytest.mark.parametrize("name", ["RESNET18", "MODEL_DWSEP_CIFAR", "SQUEEZENET_CIFAR"])
def test_export_roundtrip(tmp_path, name):
    """Save, load with the same quantization: equal quantized weights, equal plain_q_eval. The pooled windows
    (K = 16) are powers of two, so the K / (1/K) fold is exact in float32."""
    from dash_amd.ir.onnx import load_onnx_model, save_onnx_model
    from dash_amd.ir.quant import QuantizationMethod as Q
    from dash_amd.models import build_circuit, quantized_inputs

    c = build_circuit(name, Q.ScaleQuant, 5, seed=2)
    pools = [l for l in c.layers if isinstance(l, d.SumPool2d)]
    assert [l.kh * l.kw for l in pools] == [16]
    p = tmp_path / f"{name}.onnx"
    save_onnx_model(p, c)
    c2 = load_onnx_model(p, Q.ScaleQuant, 5)
    assert [type(l) for l in c2.layers] == [type(l) for l in c.layers]
    for a, b in zip(c.layers, c2.layers):
        assert a.in_src == b.in_src and a.out_dims == b.out_dims
        if isinstance(a, (d.Conv2d, d.Dense)):
            np.testing.assert_array_equal(a.q_weights, b.q_weights)
            np.testing.assert_array_equal(a.q_biases, b.q_biases)
        if isinstance(a, d.Add):
            assert a.src == b.src
        if isinstance(a, d.Concat):
            assert a.srcs == b.srcs
    for x in quantized_inputs(name, 2, Q.ScaleQuant, 5, seed=4):
        np.testing.assert_array_equal(c.plain_q_eval(x, track=False), c2.plain_q_eval(x, track=False))


# ---------------------------------------------------------------- 7. range guard
def guard_circuit():
    """Padded max pool -> Concat(pooled, pooled) -> Rescale(5) -> ReLU on 2x5x5: the max pool and the concat
    preserve values, so the rescale sees the largest input itself."""
    mp = d.MaxPool2d(5, 5, 2, 3, 3, 1, 1, pad_width=1, pad_height=1)
    cat = d.Concat([mp.out_dims, mp.out_dims, mp.in_dims], [0, 0, -1])
    c = d.Circuit([mp, cat, d.Rescale(5, cat.out_dims), d.Relu(cat.out_dims)])
    rng = np.random.default_rng(0)
    c.calibrate([rng.integers(-50, 51, size=c.input_size) for _ in range(8)], M7)
    return c


def guard_inputs(c):
    """In-range inputs, one pushed into the wrap band (index 3) and the last in-range value."""
    lim = c.layers[2].mrs_limit(M7)
    assert lim < M7 // 2
    rng = np.random.default_rng(1)
    xs = [rng.integers(-50, 51, size=c.input_size) for _ in range(3)]
    band, ok = xs[0].copy(), xs[1].copy()
    band[:] = lim - 200  # the window span stays small: only the rescale's band is hit
    ok[:] = lim - 200
    band[17] = lim
    ok[17] = lim - 1
    return xs + [band, ok]


def test_range_guard_torch_matches_numpy():
    c = guard_circuit()
    xs = guard_inputs(c)
    g = RangeGuard(c, M7, mrs=True)
    assert g.batched
    ref = [i for i, x in enumerate(xs) if g.violations_np(x)]
    assert ref == [3]
    assert sorted(g.submit(xs).bad_indices()) == ref
    gd = RangeGuard(c, M7, mrs=True, device=0)  # Concat / padded pools: never the native guard, whatever the device
    assert not gd.native_forms and not gd._native_ok()
    assert RangeGuard(d.Circuit(c.layers[2:]), M7, mrs=True, device=0).native_forms
    # the batched outputs are the numpy ones, for a ceil-mode sum pool as well
    import torch

    c2, x2 = pools_circuit()
    c3 = d.Circuit([d.SumPool2d(6, 6, 2, 3, 3, 2, 2, ceil_mode=True)])
    for cc, xx in ((c, xs[:3]), (c2, x2), (c3, [np.arange(72) - 30, np.arange(72)[::-1] * 3])):
        bad, out = RangeGuard(cc, M7, mrs=True)._bad_batch(torch.tensor(np.stack(xx)), want_out=True)
        assert not bool(bad.any())
        np.testing.assert_array_equal(out.cpu().numpy(), np.stack([cc.plain_q_eval(x, False, M7) for x in xx]))


# ---------------------------------------------------------------- 8. zoo
def test_squeezenet_cifar_builds():
    from dash_amd.models import BENCH_CONFIGS, build_circuit, quantized_inputs

    cfg = BENCH_CONFIGS["SQUEEZENET_CIFAR/DASH"]
    c = build_circuit(cfg["model"], cfg["q_method"], cfg["q_parameter"], seed=0)
    kinds = [type(l).__name__ for l in c.layers]
    assert kinds.count("Concat") == 2 and kinds.count("MaxPool2d") == 2 and kinds[-2:] == ["SumPool2d", "Flatten"]
    assert all(l.ceil_mode for l in c.layers if isinstance(l, d.MaxPool2d))
    x = quantized_inputs(cfg["model"], 1, cfg["q_method"], cfg["q_parameter"], seed=7)[0]
    y = c.plain_q_eval(x)
    assert y.shape == (10,) and c.infer_crt_base_size([x]) <= cfg["crt"]
