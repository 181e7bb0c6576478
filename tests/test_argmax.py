"""The ArgMax layer on the host: semantics, the garbled tournament of csrc/gadgets.h ArgMaxPlan through the host
garbler and evaluator, table sizes, the wire format, refusals, ONNX import and export, the range guard and the
zoo model (docs/ARGMAX.md).

The helpers below (inputs, circuits) are shared with tests/test_gpu_argmax.py.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit, RangeGuard, RangeGuardError
from dash_amd.ir.bases import crt_modulus, first_primes
from dash_amd.ir.quant import QuantizationMethod as Q
from dash_amd.native import native
from tests.test_clip import _conv_attrs, _f32, _onnx_model

M7 = crt_modulus(first_primes(7))
SEED = bytes(range(16))
GOLDEN = Path(__file__).resolve().parent / "golden" / "dense_rescale_relu_maxpool_v5.bin"
# positions whose pair operations are the first / last lanes of a wave and of a 512 tile (level 0: e = o)
BOUNDARY_AT = (0, 63, 64, 255, 256, 511, 512, -1)


# ---------------------------------------------------------------- shared helpers
def span_max(M: int) -> int:
    return min(M // 2, M - M // 2 - 1)


def argmax_inputs(dims, M: int, rounds: int = 2, seed: int = 1) -> list:
    """`rounds` input vectors for ArgMax(dims). Random values of a narrow band (so that equal maxima happen by
    chance too); on the positions BOUNDARY_AT, in turn: all candidates equal, a tie of the maximum at the first
    two, at two middle and at the last two indices, and the extreme span (minimum and maximum span_max apart)
    with the maximum first and with it last."""
    K, P = int(dims[0]), int(np.prod(dims[1:], dtype=np.int64))
    rng = np.random.default_rng(seed)
    sm = span_max(M)
    lo = -(sm // 2)
    band = max(2, min(40, sm // 2))
    out = []
    for r in range(rounds):
        v = rng.integers(-band, band, (K, P))
        for n, o in enumerate(sorted({i % P for i in BOUNDARY_AT if -P <= i < P})):
            case, col = (n + r) % 6, v[:, o]
            top = int(col.max()) + 3
            if case == 0:
                col[:] = 7
            elif case == 1:
                col[[0, min(1, K - 1)]] = top
            elif case == 2:
                col[[K // 2, max(K // 2 - 1, 0)]] = top
            elif case == 3:
                col[[K - 1, max(K - 2, 0)]] = top
            elif case == 4:
                col[:] = rng.integers(lo + 1, lo + sm, K)
                col[0], col[K - 1] = lo + sm, lo
            else:
                col[:] = rng.integers(lo + 1, lo + sm, K)
                col[0], col[K - 1] = lo, lo + sm
        out.append(v.reshape(-1))
    return out


def dense_argmax(rng, K: int = 10, n_in: int = 12):
    return d.Circuit([d.Dense.from_quantized(rng.integers(-4, 5, (K, n_in)), rng.integers(-6, 6, K)), d.ArgMax((K,))])


def _host_eval(gc, x):
    return gc.decode_outputs(gc.cpu_evaluate(gc.garble_inputs(x)))


def _entries(a) -> int:
    """16-byte table entries of a layer array."""
    return int(np.asarray(a).nbytes // 16)


def _gc(dims, crt=7, mrs=100.0, **kw):
    return GarbledCircuit(d.Circuit([d.ArgMax(dims)]), crt, mrs, seed=SEED, **kw)


# ---------------------------------------------------------------- 1. semantics
@pytest.mark.parametrize("dims", [(2,), (3,), (5,), (10,), (5, 3, 2)])
def test_semantics(dims):
    a = d.ArgMax(dims)
    assert (a.kind, a.name, d.ArgMax.kind) == (16, "argmax", 16)
    assert a.out_dims == (1,) + tuple(dims[1:]) and a.garble_spec() == (16, {"K": dims[0], "P": a.out_size})
    K = dims[0]
    for x in argmax_inputs(dims, M7, rounds=6):
        y = a.plain_q_eval(x, track=False)
        assert y.dtype == np.int64
        np.testing.assert_array_equal(y, np.argmax(x.reshape(K, -1), axis=0))
        f = a.plain_eval(x.astype(np.float32), track=False)
        assert f.dtype == np.float32
        np.testing.assert_array_equal(f, y.astype(np.float32))
    # ties go to the lowest index: first, middle, last, all equal; negative values; a span of exactly span_max
    P = a.out_size
    for vals, want in (([5] * K, 0), ([9, 9] + [1] * (K - 2), 0), ([1] * (K - 2) + [9, 9], K - 2),
                       ([-3] * K, 0), ([-9] * (K - 1) + [-2], K - 1)):
        x = np.repeat(np.asarray(vals[:K]), P)
        np.testing.assert_array_equal(a.plain_q_eval(x, track=False), np.full(P, want))
    if K >= 3:
        x = np.repeat(np.asarray([0] + [4] * 2 + [0] * (K - 3)), P)
        np.testing.assert_array_equal(a.plain_q_eval(x, track=False), np.full(P, 1))
    sm = span_max(M7)
    x = np.repeat(np.asarray([-(sm // 2)] * (K - 1) + [-(sm // 2) + sm]), P)
    np.testing.assert_array_equal(a.plain_q_eval(x, track=False), np.full(P, K - 1))


def test_range_tracking_sizes_the_differences():
    a = d.ArgMax((3, 1, 2))
    a.plain_q_eval(np.array([10, -50, 700, 0, -20, 90]))
    # position 0: 10, 700, -20 (span 720), position 1: -50, 0, 90 (span 140); outputs 1 and 2
    assert a.get_max_plain_q_val() == 720 and a.get_min_plain_q_val() == -720
    k = d.Circuit([d.ArgMax((2,))]).infer_crt_base_size([np.array([-7000, 7000])])
    assert crt_modulus(first_primes(k)) // 2 >= 14000 > crt_modulus(first_primes(k - 1)) // 2


# ---------------------------------------------------------------- 2. garbled end to end on the host
@pytest.mark.parametrize("dims", [(2,), (3,), (5,), (10,), (5, 3, 2)])
def test_garbled_single_layer(dims):
    gc = _gc(dims)
    assert gc.hardened
    for x in argmax_inputs(dims, M7, rounds=6):
        np.testing.assert_array_equal(_host_eval(gc, x), gc.plain_q_eval(x))
        np.testing.assert_array_equal(gc.plain_q_eval(x), np.argmax(x.reshape(dims[0], -1), axis=0))


def test_garbled_span_max():
    sm = span_max(M7)
    gc = _gc((3,))
    for x in ([-(sm // 2), 0, -(sm // 2) + sm], [-(sm // 2) + sm, 5, -(sm // 2)], [-(sm // 2) + sm, -(sm // 2) + sm, 0]):
        x = np.asarray(x)
        np.testing.assert_array_equal(_host_eval(gc, x), [int(np.argmax(x))])


def test_garbled_dense_argmax():
    rng = np.random.default_rng(3)
    gc = GarbledCircuit(dense_argmax(rng), 7, 100.0, seed=SEED)
    for _ in range(4):
        x = rng.integers(-20, 21, 12)
        np.testing.assert_array_equal(_host_eval(gc, x), gc.plain_q_eval(x))


def test_garbled_is_not_the_last_layer():
    """The output is an ordinary CRT label tensor: a dense layer reads it."""
    rng = np.random.default_rng(4)
    c = d.Circuit([d.ArgMax((5, 2, 2)), d.Flatten((1, 2, 2)), d.Dense.from_quantized(rng.integers(-4, 5, (3, 4)), [1, 2, 3])])
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED)
    for x in argmax_inputs((5, 2, 2), M7):
        np.testing.assert_array_equal(_host_eval(gc, x), gc.plain_q_eval(x))


def test_garbled_large_residue():
    """The base [2, 131] (M = 262): labels through the host evaluator and the decode."""
    gc = _gc((3, 5, 5), [2, 131], None)
    for x in argmax_inputs((3, 5, 5), 262, rounds=4):
        np.testing.assert_array_equal(_host_eval(gc, x), np.argmax(x.reshape(3, -1), axis=0))


# ---------------------------------------------------------------- 3. table sizes
def test_entry_counts():
    """gadgets.h ArgMaxPlan: 240 / 305 / 226 / 161 entries per pair operation at k = 7, so 161, 466 and 2341
    entries per output for K = 2, 3 and 10."""
    crt = first_primes(7)
    k, P = len(crt), sum(crt)
    n_sign = sum(crt[i + 1] * (k - 1 - i) for i in range(k - 1))
    assert (n_sign, P) == (147, 58)
    rows = (n_sign + P + 3 * k + 2 * k, n_sign + 2 * (P + 3 * k), n_sign + P + 3 * k, n_sign + 2 * k)
    assert rows == (240, 305, 226, 161)
    n = native()
    assert n.argmax_op_entries(crt, 2) == [(1, 161)]
    assert n.argmax_op_entries(crt, 3) == [(1, 240), (1, 226)]
    assert n.argmax_op_entries(crt, 10) == [(5, 240), (2, 305), (1, 305), (1, 226)]
    for K, want in ((2, 161), (3, 466), (10, 2341)):
        assert n.argmax_entries(crt, K) == want
        for dims in ((K,), (K, 3, 2)):
            gc = _gc(dims)
            pos = int(np.prod(dims[1:], dtype=np.int64))
            assert gc.table_bytes == 16 * pos * want
            assert sum(_entries(a) for a in gc.model.layer_arrays(0).values()) == pos * want


def test_array_shapes_and_no_value_gates_at_the_root():
    gc = _gc((10, 1, 3))
    arrs = gc.model.layer_arrays(0)
    assert list(gc.model.layer_params(0)["levels"]) == [4]
    want = set()
    for lv, (ops, root) in enumerate(((5, False), (2, False), (1, False), (1, True))):
        pre = f"lv{lv}."
        want |= {pre + "mrs"} | (set() if root else {pre + "mm.g", pre + "mm.e"})
        want |= {pre + "idx"} if lv == 0 else {pre + "im.g", pre + "im.e"}
    assert set(arrs) == want
    assert not any(name.startswith("lv3.mm.") for name in arrs)
    one = _gc((2,))
    assert set(one.model.layer_arrays(0)) == {"lv0.mrs", "lv0.idx"}


# ---------------------------------------------------------------- 4. wire format
def test_serialize_roundtrip():
    rng = np.random.default_rng(7)
    gc = GarbledCircuit(dense_argmax(rng), 7, 100.0, seed=SEED)
    blob = gc.model.serialize()
    back = native().GarbledModel.deserialize(blob)
    assert bytes(back.serialize()) == bytes(blob)
    assert [native().kind_name(16)] == ["argmax"]
    x = rng.integers(-20, 21, 12)
    enc = gc.garble_inputs(x)
    a, b = gc.cpu_evaluate(enc), native().cpu_evaluate(back, enc, 0)
    for (pa, la), (pb, lb) in zip(a, b):
        assert pa == pb
        np.testing.assert_array_equal(la, lb)
    np.testing.assert_array_equal(gc.decode_outputs(b), gc.plain_q_eval(x))


def parent_circuit():
    """Dense 10 -> 12, Rescale(3), ReLU, MaxPool 2x2 over (3, 2, 2): calibrated for the flagship constructions."""
    rng = np.random.default_rng(11)
    c = d.Circuit([d.Dense.from_quantized(rng.integers(-4, 5, (12, 10)), rng.integers(-6, 6, 12)), d.Rescale(3, (12,)),
                   d.Relu((12,)), d.MaxPool2d(2, 2, 3, 2, 2)])
    xs = [rng.integers(-20, 21, 10) for _ in range(3)]
    c.calibrate(xs, M7)
    return c, xs


def test_circuits_without_argmax_keep_their_bytes():
    """The golden file is the offline message of parent_circuit() (k = 7, garbler seed 0..15, rescale="mrs",
    relu="joint"), written by the commit before the ArgMax layer: it is reproduced byte for byte, loads and
    evaluates."""
    c, xs = parent_circuit()
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED, rescale="mrs", relu="joint")
    old = GOLDEN.read_bytes()
    assert bytes(gc.model.serialize()) == old
    back = native().GarbledModel.deserialize(old)
    out = native().cpu_evaluate(back, gc.garble_inputs(xs[0]), 0)
    np.testing.assert_array_equal(gc.decode_outputs(out), gc.plain_q_eval(xs[0]))


# ---------------------------------------------------------------- 5. refusals
def test_refusals():
    c = d.Circuit([d.Flatten((4,)), d.ArgMax((4,))])
    with pytest.raises(ValueError, match=r"layer 1 \(argmax\).*hardened"):
        GarbledCircuit(c, 7, 100.0, seed=SEED, hardened=False)
    with pytest.raises(ValueError, match=r"layer 1 \(argmax\).*hardened"):
        GarbledCircuit(c, 7, 100.0, seed=SEED, fused_sign=False)  # the reference casts cannot be hardened
    c2 = d.Circuit([d.Rescale(2, (4,)), d.ArgMax((4,))])
    with pytest.raises(ValueError, match=r"layer 1 \(argmax\).*hardened"):
        GarbledCircuit(c2, 7, 100.0, seed=SEED, rescale="legacy")
    with pytest.raises(ValueError, match=r"layer 1 \(argmax\).*residue 0 = 2"):
        GarbledCircuit(c, [3, 5, 7], None, seed=SEED)
    with pytest.raises(ValueError, match=r"layer 1 \(argmax\).*residue 0 = 2"):
        GarbledCircuit(c, [2, 4, 7], None, seed=SEED)  # an even residue beside the 2
    for dims in ((1,), (1, 4, 4), (4, 4)):
        with pytest.raises(ValueError, match="argmax"):
            d.ArgMax(dims)
    with pytest.raises(Exception, match="argmax"):
        native().argmax_entries(first_primes(7), 1)


# ---------------------------------------------------------------- 6. ONNX
def _argmax_node(src, out, **attrs):
    from dash_amd.ir import onnx as o

    return o._node("ArgMax", [src], [out], "head", b"".join(o._attr_int(k, v) for k, v in attrs.items()))


def _gemm_model(tmp_path, rng, tail, out_dims):
    from dash_amd.ir import onnx as o

    w, b = _f32(rng, 5, 12), _f32(rng, 5)
    gemm = o._attr_float("alpha", 1.0) + o._attr_float("beta", 1.0) + o._attr_int("transB", 1)
    nodes = [o._node("Gemm", ["input", "w", "b"], ["g"], "fc", gemm), tail]
    return _onnx_model(tmp_path / "m.onnx", nodes, {"w": w, "b": b}, (1, 12), "out", out_dims), w, b


@pytest.mark.parametrize("axis", [1, -1])
@pytest.mark.parametrize("keepdims", [0, 1, None])
def test_onnx_argmax_of_logits(tmp_path, axis, keepdims):
    from dash_amd.ir.onnx import load_onnx_model

    rng = np.random.default_rng(31)
    attrs = dict(axis=axis) if keepdims is None else dict(axis=axis, keepdims=keepdims)
    path, w, b = _gemm_model(tmp_path, rng, _argmax_node("g", "out", **attrs), (1, 1) if keepdims != 0 else (1,))
    c = load_onnx_model(path, Q.ScaleQuant, 10)
    assert [l.name for l in c.layers] == ["dense", "rescale", "argmax"] and c.output_dims == (1,)
    for _ in range(8):
        x = _f32(rng, 12) * 4
        np.testing.assert_array_equal(c.plain_eval(x, track=False), [np.argmax(w @ x + b)])


@pytest.mark.parametrize("axis", [1, -3])
@pytest.mark.parametrize("keepdims", [0, 1])
def test_onnx_argmax_over_channels(tmp_path, axis, keepdims):
    from dash_amd.ir import onnx as o
    from dash_amd.ir.onnx import load_onnx_model

    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(32)
    w, b = _f32(rng, 4, 3, 3, 3), _f32(rng, 4)
    nodes = [o._node("Conv", ["input", "w", "b"], ["c"], "conv", _conv_attrs(3, 1, 1)),
             _argmax_node("c", "out", axis=axis, keepdims=keepdims)]
    path = _onnx_model(tmp_path / "seg.onnx", nodes, {"w": w, "b": b}, (1, 3, 6, 6), "out",
                       (1, 1, 6, 6) if keepdims else (1, 6, 6))
    c = load_onnx_model(path, Q.ScaleQuant, 10)
    assert [l.name for l in c.layers] == ["conv2d", "rescale", "argmax"] and c.output_dims == (1, 6, 6)
    for _ in range(4):
        x = _f32(rng, 3, 6, 6) * 4
        ref = torch.nn.functional.conv2d(torch.tensor(x)[None], torch.tensor(w), torch.tensor(b), padding=1)[0]
        np.testing.assert_array_equal(c.plain_eval(x.reshape(-1), track=False), ref.argmax(dim=0).numpy().reshape(-1))


def test_onnx_refusals(tmp_path):
    from dash_amd.ir.onnx import load_onnx_model

    rng = np.random.default_rng(33)
    for attrs, what in ((dict(axis=1, select_last_index=1), "select_last_index"), (dict(axis=0), "axis 0"),
                        (dict(), "axis 0"), (dict(axis=2), "axis 2"), (dict(axis=-2), "axis -2")):
        path, _, _ = _gemm_model(tmp_path, rng, _argmax_node("g", "out", **attrs), (1, 1))
        with pytest.raises(NotImplementedError, match=f"head.*{what}"):
            load_onnx_model(path, Q.ScaleQuant, 10)


@pytest.mark.parametrize("scheme,param", [(Q.ScaleQuant, 5), (Q.SimpleQuant, -1), (Q.ScaleQuantPlus, 32)])
def test_onnx_export_import_roundtrip(tmp_path, scheme, param):
    from dash_amd.ir.onnx import load_onnx_model, parse_onnx, save_onnx_model
    from dash_amd.models import build_circuit, quantized_inputs

    c = build_circuit("MODEL_A_ARGMAX", scheme, param, seed=0)
    save_onnx_model(tmp_path / "a.onnx", c)
    heads = [n for n in parse_onnx(tmp_path / "a.onnx")["nodes"] if n["op_type"] == "ArgMax"]
    assert len(heads) == 1 and int(heads[0]["attrs"]["axis"]) == 1
    back = load_onnx_model(tmp_path / "a.onnx", scheme, param)
    assert [l.name for l in back.layers] == [l.name for l in c.layers]
    for x in quantized_inputs("MODEL_A", 3, scheme, param, seed=1):
        np.testing.assert_array_equal(back.plain_q_eval(x, False), c.plain_q_eval(x, False))


# ---------------------------------------------------------------- 7. range guard
def guard_case(M: int = M7):
    """ArgMax((3, 1, 2)) and three inputs: a span of exactly span_max() at both positions, span_max() + 1 at the
    first, and at the second."""
    c = d.Circuit([d.ArgMax((3, 1, 2))])
    sm = span_max(M)
    lo = -(sm // 2)
    ok = np.array([lo, lo + sm, 0, 3, lo + sm, lo])
    a, b = ok.copy(), ok.copy()
    a[0] -= 1  # position 0: lo - 1 .. lo + sm
    b[1] += 1  # position 1: lo .. lo + sm + 1
    return c, [ok, a, b], [False, True, True]


def test_range_guard_span():
    pytest.importorskip("torch")
    c, xs, want = guard_case()
    g = RangeGuard(c, M7, mrs=True, device=None)
    assert g.span_max() == span_max(M7)
    assert g.batched and not g.native_forms and not g._native_ok()
    assert [bool(g.violations_np(x)) for x in xs] == want
    assert g.submit(xs).bad_indices() == [i for i, w in enumerate(want) if w]  # the torch path, CPU device
    with pytest.raises(RangeGuardError):
        g.check(xs)
    g.check(xs[:1])
    # range_guard="auto" stays as it is (the mixed-radix rescale's and the Clip's rule); "on" refuses
    assert not GarbledCircuit(c, 7, 100.0, seed=SEED).guard_enabled
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED, range_guard="on")
    np.testing.assert_array_equal(_host_eval(gc, xs[0]), gc.plain_q_eval(xs[0]))
    for x in xs[1:]:
        with pytest.raises(RangeGuardError):
            gc.garble_inputs(x)


# ---------------------------------------------------------------- 8. zoo
def model_a_argmax():
    from dash_amd.models import BENCH_CONFIGS, build_circuit, quantized_inputs

    cfg = BENCH_CONFIGS["MODEL_A_ARGMAX/SIMPLE"]
    assert (cfg["model"], cfg["q_method"], cfg["crt"]) == ("MODEL_A_ARGMAX", Q.SimpleQuant, 8)
    c = build_circuit(cfg["model"], cfg["q_method"], cfg["q_parameter"], seed=0)
    logits = build_circuit("MODEL_A", cfg["q_method"], cfg["q_parameter"], seed=0)
    xs = quantized_inputs("MODEL_A", 3, cfg["q_method"], cfg["q_parameter"], seed=1)
    return cfg, c, logits, xs


def test_zoo_model_a_argmax():
    cfg, c, logits, xs = model_a_argmax()
    assert [l.name for l in c.layers][:-1] == [l.name for l in logits.layers] and c.layers[-1].name == "argmax"
    assert c.output_dims == (1,)
    gc = GarbledCircuit(c, cfg["crt"], cfg["mrs"], seed=SEED)
    for x in xs:
        want = [int(np.argmax(logits.plain_q_eval(x, False)))]
        np.testing.assert_array_equal(gc.plain_q_eval(x), want)
        np.testing.assert_array_equal(_host_eval(gc, x), want)


def test_trainer_refuses_a_trailing_argmax():
    pytest.importorskip("torch")
    from dash_amd.models.train import build_torch_model

    with pytest.raises(NotImplementedError, match="MODEL_A_ARGMAX.*argmax"):
        build_torch_model("MODEL_A_ARGMAX")
