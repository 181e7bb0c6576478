"""The HIP evaluator's plan, pinned: what HipEvaluator::build() (dash_amd/csrc/hip/runtime.hip) allocates, uploads
and lists as ops for the smallest circuits that reach each branch of the planner.

The other GPU suites compare output labels with the host evaluator; a planner that reorders ops, drops a `save` or
allocates a scratch twice can pass all of them. Here every case builds a fresh evaluator and compares, with exact
equality, against tests/golden/hip_plan_snapshot.json:
  * device_bytes() and table_bytes() right after construction and loading;
  * the sorted (layer, table, bytes per slot) triples of ipc_export() (streamed evaluators export nothing: null);
  * the op names of op_times() after one eager evaluate;
  * the launch log of that run.
The run's labels must equal GarbledCircuit.cpu_evaluate's, so a snapshot cannot come from a wrong run.

The fixture is written by scripts/record_hip_plan.py from this module's case table, on an MI355X, and carries the
commit whose dash_amd/csrc produced it ("recorded_from"); it is never re-recorded from the code under test.

Planning CU counts are forced to 1 or 1 << 20 (never the device's own), and the joint-fuse mode is set per case, so
the fixture does not depend on the part the test runs on. Circuits come from the other test modules where those
have builders and are garbled once per module.
"""
import functools
import json
import os
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_clip_joint as cjg  # noqa: E402
import test_gpu_grouped_conv as grp  # noqa: E402
import test_gpu_joint_fused as jf  # noqa: E402
import test_gpu_launch_forms as forms  # noqa: E402
from test_argmax import M7, argmax_inputs  # noqa: E402
from test_branching_graphs import fire_circuit, pools_circuit  # noqa: E402
from test_clip import clip_inputs  # noqa: E402
from test_garbled_layers import _shortcut_block  # noqa: E402
from test_gpu_parity import _dense_layer  # noqa: E402

FIXTURE = Path(__file__).resolve().parent / "golden" / "hip_plan_snapshot.json"
BIG = 1 << 20

# Every op-name suffix of the planner's add_op calls ("" is the bare "kind#index" of a one-op layer; an ArgMax's
# ".lvN" level infix is dropped), and its four unnumbered ops.
SUFFIXES = {"", ".A", ".B", ".C", ".H", ".mrs", ".lo.mrs", ".hi.mrs", ".lo.A", ".lo.B", ".hi.A", ".hi.B", ".clip_hi",
            ".out", ".hash", ".update", ".upd+A", ".be", ".post", ".gather", ".diff", ".add", ".idiff", ".iH", ".geom",
            ".zero", ".unpack", ".wait", "save", "restore", "stage", "stage_end"}
# The one permitted omission: ".wait" is the streamed joint Clip's wait for the Clip layer's window, a branch that
# has no GPU test yet.
UNCOVERED = {".wait"}
# Not in SUFFIXES: ".sA" / ".sB". The ReDash rescale loop names them for a plan with a sign base extension, but it
# builds its RescalePlan with sign_be = false (the legacy mode, the only one with sign_be, is planned by
# plan_rescale_legacy: ".upd+A" / ".B"), so no model can make the planner emit them.


# ------------------------------------------------------------------------------------------------------ circuits
def _garbled(circuit, crt, mrs, xs, fused=True, rescale="legacy", relu="approx", hardened=None, **kw):
    """test_gpu_parity._check's garbling: one GC per input, seed bytes([i + 1]) * 16, its default constructions."""
    gcs = [GarbledCircuit(circuit, crt, mrs, seed=bytes([i + 1]) * 16, fused_sign=fused, rescale=rescale, relu=relu,
                          hardened=hardened, **kw) for i in range(len(xs))]
    return dict(gcs=gcs, enc=[g.garble_inputs(x) for g, x in zip(gcs, xs)])


@functools.lru_cache(maxsize=None)
def _dense_relu(hardened):  # test_gpu_parity.test_dense_relu_encodings
    rng = np.random.default_rng(11)
    W1 = rng.integers(-8, 9, (24, 30)); b1 = rng.integers(-8, 9, 24)
    c = d.Circuit([d.Dense.from_quantized(W1, b1), d.Relu((24,)), d.Dense.from_quantized(W1[:6, :24], b1[:6])])
    return _garbled(c, 7, 100.0, [rng.integers(-20, 20, 30) for _ in range(2)], hardened=hardened)


@functools.lru_cache(maxsize=None)
def _dense_tf():  # "dense_tf" of test_gpu_garbler_bit_identical_all_kinds
    c = d.Circuit([_dense_layer(np.random.default_rng(11), 96, 33, channel_tf=3)])
    return _garbled(c, 8, 100.0, [np.random.default_rng(5).integers(-20, 20, 96)])


@functools.lru_cache(maxsize=None)
def _conv():  # test_gpu_parity.test_conv
    rng = np.random.default_rng(2)
    W = rng.integers(-5, 6, (8, 3, 3, 3)); b = rng.integers(-5, 6, 8)
    W2 = rng.integers(-5, 6, (4, 8, 2, 2)); b2 = rng.integers(-5, 6, 4)
    c = d.Circuit([d.Conv2d.from_quantized(W, b, 9, 9, 3, 8, 3, 3, 1, 1, pad_width=1, pad_height=1),
                   d.Conv2d.from_quantized(W2, b2, 9, 9, 8, 4, 2, 2, 2, 2)])
    return _garbled(c, 9, None, [rng.integers(-5, 6, 3 * 81) for _ in range(2)])


@functools.lru_cache(maxsize=None)
def _grouped(name):  # test_gpu_grouped_conv.test_grouped_conv_labels_match_host, base 7
    shape = grp.SHAPES[name]
    W, H, C = shape[:3]
    rng = np.random.default_rng(sum(shape))
    c = d.Circuit([grp._layer(rng, *shape)])
    return _garbled(c, 7, None, [rng.integers(-6, 7, C * H * W) for _ in range(2)])


@functools.lru_cache(maxsize=None)
def _sign_edges(fused):  # test_gpu_parity.test_sign_edges
    vals = [0, 1, -1, 55773217, -55773217, 111546434, -111546435]
    return _garbled(d.Circuit([d.Sign((len(vals),))]), 9, [76, 7, 7, 7, 7, 7, 5, 5], [vals, vals[::-1]], fused=fused)


@functools.lru_cache(maxsize=None)
def _relu_single_digit():  # test_gpu_parity.test_single_digit_mrs
    rng = np.random.default_rng(5)
    return _garbled(d.Circuit([d.Relu((64,))]), 8, 99.0, [rng.integers(-1000, 1000, 64) for _ in range(2)])


@functools.lru_cache(maxsize=None)
def _relu_mrs():  # test_gpu_parity.test_relu_mrs_sign, k = 7: 128 elements
    k = 7
    h = GarbledCircuit(d.Circuit([d.Relu((1,))]), k, None, garble_me=False).crt_modulus // 2
    vals = np.array([0, 1, -1, h - 1, -h, -h + 1, 2, -2] + list(np.random.default_rng(k).integers(-h, h, 120)),
                    dtype=np.int64)
    return _garbled(d.Circuit([d.Relu((len(vals),))]), k, None, [vals, vals[::-1].copy()], relu="mrs")


@functools.lru_cache(maxsize=None)
def _rescale_legacy(fused):  # test_gpu_parity.test_rescale_legacy
    rng = np.random.default_rng(3)
    xs = [rng.integers(-100000, 100000, 300) for _ in range(2)]
    return _garbled(d.Circuit([d.Rescale(2, (300,))]), 9, 100.0, xs, fused=fused)


@functools.lru_cache(maxsize=None)
def _rescale_mrs():  # test_gpu_parity.test_rescale_mrs, (7, 5)
    k, l = 7, 5
    c = d.Circuit([d.Rescale(l, (300,))])
    h = GarbledCircuit(c, k, 100.0, garble_me=False).crt_modulus // 2
    rng = np.random.default_rng(k + l)
    return _garbled(c, k, 100.0, [rng.integers(-h, h - (1 << l), 300) for _ in range(2)], rescale="mrs")


REDASH = {"p97_107": ([32, 97, 107], [22, 19, 15, 13]), "primes17": ([32, 3, 5, 7, 11, 13, 17], [10, 9, 9, 8, 7, 7, 6])}


@functools.lru_cache(maxsize=None)
def _rescale_redash(base):  # test_gpu_parity.test_rescale_redash
    rng = np.random.default_rng(4)
    xs = [rng.integers(-100000, 100000, 200) for _ in range(2)]
    return _garbled(d.Circuit([d.Rescale([32], (200,))]), *REDASH[base], xs)


@functools.lru_cache(maxsize=None)
def _joint_relu_kept():  # test_gpu_joint_fused.test_kept_rescale_output_is_not_fused
    k, N = 7, 528
    x, _ = forms._inputs("J", k, N)
    xs = [x, x[::-1].copy(), np.roll(x, 7)]
    circ = d.Circuit([d.Rescale(forms._shift("J", k), (N,)), d.Relu((N,)), d.Add((N,), 0)])
    gcs = [GarbledCircuit(circ, k, forms._mrs_arg(k), seed=bytes([k, i + 1]) * 8, rescale="mrs", relu="joint")
           for i in range(3)]
    return dict(gcs=gcs, enc=[g.garble_inputs(v) for g, v in zip(gcs, xs)])


@functools.lru_cache(maxsize=None)
def _clip(relu):  # test_gpu_clip.test_clip_layer, N = 75
    c = d.Circuit([d.Clip.from_quantized((75,), 0, 192)])
    gcs = [GarbledCircuit(c, 7, 100.0, seed=bytes([i + 1]) * 16, relu=relu) for i in range(2)]
    return dict(gcs=gcs, enc=[g.garble_inputs(x) for g, x in zip(gcs, clip_inputs(75, 0, 192, M7)[:2])])


@functools.lru_cache(maxsize=None)
def _joint_clip_kept():  # test_gpu_clip_joint.test_kept_rescale_output
    N, l, q_hi = 528, 5, 192
    circ = d.Circuit([d.Rescale(l, (N,)), d.Clip.from_quantized((N,), 0, q_hi), d.Add((N,), 0)])
    gcs = [GarbledCircuit(circ, 7, 100.0, seed=bytes([5, i + 1]) * 8, rescale="mrs", clip="joint") for i in range(3)]
    x = cjg._pair_inputs(gcs[0].crt_modulus, l, q_hi, N)
    return dict(gcs=gcs, enc=[g.garble_inputs(v) for g, v in zip(gcs, [x, x[::-1].copy(), np.roll(x, 7)])])


@functools.lru_cache(maxsize=None)
def _maxpool_add_sumpool():  # test_gpu_parity.test_maxpool_sumpool_add
    rng = np.random.default_rng(5)
    c = d.Circuit([d.MaxPool2d(6, 6, 2, 2, 2), d.Add((2, 3, 3), 0), d.SumPool2d(3, 3, 2, 3, 3)])
    return _garbled(c, 7, 100.0, [rng.integers(-50, 50, 72) for _ in range(2)])


@functools.lru_cache(maxsize=None)
def _branching(name):  # test_gpu_branching_graphs: padded max + sum pools; the fire module (in_src, Concat)
    c, xs = fire_circuit() if name == "fire" else pools_circuit()
    kw = dict(rescale="mrs", relu="joint", hardened=True) if name == "fire" else {}
    return _garbled(c, 7, 100.0, xs[:2], **kw)


@functools.lru_cache(maxsize=None)
def _shortcut():  # test_gpu_parity.test_projection_shortcut_in_src
    c, xs = _shortcut_block()
    return _garbled(c, c.infer_crt_base_size(xs), 100.0, xs[:2])


@functools.lru_cache(maxsize=None)
def _max9():
    rng = np.random.default_rng(9)
    return _garbled(d.Circuit([d.Max((9,))]), 7, 100.0, [rng.integers(-50, 50, 9) for _ in range(2)])


@functools.lru_cache(maxsize=None)
def _argmax(dims):  # test_gpu_argmax.test_argmax_layer
    c = d.Circuit([d.ArgMax(dims)])
    gcs = [GarbledCircuit(c, 7, 100.0, seed=bytes([i + 1]) * 16) for i in range(2)]
    return dict(gcs=gcs, enc=[g.garble_inputs(x) for g, x in zip(gcs, argmax_inputs(dims, M7, rounds=2))])


@functools.lru_cache(maxsize=None)
def _proj_mult(name):  # test_gpu_parity.test_projection_mult_mixed
    if name == "proj":
        c = d.Circuit([d.Projection((4,), [19], [91], lambda v: v), d.Projection((4,), [91], [19], lambda v: v % 19)])
        return _garbled(c, [19], None, [[0, 1, 5, 18]])
    if name == "mult":
        return _garbled(d.Circuit([d.MultLayer((4,))]), [19], None, [[2, -4, -1, -2]])
    return _garbled(d.Circuit([d.MixedModMultLayer((4,), smaller_modulus=2)]), [19], None, [[5, 1, -3, 0]])


@functools.lru_cache(maxsize=None)
def _base_ext():  # test_gpu_parity.test_base_extension
    x = np.random.default_rng(6).integers(0, 97 * 107, 20)
    g = GarbledCircuit(d.Circuit([d.BaseExtension((20,), [32])]), [32, 97, 107], [22, 19, 15, 13], seed=bytes(16))
    return dict(gcs=[g], enc=[g.garble_inputs(x)])


def _case(build, B=None, cus=1, fuse=-1, mfma=True, stream=False):
    return dict(build=build, B=B, cus=cus, fuse=fuse, mfma=mfma, stream=stream)


_J528 = functools.partial(forms._circuit, "J", 7, 528)  # Rescale(5) + joint ReLU, three GCs
_JC528 = functools.partial(cjg._pair, 7, 100.0, 5, 192, 528)  # Rescale(5) + joint Clip(0, 192), three GCs

CASES = {
    "dense_relu_hardened": _case(functools.partial(_dense_relu, True)),
    "dense_relu_reference": _case(functools.partial(_dense_relu, False), cus=BIG),
    "dense_channel_tf": _case(_dense_tf),
    "conv_mfma": _case(_conv),
    "conv_valu": _case(_conv, mfma=False),
    "conv_grouped": _case(functools.partial(_grouped, "cg4_fg6")),
    "conv_depthwise": _case(functools.partial(_grouped, "odd_width")),
    "sign_fused": _case(functools.partial(_sign_edges, True)),
    "sign_refcasts": _case(functools.partial(_sign_edges, False)),
    "relu_single_digit_mrs": _case(_relu_single_digit),
    "relu_mrs": _case(_relu_mrs, cus=BIG),
    "rescale_legacy_fused": _case(functools.partial(_rescale_legacy, True)),
    "rescale_legacy_refcasts": _case(functools.partial(_rescale_legacy, False), cus=BIG),
    "rescale_mrs": _case(_rescale_mrs, cus=BIG),
    "rescale_redash_p97_107": _case(functools.partial(_rescale_redash, "p97_107")),
    "rescale_redash_primes17": _case(functools.partial(_rescale_redash, "primes17")),
    "joint_relu_b2_auto": _case(_J528, B=2),  # deferred: one fused op
    "joint_relu_b3_auto": _case(_J528, B=3, cus=BIG),  # two kernels
    "joint_relu_b3_forced": _case(_J528, B=3, fuse=1),
    "joint_relu_kept": _case(_joint_relu_kept, fuse=1),
    "joint_relu_b2_streamed": _case(_J528, B=2, stream=True),
    "clip_approx": _case(functools.partial(_clip, "approx")),
    "clip_mrs": _case(functools.partial(_clip, "mrs")),
    "joint_clip_b1": _case(_JC528, B=1, cus=BIG),
    "joint_clip_b3_forced": _case(_JC528, B=3, fuse=1),  # the pending path
    "joint_clip_kept": _case(_joint_clip_kept, fuse=1),
    "maxpool_add_sumpool": _case(_maxpool_add_sumpool),
    "padded_pools": _case(functools.partial(_branching, "pools")),
    "fire_concat": _case(functools.partial(_branching, "fire")),
    "shortcut_in_src": _case(_shortcut),
    "max": _case(_max9),
    "argmax_3": _case(functools.partial(_argmax, (3,))),
    "argmax_5x7x11": _case(functools.partial(_argmax, (5, 7, 11))),
    "projection": _case(functools.partial(_proj_mult, "proj")),
    "mult": _case(functools.partial(_proj_mult, "mult")),
    "mixed_mod_mult": _case(functools.partial(_proj_mult, "mmult")),
    "base_extension": _case(_base_ext),
}


# ----------------------------------------------------------------------------------------------------- snapshot
def snapshot(native, name):
    """Plan and run case `name` on a fresh evaluator: the recorded fields (also the recorder's entry point)."""
    from dash_amd.runtime import HipEvaluator

    case = CASES[name]
    c = case["build"]()
    B = case["B"] or len(c["gcs"])
    gcs, enc = c["gcs"][:B], c["enc"][:B]
    base = native.hip_joint_fuse()
    native.hip_launch_log_take()
    native.hip_set_planning_cus(case["cus"])
    native.hip_set_joint_fuse(case["fuse"])
    try:
        ev = HipEvaluator([g.model for g in gcs], mfma=case["mfma"], profile=True, stream_tables=case["stream"])
        snap = dict(device_bytes=ev.device_bytes(), table_bytes=ev.table_bytes(), ipc=None)
        if not case["stream"]:
            snap["ipc"] = sorted([int(layer), table, int(nbytes)] for layer, table, nbytes, _ in ev.ipc_export())
        native.hip_launch_log(True)
        try:
            out = ev.evaluate(enc)
        finally:
            native.hip_launch_log(False)
        snap["launches"] = list(native.hip_launch_log_take())
        snap["ops"] = [n for n, _ in ev.op_times()]
    finally:
        native.hip_set_joint_fuse(base)
        native.hip_set_planning_cus(0)
    jf._same_labels([g.cpu_evaluate(e) for g, e in zip(gcs, enc)], out)
    return snap


def op_suffixes(ops):
    out = set()
    for n in ops:
        out.add(re.sub(r"\.lv\d+", "", n.split("#", 1)[1].lstrip("0123456789")) if "#" in n else n)
    return out


def _fixture():
    return json.loads(FIXTURE.read_text())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_plan_matches_the_recorded_one(native, name):
    want = _fixture()["cases"][name]
    got = snapshot(native, name)
    for field in ("device_bytes", "table_bytes", "ipc", "ops", "launches"):
        assert got[field] == want[field], field
    assert set(got) == set(want)


def test_fixture_covers_every_op_suffix():
    """Every op name the planner can emit occurs in some recorded case, except UNCOVERED; needs no device."""
    fx = _fixture()
    assert set(fx["cases"]) == set(CASES) and re.fullmatch(r"[0-9a-f]{40}", fx["recorded_from"])
    seen = set()
    for snap in fx["cases"].values():
        seen |= op_suffixes(snap["ops"])
    assert seen <= SUFFIXES, seen - SUFFIXES
    assert SUFFIXES - seen == UNCOVERED, SUFFIXES - seen
