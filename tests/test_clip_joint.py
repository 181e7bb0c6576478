"""The joint Clip construction on the host (docs/CLIP.md, csrc/gadgets.h ClipPlan joint variant): a Clip(0, q_hi)
directly behind a mixed-radix Rescale(l) takes its lower sign from that rescale's conversion and its upper sign
from one exact sign of the rescale's input against t_hi = (q_hi - 1) S + 1.

The helpers (the pair circuit, its domain and inputs) are shared with tests/test_gpu_clip_joint.py.
"""
from __future__ import annotations

import os
import sys
from pathlib import Path

import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit, RangeGuard, RangeGuardError
from dash_amd.ir.bases import crt_modulus, first_primes
from dash_amd.native import native

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_clip as tc  # noqa: E402  (the cut-down MobileNet)

SEED = bytes(range(16))
M7 = crt_modulus(first_primes(7))
GOLDEN = Path(__file__).resolve().parent / "golden" / "rescale_clip_separate_v4.bin"
# (crt, mrs, l, q_hi): k = 7 with both bounds of the issue, and the base [2, 131] (label bytes above 127)
PAIRS = {"k7_192": (7, 100.0, 5, 192), "k7_6": (7, 100.0, 5, 6), "p131": ([2, 131], None, 2, 6)}


# ---------------------------------------------------------------- shared helpers
def pair_circuit(N: int, l: int, q_hi: int, q_lo: int = 0):
    return d.Circuit([d.Rescale(l, (N,)), d.Clip.from_quantized((N,), q_lo, q_hi)])


def pair_domain(M: int, l: int, q_hi: int):
    """(t_lo, t_hi, lo, hi_exclusive): the two thresholds on the rescale's input x (y >= 0 from -S + 1, y >= q_hi
    from t_hi) and the joint construction's domain [-M/2 + t_hi, mrs_limit(M))."""
    S = 1 << l
    t_hi = (q_hi - 1) * S + 1
    return -S + 1, t_hi, -(M // 2) + t_hi, d.Rescale(l, (1,)).mrs_limit(M)


def closed_form(x, l: int, q_hi: int):
    return np.minimum(np.maximum(-((-np.asarray(x)) // (1 << l)), 0), q_hi)


def pair_values(M: int, l: int, q_hi: int) -> list:
    t_lo, t_hi, lo, hi = pair_domain(M, l, q_hi)
    vals = [t + o for t in (t_lo, t_hi) for o in range(-3, 4)] + [lo, lo + 1, hi - 1, hi - 2]
    return [v for v in vals if lo <= v < hi]


def pair_inputs(N: int, M: int, l: int, q_hi: int, seed: int = 1):
    """One input vector: random over the domain, every value of pair_values() from index 0 on (N permitting)."""
    _, _, lo, hi = pair_domain(M, l, q_hi)
    x = np.random.default_rng(seed).integers(lo, hi, N).astype(np.int64)
    v = pair_values(M, l, q_hi)[:N]
    x[:len(v)] = v
    return x


def _host_eval(gc, x):
    return gc.decode_outputs(gc.cpu_evaluate(gc.garble_inputs(x)))


def _layer_bytes(gc, i: int) -> int:
    return sum(a.nbytes for a in gc.model.layer_arrays(i).values())


def _blob(gc) -> bytes:
    return bytes(gc.model.serialize())


# ---------------------------------------------------------------- 1. the construction, end to end
@pytest.mark.parametrize("case", list(PAIRS))
def test_pair_decodes_to_the_closed_form(case):
    crt, mrs, l, q_hi = PAIRS[case]
    N = 40
    gc = GarbledCircuit(pair_circuit(N, l, q_hi), crt, mrs, seed=SEED, rescale="mrs", clip="joint")
    M = gc.crt_modulus
    assert gc.clip == "joint" and gc.joint_clips == {1: (q_hi - 1) * (1 << l) + 1} and gc.hardened
    assert native().clip_joint_threshold(gc.crt_base, l, q_hi) == pair_domain(M, l, q_hi)[1]
    p = gc.model.layer_params(1)
    assert list(p["smode"]) == [2] and list(p["t_hi"]) == [gc.joint_clips[1]]
    assert list(gc.model.layer_params(0)["sign_out"]) == [1]
    seen = set()
    for seed in range(3):
        x = pair_inputs(N, M, l, q_hi, seed)
        seen.update(int(v) for v in x)
        want = closed_form(x, l, q_hi)
        np.testing.assert_array_equal(gc.plain_q_eval(x), want)
        np.testing.assert_array_equal(_host_eval(gc, x), want)
    assert set(pair_values(M, l, q_hi)) <= seen and len(pair_values(M, l, q_hi)) >= 14
    # both branches of both signs ran
    assert {0, q_hi} <= set(int(v) for v in closed_form(sorted(seen), l, q_hi)) and len(seen) > 20


def test_entries_per_element_and_arrays():
    """n_sign + P + 5 k entries per element from the model's arrays (240 at k = 7, against 387), no lo.* array."""
    crt, N = first_primes(7), 10
    k, P = len(crt), sum(crt)
    n_sign = sum(crt[i + 1] * (k - 1 - i) for i in range(k - 1))
    gc = GarbledCircuit(pair_circuit(N, 5, 192), 7, 100.0, seed=SEED, rescale="mrs", clip="joint")
    arrays = gc.model.layer_arrays(1)
    assert set(arrays) == {"hi.mrs", "mm.g", "mm.e", "cap"} and not any(a.startswith("lo.") for a in arrays)
    entries = sum(a.nbytes // 16 for a in arrays.values())  # 128-bit entries
    assert entries == N * (n_sign + P + 5 * k) == N * 240 and n_sign == 147 and P == 58
    sep = GarbledCircuit(pair_circuit(N, 5, 192), 7, 100.0, seed=SEED, rescale="mrs", clip="separate")
    # the Clip layer itself shrinks by one sign gadget; the rescale's sign_last order has rows of its own size
    assert _layer_bytes(sep, 1) - _layer_bytes(gc, 1) == 16 * N * n_sign and _layer_bytes(sep, 1) == 16 * N * 387
    assert set(sep.model.layer_arrays(1)) == {"lo.mrs", "hi.mrs", "mm.g", "mm.e", "cap"}


# ---------------------------------------------------------------- 2. Clips that cannot be joint; the default
def _not_joint_circuits():
    N = 12
    yield "q_lo != 0", d.Circuit([d.Rescale(3, (N,)), d.Clip.from_quantized((N,), -10, 25)]), 7
    yield "no rescale", d.Circuit([d.Clip.from_quantized((N,), 0, 192)]), 7
    add = d.Circuit([d.Rescale(3, (N,)), d.Relu((N,)), d.Clip.from_quantized((N,), 0, 25)])
    yield "not directly behind", add, 7
    src = d.Circuit([d.Rescale(3, (N,)), d.Rescale(3, (N,)), d.Clip.from_quantized((N,), 0, 25)])
    src.layers[2].in_src = 0
    yield "in_src", src, 7
    yield "redash rescale", d.Circuit([d.Rescale([3], (N,)), d.Clip.from_quantized((N,), 0, 25)]), [2, 3, 5, 7, 11]


@pytest.mark.parametrize("name", ["q_lo != 0", "no rescale", "not directly behind", "in_src", "redash rescale"])
def test_clips_that_cannot_be_joint_keep_their_bytes(name):
    c, crt = next((c, crt) for n, c, crt in _not_joint_circuits() if n == name)
    mrs = 100.0 if crt == 7 else None
    kw = dict(seed=SEED, rescale="mrs", relu="mrs")
    joint = GarbledCircuit(c, crt, mrs, clip="joint", **kw)
    sep = GarbledCircuit(c, crt, mrs, clip="separate", **kw)
    assert joint.clip == "separate" and not joint.joint_clips
    assert _blob(joint) == _blob(sep)
    assert "clip" not in joint.effective_constructions()
    clip_at = [i for i, l in enumerate(c.layers) if l.name == "clip"][0]
    assert list(joint.model.layer_params(clip_at)["smode"]) == [1]


def test_default_is_separate_and_the_parent_blob_still_loads(monkeypatch):
    """The golden file is the offline message of Rescale(5) + Clip(0, 192), N = 6, k = 7, garbler seed 0..15,
    flagship constructions, written by the commit before the joint construction: the default and
    clip="separate" reproduce it byte for byte, and it loads and evaluates unchanged."""
    monkeypatch.delenv("DASH_CLIP", raising=False)
    c = pair_circuit(6, 5, 192)
    kw = dict(seed=SEED, rescale="mrs", relu="joint")
    dflt, sep = GarbledCircuit(c, 7, 100.0, **kw), GarbledCircuit(c, 7, 100.0, clip="separate", **kw)
    old = GOLDEN.read_bytes()
    assert _blob(dflt) == _blob(sep) == old
    assert dflt.clip == "separate" and "clip" not in dflt.effective_constructions()
    back = native().GarbledModel.deserialize(old)
    assert list(back.layer_params(1)["smode"]) == [1]
    x = pair_inputs(6, M7, 5, 192)
    out = native().cpu_evaluate(back, dflt.garble_inputs(x), 0)
    np.testing.assert_array_equal(dflt.decode_outputs(out), closed_form(x, 5, 192))
    assert _blob(GarbledCircuit(c, 7, 100.0, clip="joint", **kw)) != old


def test_effective_constructions():
    N = 8
    one = GarbledCircuit(pair_circuit(N, 5, 192), 7, 100.0, seed=SEED, rescale="mrs", clip="joint")
    assert one.effective_constructions() == dict(sign="fused", rescale="mrs", relu="none", encoding="hardened",
                                                 clip="joint")
    mixed = d.Circuit([d.Rescale(5, (N,)), d.Clip.from_quantized((N,), 0, 192), d.Rescale(1, (N,)),
                       d.Clip.from_quantized((N,), -3, 40), d.Rescale(1, (N,)), d.Clip.from_quantized((N,), 0, 9)])
    gc = GarbledCircuit(mixed, 7, 100.0, seed=SEED, rescale="mrs", clip="joint")
    assert gc.effective_constructions()["clip"] == "joint(2)+separate(1)" and sorted(gc.joint_clips) == [1, 5]
    x = np.random.default_rng(4).integers(-30000, 30000, N)
    np.testing.assert_array_equal(_host_eval(gc, x), gc.plain_q_eval(x))
    sep = GarbledCircuit(mixed, 7, 100.0, seed=SEED, rescale="mrs", clip="separate")
    assert sep.effective_constructions() == dict(sign="fused", rescale="mrs", relu="none", encoding="hardened")


# ---------------------------------------------------------------- 3. refusals and the environment knob
def test_refusals_name_the_layer(monkeypatch):
    monkeypatch.delenv("DASH_CLIP", raising=False)
    c = pair_circuit(5, 5, 192)
    with pytest.raises(ValueError, match="clip construction must be"):
        GarbledCircuit(c, 7, 100.0, seed=SEED, rescale="mrs", clip="both")
    # a legacy DASH rescale cannot be hardened, so the Clip itself is refused, by its layer
    with pytest.raises(ValueError, match=r"layer 1 \(clip\)"):
        GarbledCircuit(c, 7, 100.0, seed=SEED, rescale="legacy", clip="joint")
    # no DASH rescale at all: "auto" resolves to "legacy", which cannot carry the joint construction
    with pytest.raises(ValueError, match=r"clip='joint': layer 0 \(clip\).*rescale='mrs'"):
        GarbledCircuit(d.Circuit([d.Clip.from_quantized((5,), 0, 192)]), 7, 100.0, seed=SEED, clip="joint")
    with pytest.raises(ValueError, match=r"layer 1 \(clip\).*hardened"):
        GarbledCircuit(c, 7, 100.0, seed=SEED, rescale="mrs", hardened=False, clip="joint")
    # a tracked rescale input below -M/2 + t_hi
    _, t_hi, lo, _ = pair_domain(M7, 5, 192)
    low = pair_circuit(5, 5, 192)
    low.calibrate([np.array([lo - 1, 0, 1, 2, 3])], M7)
    with pytest.raises(ValueError, match=r"clip='joint': layer 1 \(clip\).*layer 0's tracked input reaches %d < %d" % (
            lo - 1, lo)):
        GarbledCircuit(low, 7, 100.0, seed=SEED, rescale="mrs", clip="joint")
    ok = pair_circuit(5, 5, 192)
    ok.calibrate([np.array([lo, 0, 1, 2, 3])], M7)
    assert GarbledCircuit(ok, 7, 100.0, seed=SEED, rescale="mrs", clip="joint").clip == "joint"
    from dash_amd.config import DashConfig

    with pytest.raises(ValueError, match="bad clip construction"):
        DashConfig(clip="both").gc_kwargs()
    assert DashConfig(clip="joint").gc_kwargs()["clip"] == "joint" and "clip" not in DashConfig().gc_kwargs()


def test_environment_knob_never_raises(monkeypatch):
    c = pair_circuit(5, 5, 192)
    _, _, lo, _ = pair_domain(M7, 5, 192)
    monkeypatch.setenv("DASH_CLIP", "joint")
    assert GarbledCircuit(c, 7, 100.0, seed=SEED, rescale="mrs").clip == "joint"
    # explicit wins over the environment
    assert GarbledCircuit(c, 7, 100.0, seed=SEED, rescale="mrs", clip="separate").clip == "separate"
    # silently separate where the resolved constructions cannot carry it
    with pytest.warns(UserWarning):
        legacy = GarbledCircuit(d.Circuit([d.Rescale(5, (5,)), d.Relu((5,))]), 7, 100.0, seed=SEED, rescale="legacy")
    assert legacy.clip == "separate"
    low = pair_circuit(5, 5, 192)
    low.calibrate([np.array([lo - 1, 0, 1, 2, 3])], M7)
    fell = GarbledCircuit(low, 7, 100.0, seed=SEED, rescale="mrs")
    assert fell.clip == "separate" and "clip" not in fell.effective_constructions()
    monkeypatch.setenv("DASH_CLIP", "separate")
    assert GarbledCircuit(c, 7, 100.0, seed=SEED, rescale="mrs").clip == "separate"
    monkeypatch.setenv("DASH_CLIP", "nonsense")  # not a value of the knob: ignored
    assert GarbledCircuit(c, 7, 100.0, seed=SEED, rescale="mrs").clip == "separate"


# ---------------------------------------------------------------- 4. wire format
def test_serialize_roundtrip_and_loader_refusal():
    N = 9
    gc = GarbledCircuit(pair_circuit(N, 5, 6), 7, 100.0, seed=SEED, rescale="mrs", clip="joint")
    blob = _blob(gc)
    back = native().GarbledModel.deserialize(blob)
    assert bytes(back.serialize()) == blob
    x = pair_inputs(N, M7, 5, 6)
    enc = gc.garble_inputs(x)
    for (pa, la), (pb, lb) in zip(gc.cpu_evaluate(enc), native().cpu_evaluate(back, enc, 0)):
        assert pa == pb
        np.testing.assert_array_equal(la, lb)
    # a hand-edited smode = 2 on a Clip that is not behind a sign_out rescale is refused by the evaluator
    sep = GarbledCircuit(pair_circuit(N, 5, 6), 7, 100.0, seed=SEED, rescale="mrs", clip="separate")
    assert list(sep.model.layer_params(1)["smode"]) == [1]
    raw = bytearray(_blob(sep))
    at = raw.find(b"smode")
    assert at > 0 and raw.count(b"smode") == 1
    one = raw.find((1).to_bytes(8, "little"), at + 5)
    assert 0 < one - at <= 16  # the parameter's single int64 value right behind its name and count
    raw[one:one + 8] = (2).to_bytes(8, "little")
    forged = native().GarbledModel.deserialize(bytes(raw))
    assert list(forged.layer_params(1)["smode"]) == [2]
    with pytest.raises(Exception, match="joint Clip without a preceding sign-producing rescale"):
        native().cpu_evaluate(forged, sep.garble_inputs(x), 0)


# ---------------------------------------------------------------- 5. range guard
def test_guard_bound_on_both_paths():
    pytest.importorskip("torch")
    N = 6
    _, t_hi, lo, hi = pair_domain(M7, 5, 192)
    gc = GarbledCircuit(pair_circuit(N, 5, 192), 7, 100.0, seed=SEED, rescale="mrs", clip="joint")
    assert gc.guard_enabled and gc.guard.joint_clips == {1: t_hi}
    ok = np.array([lo, hi - 1, 0, t_hi, -31, 5])
    low, high = ok.copy(), ok.copy()
    low[0] = lo - 1   # x - t_hi = -M/2 - 1
    high[1] = hi      # the mixed-radix wrap band
    g = gc.guard
    assert [bool(g.violations_np(x)) for x in (ok, low, high)] == [False, True, True]  # numpy path
    assert g.submit([ok, low, high]).bad_indices() == [1, 2]                             # torch path
    np.testing.assert_array_equal(_host_eval(gc, ok), closed_form(ok, 5, 192))
    for x in (low, high):
        with pytest.raises(RangeGuardError):
            gc.garble_inputs(x)
    # the separate construction's guard accepts lo - 1 (its bound is on the Clip's own small input)
    sep = GarbledCircuit(pair_circuit(N, 5, 192), 7, 100.0, seed=SEED, rescale="mrs", clip="separate")
    assert not sep.guard.violations_np(low) and sep.guard is not g
    assert not RangeGuard(pair_circuit(N, 5, 192), M7, mrs=True).violations_np(low)


# ---------------------------------------------------------------- 6. the cut-down MobileNet
def tiny_relu6_net():
    """tests/test_clip.py's cut-down MobileNet with its one narrow Clip(-0.25, 0.25) replaced by a ReLU6, so that
    every Clip meets the joint conditions."""
    ops = [("relu6",) if op[0] == "clip" else op for op in tc.TINY_MOBILENET["ops"]]
    saved = tc.TINY_MOBILENET
    tc.TINY_MOBILENET = dict(saved, ops=ops)
    try:
        return tc.tiny_mobilenet()
    finally:
        tc.TINY_MOBILENET = saved


def test_tiny_mobilenet_all_clips_joint():
    c, xs, k = tiny_relu6_net()
    nclip = sum(1 for l in c.layers if l.name == "clip")
    gc = GarbledCircuit(c, 7, 100.0, seed=SEED, rescale="mrs", relu="joint", clip="joint")
    assert nclip == 5 and len(gc.joint_clips) == nclip and gc.effective_constructions()["clip"] == "joint"
    sep = GarbledCircuit(c, 7, 100.0, seed=SEED, rescale="mrs", relu="joint", clip="separate")
    for i, l in enumerate(c.layers):
        if l.name == "clip":
            assert _layer_bytes(gc, i) == 16 * 240 * l.in_size and _layer_bytes(sep, i) == 16 * 387 * l.in_size
    assert gc.table_bytes < sep.table_bytes
    for x in xs:
        np.testing.assert_array_equal(_host_eval(gc, x), gc.plain_q_eval(x))
    # the model as tests/test_clip.py builds it keeps its Clip(-0.25, 0.25) separate
    c2, xs2, _ = tc.tiny_mobilenet()
    gc2 = GarbledCircuit(c2, 7, 100.0, seed=SEED, rescale="mrs", relu="joint", clip="joint")
    assert gc2.effective_constructions()["clip"] == "joint(4)+separate(1)"
    for x in xs2:
        np.testing.assert_array_equal(_host_eval(gc2, x), gc2.plain_q_eval(x))
