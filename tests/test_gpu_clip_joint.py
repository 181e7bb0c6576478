"""The joint Clip construction on the GPU (docs/CLIP.md): the HIP evaluator's path for a Rescale(l) + Clip(0, q_hi)
pair garbled with clip="joint" (rescale chain in mode 2 keeping its sign label, the Clip's upper sign chain in
mode 1 on the same input labels, the rescale's output-hash kernel, the clip multiply), bit-exact against the host
evaluator, and the GPU garbler's joint form byte-identical to the host garbler.

Helpers of tests/test_gpu_launch_forms.py (the pickers restated, the launch log lines) and of
tests/test_gpu_joint_fused.py (fresh evaluator under a planning count and a joint-fuse mode) are reused.

Unfused (hip_set_joint_fuse(0), and the auto mode below 2048 elements or 3 GCs): the launch log is exactly chain
mode 2, chain mode 1, out_hash.*, clip_mult.*; no k_label_hash pass of a Clip and no second sign chain. Fused
(hip_set_joint_fuse(1), or auto from 2048 elements; B >= 3, staged shapes): the two chains plus clip_out.tput, the
rescaled label never written; every other forced launch logs the unfused lines. Every case compares the labels with
GarbledCircuit.cpu_evaluate and the decoded integers with the closed form min(max(ceil(x / S), 0), q_hi).
"""
import os
import sys

import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_clip_joint as cj  # noqa: E402
import test_gpu_joint_fused as jf  # noqa: E402
import test_gpu_launch_forms as forms  # noqa: E402

pytestmark = pytest.mark.gpu

BIG = 1 << 20


def _q_hi(k):
    """The upper bound per CRT size of the `forms` J circuits (their shift l = forms._shift("J", k)): the domain
    [-M/2 + t_hi, mrs_limit) must hold both thresholds +-2. M = 6 (k = 2, l = 1) leaves [-2, 3) at q_hi = 1 and
    M = 30 (k = 3) [-10, 14) at q_hi = 3; from k = 4 on (M >= 210) ReLU6's 6 fits. No k is left out."""
    return {2: 1, 3: 3}.get(k, 6)


def _pair_inputs(M, l, q_hi, N):
    """x for GC 0: random over the joint domain; both thresholds +-2 and the domain's ends from index 70 on (N
    permitting) and, always, on the element indices where a tile, a wave or a 16-byte row starts or ends."""
    t_lo, t_hi, lo, hi = cj.pair_domain(M, l, q_hi)
    x = np.random.default_rng(N).integers(lo, hi, N).astype(np.int64)
    edges = [v for v in [t + o for t in (t_lo, t_hi) for o in (-2, -1, 0, 1, 2)] + [lo, hi - 1] if lo <= v < hi]
    if N >= 70 + len(edges):
        x[70:70 + len(edges)] = edges
    for n, i in enumerate(forms.EDGE_AT):
        if -N <= i < N:
            x[i] = edges[n % len(edges)]
    return x


_BUILT = {}


def _pair(crt, mrs, l, q_hi, N):
    """Three GCs of the pair (host garbler, one seed each), a permuted input per GC, host labels, closed form."""
    key = (str(crt), l, q_hi, N)
    if key in _BUILT:
        return _BUILT[key]
    c = cj.pair_circuit(N, l, q_hi)
    gcs = [GarbledCircuit(c, crt, mrs, seed=bytes([9, i + 1]) * 8, rescale="mrs", clip="joint") for i in range(3)]
    assert all(g.clip == "joint" for g in gcs)
    x = _pair_inputs(gcs[0].crt_modulus, l, q_hi, N)
    xs = [x, x[::-1].copy(), np.roll(x, 7)]
    enc = [g.garble_inputs(v) for g, v in zip(gcs, xs)]
    closed = [cj.closed_form(v, l, q_hi) for v in xs]
    for g, v, c0 in zip(gcs, xs, closed):
        np.testing.assert_array_equal(g.plain_q_eval(v), c0)
    _BUILT[key] = dict(gcs=gcs, enc=enc, cpu=[g.cpu_evaluate(e) for g, e in zip(gcs, enc)], closed=closed,
                       crt=gcs[0].crt_base, xs=xs)
    return _BUILT[key]


def _expected(native, crt, N, B, cus):
    k = len(crt)
    if N % 16 == 0 and N >= 512:
        out = forms._line("out_hash.staged", (forms._grid_aes(N, 512, k, B, cus), k, B), 512)
    else:
        out = forms._aes("out_hash.lane", N, k, B, cus)
    return [forms._chain(native, crt, 2, N, B, cus), forms._chain(native, crt, 1, N, B, cus), out,
            forms._relu_mult(k, N, B, cus).replace("relu_mult.", "clip_mult.")]


def _expected_fused(native, crt, N, B, cus):
    if B >= 3 and N % 16 == 0 and N >= 256:
        return [forms._chain(native, crt, 2, N, B, cus), forms._chain(native, crt, 1, N, B, cus),
                forms._line("clip_out.tput", (forms._ceil(N, 256), len(crt), B), 256)]
    return _expected(native, crt, N, B, cus)


def _run_fused(native, c, N, B, count):
    """The fusion forced on: the log, the labels against the host and against the same GCs with it forced off."""
    gcs, enc = c["gcs"][:B], c["enc"][:B]
    cus = count if count else native.hip_planning_cus()
    log, fused = jf._evaluate(native, gcs, enc, count, 1)
    print("\n".join(log))
    assert log == _expected_fused(native, c["crt"], N, B, cus)
    log_off, unfused = jf._evaluate(native, gcs, enc, count, 0)
    assert log_off == _expected(native, c["crt"], N, B, cus)
    jf._same_labels(c["cpu"][:B], fused)
    jf._same_labels(unfused, fused)
    for g, o, ref in zip(gcs, fused, c["closed"]):
        np.testing.assert_array_equal(g.decode_outputs(o), ref)
    return log


def _run(native, c, N, B, count, fuse=-1, replay=False):
    from dash_amd.runtime import HipEvaluator

    gcs, enc = c["gcs"][:B], c["enc"][:B]
    cus = count if count else native.hip_planning_cus()
    if replay:  # one evaluator, run twice: the second run replays the captured graph
        native.hip_set_planning_cus(count)
        try:
            ev = HipEvaluator([g.model for g in gcs])
            first, second = ev.evaluate(enc), ev.evaluate(enc)
        finally:
            native.hip_set_planning_cus(0)
        jf._same_labels(first, second)
        jf._same_labels(c["cpu"][:B], second)
        return
    log, gpu = jf._evaluate(native, gcs, enc, count, fuse)
    print("\n".join(log))
    assert log == _expected(native, c["crt"], N, B, cus)
    assert sum("mode=1" in ln for ln in log) == 1 and not any("k_label_hash" in ln or "clip_out" in ln for ln in log)
    assert log[3].startswith("clip_mult.staged" if N % 16 == 0 and N >= 256 else "clip_mult.lane")
    jf._same_labels(c["cpu"][:B], gpu)
    for g, o, ref in zip(gcs, gpu, c["closed"]):
        np.testing.assert_array_equal(g.decode_outputs(o), ref)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [1, 75, 513, 528, 1031, 1040])
def test_unfused_path(native, N, B):
    """A single lane, an odd size, one past a 512 tile, staged sizes with 16 live lanes in the last tile, a prime."""
    _run(native, _pair(7, 100.0, 5, 192, N), N, B, 0)


@pytest.mark.parametrize("count", [1, BIG], ids=["cus1", "cus1M"])
@pytest.mark.parametrize("N", [528, 1031])
def test_forms_under_planning_counts(native, N, count):
    """528 takes the staged multiply and 1031 the per-lane one under both counts, which move the two chains and
    the output-hash kernel between their forms."""
    _run(native, _pair(7, 100.0, 5, 192, N), N, 3, count)


@pytest.mark.parametrize("N", [528, 1031])
def test_graph_replay_gives_the_same_labels(native, N):
    _run(native, _pair(7, 100.0, 5, 192, N), N, 3, 0, replay=True)


@pytest.mark.parametrize("count", [1, 0, BIG], ids=["cus1", "device", "cus1M"])
@pytest.mark.parametrize("N", [256, 272, 528, 1040])
def test_fused_path(native, N, count):
    """One full tile; a tile, two and four tiles plus 16 live lanes: the two chains plus one clip_out.tput block
    per (tile, residue, GC) under every planning count."""
    log = _run_fused(native, _pair(7, 100.0, 5, 192, N), N, 3, count)
    assert log[2] == "clip_out.tput grid=(%d,7,3) block=256" % -(-N // 256)
    assert not any("out_hash" in ln or "clip_mult" in ln for ln in log)


@pytest.mark.parametrize("N,B", [(1031, 3), (144, 3), (528, 1), (1040, 2)])
def test_forced_fusion_falls_back(native, N, B):
    """Unstaged shapes (a prime, less than a tile) and batches below 3: the forced fusion logs the unfused lines."""
    log = _run_fused(native, _pair(7, 100.0, 5, 192, N), N, B, 1)
    assert len(log) == 4 and not any("clip_out" in ln for ln in log)


def test_auto_rule(native):
    """hip_clip_fuse_pick, the auto rule (docs/CLIP.md): batches of at least 3 GCs, staged shapes from 2048
    elements. 2064 = 8 tiles + 16 lanes fuses in auto mode, 1040 does not (test_unfused_path runs in auto mode)."""
    pick = native.hip_clip_fuse_pick
    assert pick(2048, 3) and pick(16384, 24) and pick(2064, 85)
    assert not (pick(2032, 3) or pick(2047, 24) or pick(4096, 2) or pick(16384, 1) or pick(1040, 24))
    c = _pair(7, 100.0, 5, 192, 2064)
    log, gpu = jf._evaluate(native, c["gcs"], c["enc"], 0, -1)
    assert log == _expected_fused(native, c["crt"], 2064, 3, native.hip_planning_cus())
    assert log[2] == "clip_out.tput grid=(9,7,3) block=256"
    jf._same_labels(c["cpu"], gpu)
    log2, gpu2 = jf._evaluate(native, c["gcs"][:2], c["enc"][:2], 0, -1)
    assert log2 == _expected(native, c["crt"], 2064, 2, native.hip_planning_cus())
    jf._same_labels(c["cpu"][:2], gpu2)


def test_kept_rescale_output(native):
    """A later layer reads the rescaled label (Add(src=0)): it is written by the output-hash kernel as always."""
    N, l, q_hi, B = 528, 5, 192, 3
    circ = d.Circuit([d.Rescale(l, (N,)), d.Clip.from_quantized((N,), 0, q_hi), d.Add((N,), 0)])
    gcs = [GarbledCircuit(circ, 7, 100.0, seed=bytes([5, i + 1]) * 8, rescale="mrs", clip="joint") for i in range(B)]
    assert all(g.joint_clips for g in gcs)
    x = _pair_inputs(gcs[0].crt_modulus, l, q_hi, N)
    xs = [x, x[::-1].copy(), np.roll(x, 7)]
    enc = [g.garble_inputs(v) for g, v in zip(gcs, xs)]
    log, gpu = jf._evaluate(native, gcs, enc, 1, 1)
    print("\n".join(log))
    assert any(ln.startswith("out_hash.") for ln in log) and any(ln.startswith("clip_mult.") for ln in log)
    assert len(log) == 4 and not any("clip_out" in ln for ln in log)  # never fused, whatever the knob says
    jf._same_labels([g.cpu_evaluate(e) for g, e in zip(gcs, enc)], gpu)
    for g, o, v in zip(gcs, gpu, xs):
        r = -((-v) // (1 << l))
        np.testing.assert_array_equal(g.decode_outputs(o), np.minimum(np.maximum(r, 0), q_hi) + r)


def test_large_residue_base(native):
    """[2, 131]: label bytes above 127 through both chains, the output-hash walk, the clip multiply and the fused
    kernel's two passes."""
    log = _run_fused(native, _pair([2, 131], None, 2, 6, 528), 528, 3, 1)
    assert log[2].startswith("clip_out.tput")


@pytest.mark.parametrize("k", [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12])
def test_every_k(native, k):
    log = _run_fused(native, _pair(k, forms._mrs_arg(k), forms._shift("J", k), _q_hi(k), 528), 528, 3, 1)
    assert log[2] == "clip_out.tput grid=(3,%d,3) block=256" % k


# ------------------------------------------------------------------------------------------------ GPU garbler
def test_gpu_garbler_bit_identical():
    from tests.test_gpu_parity import _gpu_vs_host

    for crt, mrs, l, q_hi, N in [(7, 100.0, 5, 192, 300), ([2, 131], None, 2, 6, 75), (3, None, 1, 3, 33)]:
        g = _gpu_vs_host(cj.pair_circuit(N, l, q_hi), crt, mrs, rescale="mrs", clip="joint")
        assert g.clip == "joint" and list(g.model.layer_params(1)["smode"]) == [2]


def test_gpu_garbler_into_evaluator_slot():
    from dash_amd.runtime import HipEvaluator
    from tests.test_gpu_parity import _same

    rng = np.random.default_rng(4)
    N, l, q_hi = 300, 5, 192
    a = d.Dense.from_quantized(rng.integers(-40, 41, (N, 30)), rng.integers(-6, 6, N))
    c = d.Circuit([a, d.Rescale(l, (N,)), d.Clip.from_quantized((N,), 0, q_hi)])
    kw = dict(rescale="mrs", relu="joint", clip="joint")
    first = GarbledCircuit(c, 7, 100.0, seed=bytes([7]) * 16, device=0, **kw)
    ev = HipEvaluator(template=first.model, batch=2, device=0)
    ev.load(0, first.model)
    into = GarbledCircuit(c, 7, 100.0, seed=bytes(range(16)), device=0, sink=ev.sink(1), **kw)
    host = GarbledCircuit(c, 7, 100.0, seed=bytes(range(16)), **kw)
    assert into.joint_clips and _same(into.model.serialize(), host.model.serialize())
    ev.load(1, into.model)
    xs = [rng.integers(-100, 101, 30) for _ in range(2)]
    for b, gc in enumerate((first, into)):
        ev.encode_compressed_into(b, gc, xs[b])
    ev.upload_inputs_compressed()
    ev.run()
    ev.fetch_outputs()
    for b, gc in enumerate((first, into)):
        want = gc.plain_q_eval(xs[b])
        assert want.max() == q_hi and want.min() == 0
        np.testing.assert_array_equal(ev.decode(b, gc), want)


def test_tiny_mobilenet_joint_on_the_device():
    """The cut-down MobileNet, every Clip joint, garbled on the device, HIP evaluator, batch 1."""
    from dash_amd.runtime import HipEvaluator

    c, xs, _ = cj.tiny_relu6_net()
    gc = GarbledCircuit(c, 7, 100.0, seed=bytes(range(16)), device=0, rescale="mrs", relu="joint", clip="joint")
    assert gc.effective_constructions()["clip"] == "joint"
    ev = HipEvaluator(template=gc.model, batch=1, device=0)
    ev.load(0, gc.model)
    for x in xs:
        ev.encode_into(0, gc, x)
        ev.upload_inputs()
        ev.run()
        np.testing.assert_array_equal(gc.decode_outputs(ev.get_outputs()[0]), gc.plain_q_eval(x))
