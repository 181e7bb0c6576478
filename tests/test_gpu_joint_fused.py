"""The fused joint rescale + ReLU output kernels at throughput batches (B >= 3), forced on with hip_set_joint_fuse.

In auto mode only batches of at most 2 GCs fuse (test_gpu_launch_forms.py covers those and pins the two-kernel path
at B = 3); here the knob forces the fusion at B = 3, where launch_rescale_relu_out picks the throughput form
(relu_out.tput: one 256-lane block per tile, residue and GC; the rescaled label never leaves LDS) for staged shapes
that are not small enough for the quad form, and the per-lane form for the others.

Circuits and inputs are those of test_gpu_launch_forms.py (J = Rescale(l) + Relu, mixed-radix rescale, joint ReLU,
host garbler, edge values around the sign threshold and +-S on tile, wave and 16-byte boundaries, a permuted input
per GC) and are shared with it. Each case asserts:
  * form: the launch log is the chain line plus one relu_out line, no out_hash / relu_mult launch;
  * labels: bit-identical to GarbledCircuit.cpu_evaluate and to the same circuits evaluated with the fusion off;
  * values: the decoded integers equal plain_q_eval and the closed form max(ceil(x / 2^l), 0).
"""
import os
import sys

import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_launch_forms as forms  # noqa: E402  (the J circuits, their inputs and the garbled-once cache)

pytestmark = pytest.mark.gpu

BIG = 1 << 20
B = 3
# one full tile; a tile, two and four tiles plus 16 live lanes; prime (per-lane form); below a tile
SIZES = [256, 272, 528, 1040, 1031, 144]


_SMALL = {}


def _small_circuit(k, N):
    """forms._circuit("J", k, N) for a layer too short for its edge list (it needs 70 + 4 S + 10 elements): the same
    random draw and the same cardinal edges on the boundary indices; the run of edge values is thinned to the
    neighbourhoods of 0, +-S and +-2 S and the domain's ends, on the indices the cardinal edges leave free."""
    if (k, N) in _SMALL:
        return _SMALL[(k, N)]
    l = forms._shift("J", k)
    M = GarbledCircuit(d.Circuit([d.Relu((1,))]), k, forms._mrs_arg(k), garble_me=False).crt_modulus
    S, h = 1 << l, M // 2
    hi = h - S
    x = np.random.default_rng(1000 * k + N).integers(-h, hi, N).astype(np.int64)
    edges = [-h, h - S - 1] + [c * S + o for c in (-2, -1, 0, 1, 2) for o in (-2, -1, 0, 1, 2)]
    cardinal = [-h, hi - 1, 0, -1, 1, -S, S, -S - 1, S + 1, -2 * S - 2, 2 * S + 2, -S + 1]
    at = {i % N: cardinal[n % len(cardinal)] for n, i in enumerate(forms.EDGE_AT) if -N <= i < N}
    free = [i for i in range(N) if i not in at]
    assert len(edges) <= len(free) and all(-h <= v < hi for v in edges + cardinal)
    x[free[:len(edges)]] = edges
    for i, v in at.items():
        x[i] = v
    xs = [x, x[::-1].copy(), np.roll(x, 7)]
    circ = d.Circuit([d.Rescale(l, (N,)), d.Relu((N,))])
    gcs = [GarbledCircuit(circ, k, forms._mrs_arg(k), seed=bytes([k, i + 1]) * 8, rescale="mrs", relu="joint")
           for i in range(3)]
    enc = [g.garble_inputs(v) for g, v in zip(gcs, xs)]
    closed = [np.maximum(-((-v) // S), 0) for v in xs]
    for g, v, c0 in zip(gcs, xs, closed):
        np.testing.assert_array_equal(g.plain_q_eval(v), c0)
    _SMALL[(k, N)] = dict(gcs=gcs, enc=enc, cpu=[g.cpu_evaluate(e) for g, e in zip(gcs, enc)], closed=closed,
                          crt=gcs[0].crt_base)
    return _SMALL[(k, N)]


def _circuit(k, N):
    l = forms._shift("J", k)
    return forms._circuit("J", k, N) if N >= 70 + 4 * (1 << l) + 10 else _small_circuit(k, N)


def _evaluate(native, gcs, enc, count, fuse):
    """One eager run of a fresh evaluator planned with `count` CUs and the fusion forced to `fuse`: (log, labels)."""
    from dash_amd.runtime import HipEvaluator

    base = native.hip_joint_fuse()
    native.hip_launch_log_take()
    native.hip_set_planning_cus(count)
    native.hip_set_joint_fuse(fuse)
    try:
        ev = HipEvaluator([g.model for g in gcs])  # fresh: an evaluator's picks freeze when it plans
        native.hip_launch_log(True)
        try:
            out = ev.evaluate(enc)  # the first run of an evaluator is eager
        finally:
            native.hip_launch_log(False)
        log = native.hip_launch_log_take()
    finally:
        native.hip_set_joint_fuse(base)
        native.hip_set_planning_cus(0)
    return log, out


def _same_labels(want, got):
    assert len(want) == len(got)
    for w, g in zip(want, got):
        assert len(w) == len(g)
        for (pw, aw), (pg, ag) in zip(w, g):
            assert pw == pg
            np.testing.assert_array_equal(aw, ag)


def _expected_out(native, k, N, count):
    cus = count if count else native.hip_planning_cus()
    if forms._ceil(N, 256) * k * B <= cus:
        return forms._line("relu_out.quad", (forms._ceil(N, 64), k, B), 256)
    if N % 16 == 0 and N >= 256:
        return forms._line("relu_out.tput", (forms._ceil(N, 256), k, B), 256)
    return forms._aes("relu_out.lane", N, k, B, cus)


def _run(native, k, N, count):
    c = _circuit(k, N)
    gcs, enc = c["gcs"][:B], c["enc"][:B]
    log, fused = _evaluate(native, gcs, enc, count, 1)
    print("\n".join(log))
    cus = count if count else native.hip_planning_cus()
    assert log == [forms._chain(native, c["crt"], 2, N, B, cus), _expected_out(native, k, N, count)]
    assert not any("out_hash" in ln or "relu_mult" in ln for ln in log)
    log_off, unfused = _evaluate(native, gcs, enc, count, 0)
    assert log_off == forms._expected(native, "J", c["crt"], N, B, cus)  # out_hash + relu_mult
    _same_labels(c["cpu"][:B], fused)
    _same_labels(unfused, fused)
    for g, o, ref in zip(gcs, fused, c["closed"]):
        np.testing.assert_array_equal(g.decode_outputs(o), ref)  # == plain_q_eval (checked when garbled)


@pytest.mark.parametrize("count", [1, 0, BIG], ids=["cus1", "device", "cus1M"])
@pytest.mark.parametrize("N", SIZES)
def test_fused_k7(native, N, count):
    _run(native, 7, N, count)


def test_fused_k7_takes_the_throughput_form(native):
    """Written out, not derived: at planning count 1 every staged size runs relu_out.tput, one block per tile."""
    c = forms._circuit("J", 7, 1040)
    log, _ = _evaluate(native, c["gcs"][:B], c["enc"][:B], 1, 1)
    assert log[1:] == ["relu_out.tput grid=(5,7,3) block=256"]


@pytest.mark.parametrize("k", [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12])
def test_fused_every_k(native, k):
    _run(native, k, 528, 1)


def test_kept_rescale_output_is_not_fused(native):
    """A later layer reads the rescaled label (Add(src=0)): the planner must not defer it, whatever the knob says."""
    k, N = 7, 528
    l = forms._shift("J", k)
    x, S = forms._inputs("J", k, N)
    xs = [x, x[::-1].copy(), np.roll(x, 7)]
    circ = d.Circuit([d.Rescale(l, (N,)), d.Relu((N,)), d.Add((N,), 0)])
    gcs = [GarbledCircuit(circ, k, forms._mrs_arg(k), seed=bytes([k, i + 1]) * 8, rescale="mrs", relu="joint")
           for i in range(B)]
    enc = [g.garble_inputs(v) for g, v in zip(gcs, xs)]
    log, gpu = _evaluate(native, gcs, enc, 1, 1)
    print("\n".join(log))
    assert any(ln.startswith("out_hash.") for ln in log) and any(ln.startswith("relu_mult.") for ln in log)
    assert not any("relu_out" in ln for ln in log)
    _same_labels([g.cpu_evaluate(e) for g, e in zip(gcs, enc)], gpu)
    for g, o, v in zip(gcs, gpu, xs):
        r = -((-v) // S)
        np.testing.assert_array_equal(g.decode_outputs(o), np.maximum(r, 0) + r)
        np.testing.assert_array_equal(g.plain_q_eval(v), np.maximum(r, 0) + r)
