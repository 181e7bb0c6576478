"""The staged mixed-radix chain's pair payloads: folded into the sign key, kept in LDS slots, or sent through a.ps.

k_mrs_chain_s (mrs_chain.h) keeps the payloads P[l][j] that position l hands to a later position j in per-lane
LDS slots that are reused once read, folds the ones aimed at the sign position (modes 1, 2) into a running XOR and
leaves what does not fit to the HBM scratch. ``hip_set_planning_cus(1)`` plans these small launches as the headline
is planned (staged form, capped grid, strided tile loop), as tests/test_gpu_launch_forms.py does.

Shapes: N = 512 is one full tile; 528 ends in a tile of 16 live lanes, whose spare lanes must not disturb slots
or the accumulator; 4624 = 9 * 512 + 16 is ten tiles on a grid capped at four blocks, so a block reuses its slots and
restarts its accumulator tile after tile. K = 2 has no stored pair in modes 1 and 2, K = 3 one, K = 7 is the
headline, and at K = 12 (66 pairs) slots, fold and the a.ps overflow all run in one kernel.

Each case asserts that the chain ran in its staged form, that the labels are bit-identical to
GarbledCircuit.cpu_evaluate, and that the decoded integers equal plain_q_eval. Circuits as in
tests/test_gpu_launch_forms.py: host garbler, 3 GCs, a different permutation of the inputs per GC; R = Rescale
(chain mode 0), S = Relu with the exact sign (mode 1), J = Rescale + Relu joint (mode 2).
"""
import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit

pytestmark = pytest.mark.gpu

SIZES = [512, 528, 4624]
KS = [2, 3, 7, 12]
EDGE_AT = [0, 15, 16, 63, 64, 511, 512, 527, 528, 4607, 4608, -17, -16, -1]  # tile / wave / 16-byte row boundaries


def _mrs_arg(k):
    return 100.0 if 4 <= k <= 11 else None  # the approximate sign's base (unused by the mixed-radix constructions)


def _shift(k):
    return 1 if k <= 3 else (2 if k <= 5 else 5)


def _build(kind, k, N):
    l = _shift(k)
    if kind == "R":
        layers, kw = [d.Rescale(l, (N,))], dict(rescale="mrs")
    elif kind == "S":
        layers, kw = [d.Relu((N,))], dict(relu="mrs")
    else:
        layers, kw = [d.Rescale(l, (N,)), d.Relu((N,))], dict(rescale="mrs", relu="joint")
    M = GarbledCircuit(d.Circuit([d.Relu((1,))]), k, _mrs_arg(k), garble_me=False).crt_modulus
    S, h = 1 << l, M // 2
    hi = h if kind == "S" else h - S  # the rescale's non-wrapping domain [-h, h - S)
    rng = np.random.default_rng(77 * k + N)
    x = rng.integers(-h, hi, N).astype(np.int64)
    edges = [v for v in [-h, hi - 1, 0, -1, 1, -S, S, -S - 1, S + 1, -S + 1] if -h <= v < hi]
    for n, i in enumerate(EDGE_AT):
        if -N <= i < N:
            x[i] = edges[n % len(edges)]
    xs = [x, x[::-1].copy(), np.roll(x, 7)]  # a permutation per GC: a wrong batch stride cannot cancel out
    c = d.Circuit(layers)
    gcs = [GarbledCircuit(c, k, _mrs_arg(k), seed=bytes([k, i + 11]) * 8, **kw) for i in range(3)]
    enc = [g.garble_inputs(v) for g, v in zip(gcs, xs)]
    cpu = [g.cpu_evaluate(e) for g, e in zip(gcs, enc)]
    plain = [g.plain_q_eval(v) for g, v in zip(gcs, xs)]
    return dict(gcs=gcs, enc=enc, cpu=cpu, plain=plain)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind", ["R", "S", "J"])
def test_staged_chain_payloads(native, kind, k, N):
    from dash_amd.runtime import HipEvaluator

    c = _build(kind, k, N)
    native.hip_launch_log_take()
    native.hip_set_planning_cus(1)
    try:
        ev = HipEvaluator([g.model for g in c["gcs"]])  # fresh: an evaluator's picks freeze at graph capture
        native.hip_launch_log(True)
        try:
            gpu = ev.evaluate(c["enc"])  # the first run of an evaluator is eager
        finally:
            native.hip_launch_log(False)
        log = native.hip_launch_log_take()
    finally:
        native.hip_set_planning_cus(0)
    print("\n".join(log))
    mode = {"R": 0, "S": 1, "J": 2}[kind]
    tiles = -(-N // 512)
    want = "chain.staged K=%d mode=%d grid=(%d,1,3) block=512" % (k, mode, min(tiles, 4))
    assert [ln for ln in log if ln.startswith("chain.")] == [want], log
    for want_gc, got_gc in zip(c["cpu"], gpu):
        assert len(want_gc) == len(got_gc)
        for (pw, aw), (pg, ag) in zip(want_gc, got_gc):
            assert pw == pg
            np.testing.assert_array_equal(aw, ag)
    for g, o, ref in zip(c["gcs"], gpu, c["plain"]):
        np.testing.assert_array_equal(g.decode_outputs(o), ref)
