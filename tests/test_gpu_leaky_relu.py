"""The LeakyRelu layer on the GPU (docs/LEAKY_RELU.md): the HIP evaluator's leaky multiply in its per-lane
(k_leaky_mult, log name leaky_mult.lane), staged (k_leaky_mult_s, leaky_mult.staged) and fused throughput
(k_rescale_leaky_out_t, leaky_out.tput) forms, bit-exact against the host evaluator over one eager and two
graph-replayed rounds of two GCs, every sign construction, the GPU garbler byte-identical to the host garbler (also
into an evaluator slot) and the two-layer chain whose second rescale absorbs the layer's scale bits. Circuits and
inputs: tests/leaky_cases.py."""
import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit
from tests import test_gpu_joint_fused as jf
from tests.leaky_cases import (M7, conv_chain, conv_chain_inputs, expected, leaky_circuit, leaky_inputs, rescale_leaky,
                               slopes)
from tests.test_gpu_mul import _run
from tests.test_gpu_parity import _gpu_vs_host, _same

pytestmark = pytest.mark.gpu
forms = jf.forms  # the J inputs and the pickers restated, one module object with test_gpu_joint_fused

S = 4


# approx with the legacy rescale is the reference encoding; the mixed-radix constructions are hardened
_KW = {"approx": dict(rescale="legacy", relu="approx", hardened=False), "mrs": dict(rescale="mrs", relu="mrs"),
       "joint": dict(rescale="mrs", relu="joint")}


def _mult_lines(log):
    return [l.split()[0] for l in log if l.startswith("leaky_mult.")]


@pytest.mark.parametrize("N,form", [(1, "lane"), (77, "lane"), (256, "staged"), (260, "lane"), (272, "staged")])
def test_scalar_slope(native, N, form):
    """One element; below two waves; exactly one staged tile (k_leaky_mult_s); N % 16 != 0, the lane form
    (k_leaky_mult); staged with a partial last tile."""
    c = leaky_circuit((N,), S)
    n = c.layers[0].n
    log = _run(c, leaky_inputs((N,), 7, S, rounds=6), log=native, want=lambda x: expected(x, n, S))
    print("\n".join(log))
    assert _mult_lines(log) == ["leaky_mult." + form], log


@pytest.mark.parametrize("dims,form", [((5, 4, 20), "staged"), ((3, 20, 26), "lane")], ids=["5x4x20", "3x20x26"])
def test_per_channel_slopes(native, dims, form):
    """(5, 4, 20): N = 400, a staged tile that crosses the channel boundaries at 80, 160, 240 and 320; (3, 20, 26):
    N = 1560, N % 16 != 0, a boundary at 520. The slopes include n = 0 and n = 2^s - 1."""
    c = leaky_circuit(dims, S, per_channel=True)
    n, bc = c.layers[0].n, c.layers[0].bc
    assert 0 in n and (1 << S) - 1 in n and n.size == dims[0] and bc == dims[1] * dims[2]
    log = _run(c, leaky_inputs(dims, 7, S, rounds=6), log=native, want=lambda x: expected(x, n, S, bc))
    assert _mult_lines(log) == ["leaky_mult." + form], log


@pytest.mark.parametrize("relu", ["approx", "mrs", "joint"])
def test_sign_constructions(native, relu):
    """conv -> Rescale(3) -> LeakyRelu (per-channel, N = 272) under each sign construction; two GCs (B = 2), so the
    joint case is a launch at which the ReLU would take a small-batch fused form: the leaky runs the output-hash
    kernel and the staged multiply."""
    c = conv_chain()
    kw = _KW[relu]
    log = _run(c, conv_chain_inputs(rounds=6), log=native, **kw)
    print("\n".join(log))
    assert _mult_lines(log) == ["leaky_mult.staged"], log
    assert not any(l.startswith(("relu_mult.", "relu_out.", "leaky_out.")) for l in log)
    if relu == "joint":
        assert any("out_hash." in l for l in log), log


# ---------------------------------------------------------------- the fused throughput form
B = 3


def _joint_case(k, N, per_channel=True):
    l = forms._shift("J", k)
    c = rescale_leaky(k, N, l, per_channel)
    x, _ = forms._inputs("J", k, N)
    xs = [x, x[::-1].copy(), np.roll(x, 7)]
    gcs = [GarbledCircuit(c, k, forms._mrs_arg(k), seed=bytes([k, i + 1]) * 8, rescale="mrs", relu="joint")
           for i in range(B)]
    assert gcs[0].effective_constructions()["relu"] == "joint"
    enc = [g.garble_inputs(v) for g, v in zip(gcs, xs)]
    lk = c.layers[1]
    want = [expected(-((-v) // (1 << l)), lk.n, lk.slope_bits, lk.bc) for v in xs]
    return c, gcs, enc, xs, want


@pytest.mark.parametrize("k,N", [(7, 528), (7, 1040), (2, 528), (12, 528)])
def test_fused_throughput_form(native, k, N):
    """B = 3, the fusion forced on, planned for one CU (so no launch is small enough for the quad form): the log
    shows leaky_out.tput (k_rescale_leaky_out_t), one block per tile, and neither an output-hash nor a multiply
    launch. The labels equal the host evaluator's and those with the knob forced off."""
    c, gcs, enc, xs, want = _joint_case(k, N)
    log, fused = jf._evaluate(native, gcs, enc, 1, 1)
    print("\n".join(log))
    assert log[1:] == [forms._line("leaky_out.tput", (forms._ceil(N, 256), k, B), 256)], log
    log_off, unfused = jf._evaluate(native, gcs, enc, 1, 0)
    assert any("out_hash." in l for l in log_off) and _mult_lines(log_off) == ["leaky_mult.staged"], log_off
    assert not any("leaky_out" in l for l in log_off)
    jf._same_labels([g.cpu_evaluate(e) for g, e in zip(gcs, enc)], fused)
    jf._same_labels(unfused, fused)
    for g, o, v, w in zip(gcs, fused, xs, want):
        np.testing.assert_array_equal(g.decode_outputs(o), w)
        np.testing.assert_array_equal(g.plain_q_eval(v), w)


def test_kept_rescale_output_is_not_fused(native):
    """A later Add reads the rescaled label: the planner must not defer it, whatever the knob says."""
    k, N = 7, 528
    l = forms._shift("J", k)
    x, _ = forms._inputs("J", k, N)
    xs = [x, x[::-1].copy(), np.roll(x, 7)]
    lk = d.LeakyRelu.from_quantized((N,), 1, 1)
    circ = d.Circuit([d.Rescale(l, (N,)), lk, d.Add((N,), 0)])
    gcs = [GarbledCircuit(circ, k, forms._mrs_arg(k), seed=bytes([k, i + 1]) * 8, rescale="mrs", relu="joint")
           for i in range(B)]
    enc = [g.garble_inputs(v) for g, v in zip(gcs, xs)]
    log, gpu = jf._evaluate(native, gcs, enc, 1, 1)
    print("\n".join(log))
    assert any("out_hash." in l for l in log) and _mult_lines(log) == ["leaky_mult.staged"], log
    assert not any("leaky_out" in l for l in log)
    jf._same_labels([g.cpu_evaluate(e) for g, e in zip(gcs, enc)], gpu)
    for g, o, v in zip(gcs, gpu, xs):
        r = -((-v) // (1 << l))
        np.testing.assert_array_equal(g.decode_outputs(o), expected(r, [1], 1) + r)
        np.testing.assert_array_equal(g.plain_q_eval(v), expected(r, [1], 1) + r)


# ---------------------------------------------------------------- GPU garbler
@pytest.mark.parametrize("relu", ["approx", "mrs", "joint"])
def test_gpu_garbler_bit_identical(relu):
    """The device garbles the ReLU's tables and maps the zero labels with one elementwise kernel; the model and the
    decoder equal the host garbler's byte for byte."""
    kw = _KW[relu]
    g = _gpu_vs_host(conv_chain(), 7, 100.0, **kw)
    assert g.effective_constructions()["relu"] == relu


def test_gpu_garbler_into_evaluator_slot():
    """The GPU garbler writes the tables straight into an evaluator slot (HipEvaluator.sink); both slots evaluate
    and decode."""
    from dash_amd.runtime import HipEvaluator

    c = conv_chain()
    kw = dict(rescale="mrs", relu="joint")
    first = GarbledCircuit(c, 7, 100.0, seed=bytes([7]) * 16, device=0, **kw)
    ev = HipEvaluator(template=first.model, batch=2, device=0)
    ev.load(0, first.model)
    seed = bytes(range(16))
    into = GarbledCircuit(c, 7, 100.0, seed=seed, device=0, sink=ev.sink(1), **kw)
    host = GarbledCircuit(c, 7, 100.0, seed=seed, **kw)
    assert _same(into.model.serialize(), host.model.serialize())
    ev.load(1, into.model)
    xs = conv_chain_inputs()
    for b, gc in enumerate((first, into)):
        ev.encode_compressed_into(b, gc, xs[b])
    ev.upload_inputs_compressed()
    ev.run()
    ev.fetch_outputs()
    for b, gc in enumerate((first, into)):
        np.testing.assert_array_equal(ev.decode(b, gc), c.plain_q_eval(xs[b], False, M7))


# ---------------------------------------------------------------- the scale bits reach the next rescale
def test_two_layer_chain():
    """conv -> Rescale(l) -> LeakyRelu(s) -> conv(in_scale_bits = s) -> Rescale(l + s), decoded exactly: the
    mixed-radix rescale with l + s = 6 bits runs on the device."""
    c = conv_chain(second=True)
    assert c.layers[4].l == c.layers[1].l + c.layers[2].slope_bits == 6

    def want(x):
        lk = c.layers[2]
        y = c.layers[0].plain_q_eval(x, False)
        y = expected(-((-y) // 8), lk.n, lk.slope_bits, lk.bc)
        return -((-c.layers[3].plain_q_eval(y, False)) // 64)

    _run(c, conv_chain_inputs(rounds=6), rescale="mrs", relu="joint", want=want)
