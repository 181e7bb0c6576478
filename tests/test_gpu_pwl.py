"""The PiecewiseLinear layer on the GPU (docs/PWL.md): the HIP evaluator's one-pass multiply in its per-lane
(k_pwl_mult, log name pwl_mult.lane) and staged (k_pwl_mult_s, pwl_mult.staged) forms for 1, 2 and 8 kept
breakpoints, bit-exact against the host evaluator and the integer model over one eager and two graph-replayed
rounds of two GCs; every sign construction and the smallest and largest CRT bases; the GPU garbler byte-identical
to the host garbler (also into an evaluator slot); and the imported conv -> Rescale -> Sigmoid -> Mul -> conv chain
end to end. Layers and inputs: tests/pwl_cases.py."""
import numpy as np
import pytest

from dash_amd.garbling import GarbledCircuit
from dash_amd.ir.bases import crt_modulus, first_primes
from dash_amd.ir.quant import QuantizationMethod as Q
from tests.pwl_cases import M7, conv_chain, conv_chain_inputs, pwl_circuit, pwl_inputs, shape_for, want_of
from tests.test_gpu_mul import _run
from tests.test_gpu_parity import _gpu_vs_host, _same

pytestmark = pytest.mark.gpu

_KW = {"approx": dict(rescale="mrs", relu="approx"), "mrs": dict(rescale="mrs", relu="mrs"),
       "joint": dict(rescale="mrs", relu="joint")}


def _mult_lines(log):
    return [l.split()[0] for l in log if l.startswith("pwl_mult.")]


def _check_log(log, form):
    print("\n".join(log))
    assert _mult_lines(log) == ["pwl_mult." + form], log
    assert not any(l.startswith(("relu_mult.", "clip_mult.")) for l in log), log


def _form(N):
    return "staged" if N % 16 == 0 and N >= 256 else "lane"


@pytest.mark.parametrize("N,form", [(1, "lane"), (77, "lane"), (260, "lane"), (256, "staged"), (272, "staged")])
def test_forms(native, N, form):
    """m = 2. One element; below two waves; N % 16 != 0 with more than one block (k_pwl_mult); exactly one staged
    tile; staged with a partial last tile (k_pwl_mult_s)."""
    c = pwl_circuit((N,), "m2")
    log = _run(c, pwl_inputs((N,), c.layers[0], rounds=6), log=native, want=want_of(c.layers[0]), relu="mrs")
    _check_log(log, form)


@pytest.mark.parametrize("N", [272, 77])
@pytest.mark.parametrize("name,m", [("m1", 1), ("m8", 8), ("drop", 2)])
def test_breakpoint_counts(native, name, m, N):
    """One and eight breakpoints (the sigmoid's integers: steps of both signs), and three given of which the middle
    one is dropped (outer slopes not 0, a negative step), staged and per lane."""
    c = pwl_circuit((N,), name)
    lay = c.layers[0]
    assert len(lay.kept) == m
    log = _run(c, pwl_inputs((N,), lay, rounds=6), log=native, want=want_of(lay), relu="mrs")
    _check_log(log, _form(N))


@pytest.mark.parametrize("relu", ["approx", "mrs", "joint"])
def test_sign_constructions(native, relu):
    """conv -> Rescale(3) -> PiecewiseLinear (N = 272) under each sign construction; "joint" resolves to the exact
    sign for this layer (the rescale before it keeps its own output pass)."""
    c = conv_chain("m2")
    log = _run(c, conv_chain_inputs(rounds=6), log=native, **_KW[relu])
    _check_log(log, "staged")
    assert not any(l.startswith(("relu_out.", "leaky_out.")) for l in log)


@pytest.mark.parametrize("k,relu,N", [(2, "mrs", 272), (2, "mrs", 77), (12, "mrs", 272), (12, "mrs", 77),
                                      (4, "approx", 272), (9, "approx", 272)])
def test_base_sizes(native, k, relu, N):
    """The smallest and largest CRT bases of the host test (tests/test_pwl.py) for each sign construction."""
    name = shape_for(k, "m8")
    c = pwl_circuit((N,), name)
    lay = c.layers[0]
    mrs = 100.0 if 4 <= k <= 11 else None
    log = _run(c, pwl_inputs((N,), lay, k=k, rounds=6), crt=k, mrs=mrs, log=native, want=want_of(lay), **_KW[relu])
    _check_log(log, _form(N))


# ---------------------------------------------------------------- GPU garbler
@pytest.mark.parametrize("relu", ["approx", "mrs"])
@pytest.mark.parametrize("name", ["m2", "m8"])
def test_gpu_garbler_bit_identical(name, relu):
    """Per breakpoint the device folds T_i into the labels, runs the sign's and the half gates' passes on the
    breakpoint's stream slots and adds the output labels into the combination; the model and the decoder equal the
    host garbler's byte for byte."""
    g = _gpu_vs_host(conv_chain(name), 7, 100.0, **_KW[relu])
    assert g.model.layer_kind(2) == 21


def test_gpu_garbler_into_evaluator_slot():
    """The GPU garbler writes the tables straight into an evaluator slot (HipEvaluator.sink); both slots evaluate
    and decode."""
    from dash_amd.runtime import HipEvaluator

    c = conv_chain("m8")
    kw = _KW["mrs"]
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


# ---------------------------------------------------------------- end to end
def test_imported_sigmoid_gate_end_to_end(tmp_path):
    """The imported conv -> Rescale -> Sigmoid -> Mul (channel gate) -> conv chain, garbled on the GPU and run by
    the HIP evaluator, decodes to the plaintext quantized model."""
    from dash_amd.ir.onnx import load_onnx_model
    from dash_amd.runtime import HipEvaluator
    from tests.test_pwl import gate_onnx

    l, s = 3, 5  # l + s = 8: the GPU garbler's mixed-radix rescale stages a row of 2^(l + s + 1) entries in LDS
    c = load_onnx_model(gate_onnx(tmp_path), Q.ScaleQuant, l, pwl_bits=s)
    assert [x.name for x in c.layers].count("pwl") == 1 and c.layers[6].l == l + s
    rng = np.random.default_rng(3)
    xs = [np.round(rng.uniform(-1, 1, c.layers[0].in_size) * (1 << l)).astype(np.int64) for _ in range(2)]
    k = max(7, c.infer_crt_base_size(xs))
    M = crt_modulus(first_primes(k))
    assert k <= 9 and c.required_crt_modulus() <= M
    gcs = [GarbledCircuit(c, k, 100.0, seed=bytes([i + 1]) * 16, device=0, rescale="mrs", relu="mrs") for i in range(2)]
    ev = HipEvaluator([g.model for g in gcs])
    out = ev.evaluate([g.garble_inputs(x) for g, x in zip(gcs, xs)])
    for g, x, o in zip(gcs, xs, out):
        np.testing.assert_array_equal(g.decode_outputs(o), c.plain_q_eval(x, False, M))
