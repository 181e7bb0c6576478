"""The Gather layer on the GPU (docs/GATHER.md): the HIP evaluator's two forms (k_gather4, logged gather.dword, and
the byte kernel, gather.byte) bit-exact against the host evaluator over an eager, a capturing and a replaying round,
their launch grids written out from the formulas, the in_src source read in place, the layer behind an ArgMax and
in front of a ReLU, the GPU garbler byte-identical to the host garbler (also into an evaluator slot) and both zoo
models end to end. Circuits and inputs: tests/gather_cases.py."""
import numpy as np
import pytest

from dash_amd.garbling import GarbledCircuit
from tests.gather_cases import (BYTE, DWORD, M7, SHAPES, argmax_case, gather_circuit, gather_index, gather_inputs,
                                in_src_case, repeats_relu_case, shuffle_unit_case)
from tests.test_gpu_matmul import _run
from tests.test_gpu_parity import _gpu_vs_host, _same

pytestmark = pytest.mark.gpu

K, B = 7, 2  # residues of the base, GCs per evaluator in _run


def _nmax() -> int:
    """The widest label of the k = 7 base in components, read off the host label format [N, n_p]."""
    gc = GarbledCircuit(gather_circuit("odd3"), K, 100.0, seed=bytes(16))
    return max(np.asarray(a).shape[1] for _, a in gc.garble_inputs(gather_inputs("odd3")[0]))


def _want_log(form: str, nout: int, batch: int = B) -> str:
    """dword: a lane owns 4 outputs, a block of 256 lanes 1024; byte: one lane per output and component row of the
    widest residue. Grid (x, residues, GCs)."""
    x = -(-nout // 1024) if form == "dword" else -(-nout * _nmax() // 256)
    return f"gather.{form} grid=({x},{K},{batch}) block=256"


def _run_shape(name, log=None):
    idx = gather_index(name)
    return _run(gather_circuit(name), gather_inputs(name), log=log, want=lambda x: np.asarray(x)[idx])


def _gather_lines(log):
    return [l for l in log if l.startswith("gather.")]


@pytest.mark.parametrize("name", DWORD + BYTE)
def test_gather_shapes(native, name):
    """The rule: the dword form where Nout % 4 == 0 (the buffers are 4-byte aligned), else the byte form. Three rounds
    of two GCs on a side stream: eager, capture and launch, replay."""
    log = _run_shape(name, log=native)
    print("\n".join(log))
    assert _gather_lines(log) == [_want_log("dword" if name in DWORD else "byte", SHAPES[name][1])], log


FORCED_BYTE_SCRIPT = """
import sys
sys.path.insert(0, {root!r})
from dash_amd.native import native
from tests.gather_cases import SHAPES
from tests.test_gpu_gather import _gather_lines, _run_shape, _want_log
for name in {names!r}:
    log = _run_shape(name, log=native())
    assert _gather_lines(log) == [_want_log("byte", SHAPES[name][1])], log
print("same")
"""


def test_byte_form_on_the_dword_shapes():
    """DASH_GATHER_FORM=byte (read when an evaluator is planned) forces the byte form on the dword shapes, in a child
    process: both forms compute the same labels."""
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = str(Path(__file__).resolve().parents[1])
    env = dict(os.environ, DASH_GATHER_FORM="byte")
    r = subprocess.run([sys.executable, "-c", FORCED_BYTE_SCRIPT.format(root=root, names=list(DWORD))],
                       capture_output=True, text=True, timeout=120, env=env, cwd=root)
    assert r.returncode == 0 and r.stdout.strip().endswith("same"), r.stdout + r.stderr


def test_in_src_is_read_in_place(native):
    """Conv -> Relu -> Gather(in_src = the conv) -> Add: the Gather reads the conv's saved copy where it lies. The op
    list has the two saved outputs (the conv for the Gather, the Relu for the Add; one save op per residue) and no
    restore."""
    from dash_amd.runtime import HipEvaluator

    c, xs, want = in_src_case()
    log = _run(c, xs, want=want, log=native)
    assert _gather_lines(log) == [_want_log("dword", 32)], log
    gcs = [GarbledCircuit(c, K, 100.0, seed=bytes([i + 1]) * 16) for i in range(2)]
    ev = HipEvaluator([g.model for g in gcs], profile=True)
    ev.evaluate([g.garble_inputs(x) for g, x in zip(gcs, xs)])
    names = [n for n, _ in ev.op_times()]
    print(names)
    assert "restore" not in names and names.count("save") == 2 * K and names.count("gather#2") == 1


def test_shuffle_unit():
    c, xs = shuffle_unit_case()
    _run(c, xs)


def test_behind_an_argmax():
    c, xs, want = argmax_case()
    _run(c, xs, want=want)


def test_repeats_in_front_of_a_relu(native):
    c, xs, want = repeats_relu_case()
    log = _run(c, xs, want=want, log=native)
    assert _gather_lines(log) == [_want_log("dword", 12)], log


def test_reference_encoding():
    c, xs, want = in_src_case()
    _run(c, xs, want=want, hardened=False)


@pytest.mark.parametrize("case", ["perm1024", "rep1028", "odd1025", "in_src", "argmax"])
def test_gpu_garbler_bit_identical_gather(case, monkeypatch, capfd):
    """A Gather garbles on the device (GpuGarbler::gather_dev; the trace names it once per layer), an in_src source
    from the device copy the garbler keeps; the host garbler is the reference."""
    monkeypatch.setenv("DASH_GG_TRACE", "1")
    c = {"in_src": lambda: in_src_case()[0], "argmax": lambda: argmax_case()[0]}.get(case, lambda: gather_circuit(case))()
    _gpu_vs_host(c, K, 100.0)
    err = capfd.readouterr().err
    assert err.count("[gg] gather") == 1, err


def test_gpu_garbler_gather_into_evaluator_slot():
    """The GPU garbler writes the tables of the ReLU behind a Gather with repeats straight into an evaluator slot
    (HipEvaluator.sink); evaluate and decode both slots."""
    from dash_amd.runtime import HipEvaluator

    c, xs, want = repeats_relu_case()
    first = GarbledCircuit(c, K, 100.0, seed=bytes([7]) * 16, device=0)
    ev = HipEvaluator(template=first.model, batch=2, device=0)
    ev.load(0, first.model)
    seed = bytes(range(16))
    into = GarbledCircuit(c, K, 100.0, seed=seed, device=0, sink=ev.sink(1))
    host = GarbledCircuit(c, K, 100.0, seed=seed)
    assert _same(into.model.serialize(), host.model.serialize())
    ev.load(1, into.model)
    for b, gc in enumerate((first, into)):
        ev.encode_compressed_into(b, gc, xs[b])
    ev.upload_inputs_compressed()
    ev.run()
    ev.fetch_outputs()
    for b, gc in enumerate((first, into)):
        np.testing.assert_array_equal(ev.decode(b, gc), want(xs[b]))


@pytest.mark.parametrize("name", ["SHUFFLENET_V2_CIFAR", "SUBPIXEL_SEG_CIFAR"])
def test_zoo_models_end_to_end(native, name):
    """Batch 1 through the GPU garbler and the HIP evaluator, equal to the plaintext quantized model; every Gather of
    both models has Nout % 4 == 0 and takes the dword form."""
    from dash_amd.ir.quant import QuantizationMethod as Q
    from dash_amd.models import build_circuit, quantized_inputs
    from dash_amd.runtime import HipEvaluator

    c = build_circuit(name, Q.ScaleQuant, 5, seed=0)
    xs = quantized_inputs(name, 2, Q.ScaleQuant, 5, seed=7)
    c.calibrate(xs, M7)
    assert c.required_crt_modulus() <= M7
    gc = GarbledCircuit(c, K, 100.0, seed=bytes(range(16)), device=0)
    ev = HipEvaluator(template=gc.model, batch=1, device=0)
    ev.load(0, gc.model)
    ev.encode_compressed_into(0, gc, xs[0])
    ev.upload_inputs_compressed()
    native.hip_launch_log_take()
    native.hip_launch_log(True)
    try:
        ev.run()
    finally:
        native.hip_launch_log(False)
    log = native.hip_launch_log_take()
    ev.fetch_outputs()
    np.testing.assert_array_equal(ev.decode(0, gc), c.plain_q_eval(xs[0], False, M7))
    n_gather = sum(l.name == "gather" for l in c.layers)
    assert n_gather >= 1 and [l.split()[0] for l in _gather_lines(log)] == ["gather.dword"] * n_gather, log
