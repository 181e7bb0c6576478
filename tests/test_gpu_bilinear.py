"""The Bilinear layer on the GPU (docs/BILINEAR.md): the HIP evaluator's two forms (k_bilinear4, logged
bilinear.dword, and k_bilinear, bilinear.byte) bit-exact against the host evaluator with their launch grids written
out from the formulas, a base whose tap weights vanish mod a residue, graph replay, the GPU garbler byte-identical to
the host garbler (also into an evaluator slot) and both zoo models end to end. Circuits: tests/bilinear_cases.py.

The shapes are the smallest at which each form can go wrong:
  dword1080   (3, 9, 10) -> (3, 18, 20): the dword form; Nout = 1080 crosses the 1024-output block boundary with a
              partial last block, channel offsets, clamped border rows and columns
  byte_f2x3   (2, 3, 5) -> (2, 6, 15): OW % 4 != 0, the byte form; another factor per axis, fx = 3 non-dyadic
  one_row     (4, 1, 4) -> (4, 2, 8): a single input row, both row taps read it
  corners7x8  (1, 4, 4) -> (1, 7, 8), align_corners: a non-integer factor, weights of 0 and 2^b"""
import math

import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit
from tests.bilinear_cases import B3, BYTE, DWORD, M7, SHAPES, bilinear_circuit, conv_bilinear_conv, inputs, layer
from tests.test_gpu_matmul import _run
from tests.test_gpu_parity import _check, _gpu_vs_host, _same

pytestmark = pytest.mark.gpu

K, B = 7, 3  # residues of the base, GCs per evaluator in _check
NMAX = max(int(math.floor(128.0 / math.log2(p))) for p in (2, 3, 5, 7, 11, 13, 17))  # components of the widest label


def _want_log(form: str, nout: int, batch: int = B, k: int = K, nmax: int = NMAX) -> str:
    """dword: a lane owns 4 outputs, a block of 256 lanes 1024; byte: one lane per output and component row of the
    widest residue. Grid (x, residues, GCs)."""
    x = -(-nout // 1024) if form == "dword" else -(-nout * nmax // 256)
    return f"bilinear.{form} grid=({x},{k},{batch}) block=256"


def _logged(native, fn):
    native.hip_launch_log_take()
    native.hip_launch_log(True)
    try:
        out = fn()
    finally:
        native.hip_launch_log(False)
    return out, [l for l in native.hip_launch_log_take() if l.startswith("bilinear.")]


def _run_shape(native, name):
    c = bilinear_circuit(name)
    _, log = _logged(native, lambda: _check(c, K, 100.0, inputs(c, B), hardened=True))
    return log


@pytest.mark.parametrize("name", DWORD + BYTE)
def test_bilinear_shapes(native, name):
    """One layer, 3 GCs at k = 7: HIP labels == host labels bit for bit, decoded == plain_q_eval, and the rule: the
    dword form where OW % 4 == 0 (the buffers are 4-byte aligned), else the byte form. Residue 2 of the base sees
    vanishing tap weights in every shape (every even numerator is 0 there)."""
    l = layer(name)
    assert (l.OW % 4 == 0) == (name in DWORD)
    w = {int(a) * int(b) for a in set(l.ny) | {(1 << l.by) - int(v) for v in l.ny}
         for b in set(l.nx) | {(1 << l.bx) - int(v) for v in l.nx}}
    assert any(v % 2 == 0 for v in w) and any(v % 2 for v in w)
    log = _run_shape(native, name)
    print("\n".join(log))
    assert log == [_want_log("dword" if name in DWORD else "byte", l.out_size)], log


def test_dword1080_has_a_partial_second_block():
    l = layer("dword1080")
    assert l.out_size == 1080 and -(-l.out_size // 1024) == 2 and l.out_size % 1024 == 56
    assert 0 in l.ny and 0 in l.nx and l.y0[-1] == l.y1[-1] and l.x0[-1] == l.x1[-1]  # clamped borders
    c = layer("corners7x8")
    assert (c.by, c.bx) == (1, 6) and {0, 64} <= set(int(v) for v in c.nx) | {64 - int(v) for v in c.nx}


def test_form_coverage(native):
    """Both kernel forms are taken by the shapes above, read from the launch log of the evaluator's planned ops."""
    forms = {name: _run_shape(native, name)[0].split()[0] for name in SHAPES}
    assert set(forms.values()) == {"bilinear.dword", "bilinear.byte"}, forms
    assert forms["dword1080"] == "bilinear.dword" and forms["byte_f2x3"] == "bilinear.byte"


FORCED_BYTE_SCRIPT = """
import sys
sys.path.insert(0, {root!r})
from dash_amd.native import native
from tests.bilinear_cases import layer
from tests.test_gpu_bilinear import _run_shape, _want_log
log = _run_shape(native(), "dword1080")
assert log == [_want_log("byte", layer("dword1080").out_size)], log
print("same")
"""


def test_byte_form_on_the_dword_shape():
    """DASH_BILINEAR_FORM=byte (read when an evaluator is planned) forces the byte form on the first shape, in a child
    process: both forms compute the same labels."""
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = str(Path(__file__).resolve().parents[1])
    env = dict(os.environ, DASH_BILINEAR_FORM="byte")
    r = subprocess.run([sys.executable, "-c", FORCED_BYTE_SCRIPT.format(root=root)], capture_output=True, text=True,
                       timeout=120, env=env, cwd=root)
    assert r.returncode == 0 and r.stdout.strip().endswith("same"), r.stdout + r.stderr


@pytest.mark.parametrize("name", ["dword1080", "byte_f2x3"])
def test_base_5_7_131(native, name):
    """The base (5, 7, 131): a residue above 127 (label bytes and reduced weights up to 130, the accumulate's largest
    products) and other zero patterns of the reduced weights than at p = 2."""
    c = bilinear_circuit(name)
    xs = inputs(c, B, lim=1)
    assert all(np.abs(c.plain_q_eval(x, False)).max() < (5 * 7 * 131) // 2 for x in xs)
    _, log = _logged(native, lambda: _check(c, B3, None, xs, hardened=True))
    nmax = max(int(math.floor(128.0 / math.log2(p))) for p in B3)
    assert log == [_want_log("dword" if name in DWORD else "byte", c.output_size, k=3, nmax=nmax)], log


def test_graph_replay(native):
    """conv -> bilinear -> conv -> rescale -> relu, two GCs on a side stream: an eager round, a capturing one and a
    replay, each against the host evaluator and the plaintext."""
    rng = np.random.default_rng(6)
    c = conv_bilinear_conv(rng, factors=2)
    xs = [rng.integers(-3, 4, c.input_size) for _ in range(6)]
    log = _run(c, xs, log=native, rescale="mrs", relu="joint", hardened=True)
    assert [l.split()[0] for l in log if l.startswith("bilinear.")] == ["bilinear.byte"], log  # OW = 10


@pytest.mark.parametrize("case", ["upconv_byte", "dword_relu"])
def test_gpu_garbler_bit_identical(case, monkeypatch, capfd):
    """The layer garbles on the device through the evaluator's own kernels (GpuGarbler::bilinear_dev; the trace names
    it once per layer); the host garbler is the reference, byte for byte."""
    monkeypatch.setenv("DASH_GG_TRACE", "1")
    if case == "upconv_byte":
        c, kw = conv_bilinear_conv(np.random.default_rng(7), factors=(2, 3), bits=2), dict(rescale="mrs", relu="joint")
    else:
        bl = layer("dword1080")
        c, kw = d.Circuit([bl, d.Relu(bl.out_dims)]), {}
    g = _gpu_vs_host(c, K, 100.0, hardened=True, **kw)
    err = capfd.readouterr().err
    assert err.count("[gg] bilinear") == 1, err
    from dash_amd.runtime import HipEvaluator

    x = np.random.default_rng(8).integers(-3, 4, c.input_size)
    ev = HipEvaluator(template=g.model, batch=1, device=0)
    ev.load(0, g.model)
    ev.encode_compressed_into(0, g, x)
    ev.upload_inputs_compressed()
    ev.run()
    ev.fetch_outputs()
    np.testing.assert_array_equal(ev.decode(0, g), g.plain_q_eval(x))


def test_gpu_garbler_into_evaluator_slot():
    """The GPU garbler writes the tables of the rescale and ReLU behind the up-conv straight into an evaluator slot
    (HipEvaluator.sink); evaluate and decode both slots."""
    from dash_amd.runtime import HipEvaluator

    rng = np.random.default_rng(9)
    c = conv_bilinear_conv(rng, factors=2)
    xs = [rng.integers(-3, 4, c.input_size) for _ in range(2)]
    kw = dict(rescale="mrs", relu="joint", hardened=True)
    first = GarbledCircuit(c, K, 100.0, seed=bytes([7]) * 16, device=0, **kw)
    ev = HipEvaluator(template=first.model, batch=2, device=0)
    ev.load(0, first.model)
    seed = bytes(range(16))
    into = GarbledCircuit(c, K, 100.0, seed=seed, device=0, sink=ev.sink(1), **kw)
    host = GarbledCircuit(c, K, 100.0, seed=seed, **kw)
    assert _same(into.model.serialize(), host.model.serialize())
    ev.load(1, into.model)
    for b, gc in enumerate((first, into)):
        ev.encode_compressed_into(b, gc, xs[b])
    ev.upload_inputs_compressed()
    ev.run()
    ev.fetch_outputs()
    for b, gc in enumerate((first, into)):
        np.testing.assert_array_equal(ev.decode(b, gc), c.plain_q_eval(xs[b], False, M7))


@pytest.mark.parametrize("name", ["DEEPLAB_HEAD_CIFAR", "UNET_BILINEAR_CIFAR"])
def test_zoo_models_end_to_end(native, name):
    """Batch 1 through the GPU garbler and the HIP evaluator, equal to the plaintext quantized model: the consumed
    pending bits (Rescale(l + s) behind the up-conv) and the ArgMax on scaled scores. Every Bilinear of both models
    has OW % 4 == 0 and takes the dword form."""
    from dash_amd.ir.quant import QuantizationMethod as Q
    from dash_amd.models import BENCH_CONFIGS, build_circuit, quantized_inputs
    from dash_amd.runtime import HipEvaluator

    cfg = BENCH_CONFIGS[f"{name}/DASH"]
    c = build_circuit(name, Q.ScaleQuant, cfg["q_parameter"], seed=0)
    xs = quantized_inputs(name, 2, Q.ScaleQuant, cfg["q_parameter"], seed=7)
    c.calibrate(xs, M7)
    assert c.required_crt_modulus() <= M7
    gc = GarbledCircuit(c, cfg["crt"], cfg["mrs"], seed=bytes(range(16)), device=0)
    assert gc.hardened and gc.rescale == "mrs"
    ev = HipEvaluator(template=gc.model, batch=1, device=0)
    ev.load(0, gc.model)
    ev.encode_compressed_into(0, gc, xs[0])
    ev.upload_inputs_compressed()
    (_, log) = _logged(native, ev.run)
    ev.fetch_outputs()
    np.testing.assert_array_equal(ev.decode(0, gc), c.plain_q_eval(xs[0], False, M7))
    n = sum(l.name == "bilinear" for l in c.layers)
    assert n >= 1 and [l.split()[0] for l in log] == ["bilinear.dword"] * n, log
