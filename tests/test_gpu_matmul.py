"""The MatMul layer on the GPU: the HIP evaluator (the key pre-pass, k_matmul and k_matmul_b) bit-exact against the
host evaluator over eager and graph-replayed rounds, the launch forms at their tile edges, the GPU garbler
byte-identical to the host garbler (also into an evaluator slot), the tiny non-local architecture end to end and the
range guard's torch path on the device (docs/MATMUL.md). Circuits and inputs: tests/matmul_cases.py."""
import itertools

import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit, RangeGuard
from tests.matmul_cases import (M7, TINY_NONLOCAL, expected, gram_circuit, gram_expected, gram_inputs, guard_case, lim_of,
                                matmul_circuit, matmul_inputs, tiny_arch)
from tests.test_gpu_parity import _gpu_vs_host, _same

pytestmark = pytest.mark.gpu


def _labels_equal(cpu, gpu):
    for c, g in zip(cpu, gpu):
        assert len(c) == len(g)
        for (pc, ac), (pg, ag) in zip(c, g):
            assert pc == pg
            np.testing.assert_array_equal(ac, ag)


def _run(c, xs, crt=7, mrs=100.0, plain=True, want=None, log=None, **kw):
    """Two GCs (different seeds) of circuit c on one evaluator, one round per pair of xs, all on one side stream:
    the evaluator runs eagerly the first time and replays a captured hipGraph from its second run on a non-null
    stream (the second round captures and launches, a third only launches). Labels bit-exact against the host
    evaluator, decoded outputs == plain_q_eval (and == want(x)). Returns the first round's launch log when `log`
    (the native module) is given."""
    import torch

    from dash_amd.runtime import HipEvaluator

    gcs = [GarbledCircuit(c, crt, mrs, seed=bytes([i + 1]) * 16, **kw) for i in range(2)]
    ev = HipEvaluator([g.model for g in gcs])
    st = torch.cuda.Stream()
    assert st.cuda_stream != 0  # the null stream never replays
    taken = None
    for r in range(0, len(xs), 2):
        pair = xs[r:r + 2]
        enc = [g.garble_inputs(x) for g, x in zip(gcs, pair)]
        cpu = [g.cpu_evaluate(e) for g, e in zip(gcs, enc)]
        if log is not None and r == 0:
            log.hip_launch_log_take()
            log.hip_launch_log(True)
            try:
                gpu = ev.evaluate(enc, st)
            finally:
                log.hip_launch_log(False)
            taken = log.hip_launch_log_take()
        else:
            gpu = ev.evaluate(enc, st)
        _labels_equal(cpu, gpu)
        if plain:
            for g, x, o in zip(gcs, pair, gpu):
                y = g.decode_outputs(o)
                np.testing.assert_array_equal(y, g.plain_q_eval(x))
                if want is not None:
                    np.testing.assert_array_equal(y, want(x))
    return taken


def _run_case(M, T, N, ta=False, tb=False, log=None, rounds=3):
    return _run(matmul_circuit(M, T, N, ta, tb), matmul_inputs(M, T, N, ta, tb, rounds=2 * rounds), log=log,
                want=lambda x: expected(M, T, N, x, ta, tb))


SHAPES = [((1, 1, 1), "lane"), ((1, 5, 1), "lane"), ((3, 1, 4), "lane"), ((7, 3, 11), "lane"), ((15, 2, 17), "lane"),
          ((16, 2, 16), "blocked"), ((13, 4, 20), "lane"),
          ((15, 3, 16), "lane"), ((17, 3, 16), "blocked"), ((16, 3, 15), "lane"), ((16, 3, 17), "blocked"),
          ((16, 15, 16), "blocked"), ((16, 16, 16), "blocked"), ((16, 17, 16), "blocked"), ((33, 18, 35), "blocked")]


@pytest.mark.parametrize("shape,form", SHAPES, ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else s)
def test_matmul_shapes(native, shape, form):
    """(1, 1, 1); (1, 5, 1) a dot product; (3, 1, 4) T = 1; (7, 3, 11) 77 outputs, below two waves. The lane form
    (matmul.lane) has one tile edge, its block of 256 outputs: (15, 2, 17) has 255, just below it, and (13, 4, 20)
    260, past it; (16, 2, 16), exactly 256, is one full tile of the blocked form (matmul.blocked), which the planner
    picks where M >= I = 16 and N >= L = 16. I: (15, 3, 16) just below (lane), (16, 2, 16) at, (17, 3, 16) just above
    (a second tile row of one live row). L: (16, 3, 15) just below (lane), (16, 2, 16) at, (16, 3, 17) just above (a
    second tile column of one live column). The t chunk of 16: (16, 15, 16) just below, (16, 16, 16) at, (16, 17, 16)
    just above (a second chunk of one product). (33, 18, 35): 3 x 3 tiles with partial last tiles and two chunks."""
    log = _run_case(*shape, log=native)
    print("\n".join(log))
    forms = [l.split() for l in log if l.startswith("matmul.")]
    assert [f[0] for f in forms] == ["matmul." + form], log


@pytest.mark.parametrize("form", ["lane", "blocked"])
def test_matmul_forms_agree_off_their_rule(form):
    """Each form is correct for every shape: DASH_MATMUL_FORM (read when an evaluator is planned) forces the lane
    form on a tiled shape and the blocked form on shapes thinner than a tile, in a child process each."""
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = str(Path(__file__).resolve().parents[1])
    shapes = [(16, 17, 16), (33, 18, 35)] if form == "lane" else [(1, 5, 1), (7, 3, 11), (13, 4, 20)]
    code = FORCED_FORM_SCRIPT.format(root=root, shapes=shapes, form=form)
    env = dict(os.environ, DASH_MATMUL_FORM=form)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env, cwd=root)
    assert r.returncode == 0 and r.stdout.strip().endswith("same"), r.stdout + r.stderr


FORCED_FORM_SCRIPT = """
import sys
sys.path.insert(0, {root!r})
from dash_amd.native import native
from tests.test_gpu_matmul import _run_case
for shape in {shapes!r}:
    log = _run_case(*shape, log=native())
    assert [l.split()[0] for l in log if l.startswith("matmul.")] == ["matmul.{form}"], log
print("same")
"""


@pytest.mark.parametrize("ta,tb", list(itertools.product([False, True], [False, True])), ids=["nn", "nt", "tn", "tt"])
def test_matmul_transposes(ta, tb):
    _run_case(5, 3, 7, ta, tb)


def test_matmul_gram():
    """x x^T: src is the layer's own input (with trans_b), which the kernel reads from the current activation."""
    _run(gram_circuit(6, 5), gram_inputs(6, 5, rounds=6), want=lambda x: gram_expected(6, 5, x))


def test_matmul_operand_is_the_circuit_input():
    """y = the circuit input (src = -1) as a 3 x 8 matrix, x = a permutation of it through a dense layer as 4 x 3."""
    M, T, N = 4, 3, 8
    rng = np.random.default_rng(2)
    sel = rng.permutation(T * N)[:M * T]
    w = np.zeros((M * T, T * N), dtype=np.int64)
    w[np.arange(M * T), sel] = 1
    c = d.Circuit([d.Dense.from_quantized(w, np.zeros(M * T, dtype=np.int64)), d.MatMul((M, T), -1, (T, N))])
    lim = lim_of(T)
    xs = [rng.integers(-lim, lim + 1, T * N) for _ in range(6)]
    _run(c, xs, want=lambda x: (x[sel].reshape(M, T) @ x.reshape(T, N)).reshape(-1))


def test_matmul_operand_from_three_layers_back():
    """y = the output of layer 0, x three layers later with a conv in between: the saved buffer survives the layers
    that reuse the ping-pong buffers, eagerly and under graph replay."""
    rng = np.random.default_rng(3)
    conv0 = d.Conv2d.from_quantized(rng.integers(-2, 3, (2, 2, 1, 1)), rng.integers(-2, 3, 2), 4, 4, 2, 2, 1, 1, 1, 1)
    conv1 = d.Conv2d.from_quantized(rng.integers(-2, 3, (2, 2, 3, 3)), rng.integers(-2, 3, 2), 4, 4, 2, 2, 3, 3, 1, 1,
                                    pad_width=1, pad_height=1)
    # x = conv1's output as 2 x 16, y = conv0's output (2, 4, 4) transposed to 16 x 2
    c = d.Circuit([conv0, conv1, d.Flatten((2, 4, 4)), d.MatMul((2, 16), 0, (2, 4, 4), trans_b=True)])
    xs = [rng.integers(-4, 5, 32) for _ in range(6)]

    def want(x):
        y = c.layers[0].plain_q_eval(x, False)
        a = c.layers[1].plain_q_eval(y, False)
        return (a.reshape(2, 16) @ y.reshape(2, 16).T).reshape(-1)

    _run(c, xs, want=want)


def test_matmul_large_residue():
    """Activation bytes above 127 through the digit loops: the base [2, 131] (M = 262; T = 3, operands up to 6),
    labels only."""
    lim = lim_of(3, 262)
    assert lim == 6
    _run(matmul_circuit(5, 3, 7), matmul_inputs(5, 3, 7, rounds=6, lim=lim), crt=[2, 131], mrs=None, plain=False)


@pytest.mark.parametrize("shape,ta,tb", [((13, 4, 20), False, False), ((5, 3, 7), True, True), ((5, 3, 7), True, False),
                                         ((3, 37, 4), False, True), ((1, 1, 1), False, False)],
                         ids=["260", "tt", "tn", "T37", "1"])
def test_gpu_garbler_bit_identical_matmul(shape, ta, tb, monkeypatch, capfd):
    """A MatMul garbles on the device (GpuGarbler::matmul_dev; the trace names it once per layer): the operands
    gathered per product, Mul's projections, the segmented sum (T = 37: three groups of at most 16 terms); the host
    garbler is the reference. Then the device-garbled model evaluates to the product."""
    from dash_amd.runtime import HipEvaluator

    monkeypatch.setenv("DASH_GG_TRACE", "1")
    c = matmul_circuit(*shape, ta, tb)
    g = _gpu_vs_host(c, 7, 100.0)
    err = capfd.readouterr().err
    assert err.count("[gg] matmul") == 1 and "[gg] mul" not in err
    monkeypatch.delenv("DASH_GG_TRACE")
    x = matmul_inputs(*shape, ta, tb)[0]
    ev = HipEvaluator(template=g.model, batch=1, device=0)
    ev.load(0, g.model)
    ev.encode_compressed_into(0, g, x)
    ev.upload_inputs_compressed()
    ev.run()
    ev.fetch_outputs()
    np.testing.assert_array_equal(ev.decode(0, g), expected(*shape, x, ta, tb))


def test_gpu_garbler_gram_bit_identical():
    """x x^T on the device garbler: both gathers read the one saved tensor."""
    _gpu_vs_host(gram_circuit(6, 5), 7, 100.0)


def test_gpu_garbler_matmul_into_evaluator_slot():
    """The GPU garbler writes a MatMul's tables straight into an evaluator slot (HipEvaluator.sink); evaluate and
    decode both slots."""
    from dash_amd.runtime import HipEvaluator

    shape = (7, 3, 11)
    c = matmul_circuit(*shape)
    first = GarbledCircuit(c, 7, 100.0, seed=bytes([7]) * 16, device=0)
    ev = HipEvaluator(template=first.model, batch=2, device=0)
    ev.load(0, first.model)
    seed = bytes(range(16))
    into = GarbledCircuit(c, 7, 100.0, seed=seed, device=0, sink=ev.sink(1))
    host = GarbledCircuit(c, 7, 100.0, seed=seed)
    assert _same(into.model.serialize(), host.model.serialize())
    ev.load(1, into.model)
    xs = matmul_inputs(*shape)
    for b, gc in enumerate((first, into)):
        ev.encode_compressed_into(b, gc, xs[b])
    ev.upload_inputs_compressed()
    ev.run()
    ev.fetch_outputs()
    for b, gc in enumerate((first, into)):
        np.testing.assert_array_equal(ev.decode(b, gc), expected(*shape, xs[b]))


def test_tiny_nonlocal_end_to_end():
    """GPU garbler (both MatMuls on the device) plus the HIP evaluator at batch 2 over three rounds on a side stream (eager, graph
    capture, graph replay), equal to the plaintext quantized model."""
    import torch

    from dash_amd.runtime import HipEvaluator

    c, xs = tiny_arch("_TINY_NONLOCAL_GPU", TINY_NONLOCAL, n_inputs=6)
    gcs = [GarbledCircuit(c, 7, 100.0, seed=bytes([i + 3]) * 16, device=0) for i in range(2)]
    host = GarbledCircuit(c, 7, 100.0, seed=bytes([3]) * 16)
    assert _same(gcs[0].model.serialize(), host.model.serialize())
    ev = HipEvaluator(template=gcs[0].model, batch=2, device=0)
    for b, gc in enumerate(gcs):
        ev.load(b, gc.model)
    st = torch.cuda.Stream()
    for r in range(3):
        for b, gc in enumerate(gcs):
            ev.encode_compressed_into(b, gc, xs[2 * r + b])
        ev.upload_inputs_compressed(st)
        ev.run(st)
        ev.fetch_outputs(st)
        for b, gc in enumerate(gcs):
            np.testing.assert_array_equal(ev.decode(b, gc), c.plain_q_eval(xs[2 * r + b], False, M7))


HOST_MATMUL_SCRIPT = """
import hashlib, sys
sys.path.insert(0, {root!r})
from dash_amd.garbling import GarbledCircuit
from tests.matmul_cases import gram_circuit, matmul_circuit
for c in (matmul_circuit(7, 3, 11), matmul_circuit(5, 3, 7, True, True), gram_circuit(6, 5)):
    seed = bytes(range(16))
    dev = GarbledCircuit(c, 7, 100.0, seed=seed, device=0)
    host = GarbledCircuit(c, 7, 100.0, seed=seed)
    a, b = bytes(dev.model.serialize()), bytes(host.model.serialize())
    assert len(a) == len(b) and hashlib.sha256(a).digest() == hashlib.sha256(b).digest(), c
    assert bytes(dev.decoder.serialize()) == bytes(host.decoder.serialize())
print("same")
"""


def test_host_garbled_matmul_with_device_saved_operand():
    """DASH_GG_HARD=0 keeps the hardened gadget layers on the host garbler while the linear layers and the saved
    outputs stay on the device: the MatMul's operand is fetched from its device copy. The switch is read once per
    process, so this runs in a child; the result is byte-identical to the all-host garbler."""
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = str(Path(__file__).resolve().parents[1])
    env = dict(os.environ, DASH_GG_HARD="0", DASH_GG_TRACE="1")
    r = subprocess.run([sys.executable, "-c", HOST_MATMUL_SCRIPT.format(root=root)], capture_output=True, text=True,
                       timeout=120, env=env, cwd=root)
    assert r.returncode == 0 and r.stdout.strip().endswith("same"), r.stdout + r.stderr
    assert "[gg] matmul" not in r.stderr and "[gg] dense" in r.stderr  # the MatMul on the host, the dense on the device


def test_range_guard_torch_path_on_device():
    c, xs, want = guard_case()
    g = RangeGuard(c, M7, mrs=True, device=0)
    assert not g._native_ok()  # guard.hip has no MatMul: the batched torch path on the device
    assert g.submit(xs).bad_indices() == [i for i, x in enumerate(xs) if g.violations_np(x)] == \
        [i for i, w in enumerate(want) if w]
