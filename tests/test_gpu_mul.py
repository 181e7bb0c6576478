"""The Mul layer on the GPU: the HIP evaluator (k_mul, k_mul_s, k_mul_sq) bit-exact against the host evaluator over
eager and graph-replayed rounds, the launch forms, the GPU garbler byte-identical to the host garbler (also into an
evaluator slot), the tiny SE and square architectures end to end and the range guard's torch path on the device
(docs/MUL.md). Circuits and inputs: tests/mul_cases.py."""
import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit, RangeGuard
from tests.mul_cases import M7, TINY_SE, TINY_SQUARE, expected, guard_case, mul_circuit, mul_inputs, tiny_arch
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


def _run_case(dims, kind, log=None, rounds=3):
    return _run(mul_circuit(dims, kind), mul_inputs(dims, kind, rounds=2 * rounds), log=log,
                want=lambda x: expected(dims, kind, x))


ELEM = [(1,), (77,), (256,), (260,), (272,)]
BCAST = [((3, 1, 1), "bc3"), ((5, 4, 20), "bc1"), ((3, 20, 26), "bc3")]


@pytest.mark.parametrize("dims", ELEM, ids=lambda s: "x".join(map(str, s)))
def test_mul_elementwise(dims):
    """(1,); (77,) below two waves; (256,) exactly one staged tile; (260,) past a tile with N % 16 != 0, the lane
    form; (272,) staged with a partial last tile."""
    _run_case(dims, "elem")


@pytest.mark.parametrize("dims,kind", BCAST, ids=["3x1x1", "5x4x20", "3x20x26"])
def test_mul_broadcast(dims, kind):
    """(3, 1, 1) x (3, 1, 1): bc = 1 through the broadcast constructor; (5, 4, 20) with (5,): N = 400, staged, a
    tile that crosses the channel boundaries at 80, 160, 240, 320; (3, 20, 26) with (3, 1, 1): N = 1560, N % 16 != 0,
    channel boundary at 520."""
    c = mul_circuit(dims, kind)
    assert c.layers[1].bc == int(np.prod(dims[1:]))
    _run_case(dims, kind)


@pytest.mark.parametrize("dims", [(77,), (272,)], ids=["77", "272"])
def test_mul_square(dims):
    _run_case(dims, "sq")


def test_mul_operand_is_the_circuit_input():
    """y = the circuit input (src = -1), x = a permutation of it through a dense layer."""
    N = 40
    rng = np.random.default_rng(2)
    perm = rng.permutation(N)
    w = np.zeros((N, N), dtype=np.int64)
    w[np.arange(N), perm] = 1
    c = d.Circuit([d.Dense.from_quantized(w, np.zeros(N, dtype=np.int64)), d.Mul((N,), -1)])
    _run(c, mul_inputs((N,), "sq", rounds=6), want=lambda x: x[perm] * x)


def test_mul_operand_from_three_layers_back():
    """y = the output of layer 0, x three layers later with a conv in between: the saved buffer survives the layers
    that reuse the ping-pong buffers, eagerly and under graph replay."""
    rng = np.random.default_rng(3)
    conv0 = d.Conv2d.from_quantized(rng.integers(-2, 3, (2, 2, 1, 1)), rng.integers(-2, 3, 2), 4, 4, 2, 2, 1, 1, 1, 1)
    conv1 = d.Conv2d.from_quantized(rng.integers(-2, 3, (2, 2, 3, 3)), rng.integers(-2, 3, 2), 4, 4, 2, 2, 3, 3, 1, 1,
                                    pad_width=1, pad_height=1)
    c = d.Circuit([conv0, conv1, d.Flatten((2, 4, 4)), d.Mul((32,), 0)])
    xs = [rng.integers(-4, 5, 32) for _ in range(6)]
    _run(c, xs, want=lambda x: c.layers[1].plain_q_eval(c.layers[0].plain_q_eval(x, False), False) *
         c.layers[0].plain_q_eval(x, False))


@pytest.mark.parametrize("dims,kind", [((272,), "elem"), ((3, 5, 7), "bc1"), ((77,), "sq")], ids=["elem", "bc", "sq"])
def test_mul_large_residue(dims, kind):
    """Activation bytes above 127 through the digit loops: the base [2, 131] (M = 262; operands up to 11), labels
    only."""
    _run(mul_circuit(dims, kind), mul_inputs(dims, kind, rounds=6, lim=11), crt=[2, 131], mrs=None, plain=False)


@pytest.mark.parametrize("dims,kind,form", [((1,), "elem", "lane"), ((77,), "elem", "lane"), ((256,), "elem", "staged"),
                                            ((260,), "elem", "lane"), ((272,), "elem", "staged"),
                                            ((3, 1, 1), "bc3", "lane"), ((5, 4, 20), "bc1", "staged"),
                                            ((3, 20, 26), "bc3", "lane"), ((77,), "sq", "sq"), ((272,), "sq", "sq")])
def test_mul_launch_forms(native, dims, kind, form):
    """mult_grid's rule: staged where N % 16 == 0 and N >= 256 (the output is always apart from the input), else
    the lane form; a square has the one form."""
    log = _run_case(dims, kind, log=native, rounds=1)
    print("\n".join(log))
    assert [l.split()[0] for l in log if l.startswith("mul.")] == ["mul." + form], log


@pytest.mark.parametrize("dims,kind", [((272,), "elem"), ((5, 4, 20), "bc1"), ((3, 20, 26), "bc3"), ((77,), "sq")],
                         ids=["elem", "bc1", "bc3", "sq"])
def test_gpu_garbler_bit_identical_mul(dims, kind, monkeypatch, capfd):
    """A Mul garbles on the device (GpuGarbler::mul; the trace names it once per layer); the host garbler is the
    reference. Then the device-garbled model evaluates to the product."""
    from dash_amd.runtime import HipEvaluator

    monkeypatch.setenv("DASH_GG_TRACE", "1")
    c = mul_circuit(dims, kind)
    g = _gpu_vs_host(c, 7, 100.0)
    assert capfd.readouterr().err.count("[gg] mul") == 1
    monkeypatch.delenv("DASH_GG_TRACE")
    x = mul_inputs(dims, kind)[0]
    ev = HipEvaluator(template=g.model, batch=1, device=0)
    ev.load(0, g.model)
    ev.encode_compressed_into(0, g, x)
    ev.upload_inputs_compressed()
    ev.run()
    ev.fetch_outputs()
    np.testing.assert_array_equal(ev.decode(0, g), expected(dims, kind, x))


@pytest.mark.parametrize("dims,kind", [((5, 4, 20), "bc1"), ((77,), "sq")], ids=["bc", "sq"])
def test_gpu_garbler_mul_into_evaluator_slot(dims, kind):
    """The GPU garbler writes a Mul's tables straight into an evaluator slot (HipEvaluator.sink); evaluate and
    decode both slots."""
    from dash_amd.runtime import HipEvaluator

    c = mul_circuit(dims, kind)
    first = GarbledCircuit(c, 7, 100.0, seed=bytes([7]) * 16, device=0)
    ev = HipEvaluator(template=first.model, batch=2, device=0)
    ev.load(0, first.model)
    seed = bytes(range(16))
    into = GarbledCircuit(c, 7, 100.0, seed=seed, device=0, sink=ev.sink(1))
    host = GarbledCircuit(c, 7, 100.0, seed=seed)
    assert _same(into.model.serialize(), host.model.serialize())
    ev.load(1, into.model)
    xs = mul_inputs(dims, kind)
    for b, gc in enumerate((first, into)):
        ev.encode_compressed_into(b, gc, xs[b])
    ev.upload_inputs_compressed()
    ev.run()
    ev.fetch_outputs()
    for b, gc in enumerate((first, into)):
        np.testing.assert_array_equal(ev.decode(b, gc), expected(dims, kind, xs[b]))


@pytest.mark.parametrize("arch", ["se", "square"])
def test_tiny_arch_end_to_end(arch):
    """GPU garbler plus HIP evaluator at batch 2 over three rounds on a side stream (eager, graph capture, graph
    replay), equal to the plaintext quantized model."""
    import torch

    from dash_amd.runtime import HipEvaluator

    c, xs = tiny_arch("_TINY_MUL_GPU", TINY_SE if arch == "se" else TINY_SQUARE, n_inputs=6)
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


HOST_MUL_SCRIPT = """
import hashlib, sys
sys.path.insert(0, {root!r})
from dash_amd.garbling import GarbledCircuit
from tests.mul_cases import mul_circuit
for dims, kind in (((5, 4, 20), "bc1"), ((77,), "elem")):
    c = mul_circuit(dims, kind)
    seed = bytes(range(16))
    dev = GarbledCircuit(c, 7, 100.0, seed=seed, device=0)
    host = GarbledCircuit(c, 7, 100.0, seed=seed)
    a, b = bytes(dev.model.serialize()), bytes(host.model.serialize())
    assert len(a) == len(b) and hashlib.sha256(a).digest() == hashlib.sha256(b).digest(), (dims, kind)
    assert bytes(dev.decoder.serialize()) == bytes(host.decoder.serialize())
print("same")
"""


def test_host_garbled_mul_with_device_saved_operand():
    """DASH_GG_HARD=0 keeps the hardened gadget layers on the host garbler while the linear layers and the saved
    outputs stay on the device: the Mul's operand is fetched from its device copy. The switch is read once per
    process, so this runs in a child; the result is byte-identical to the all-host garbler."""
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = str(Path(__file__).resolve().parents[1])
    env = dict(os.environ, DASH_GG_HARD="0", DASH_GG_TRACE="1")
    r = subprocess.run([sys.executable, "-c", HOST_MUL_SCRIPT.format(root=root)], capture_output=True, text=True,
                       timeout=120, env=env, cwd=root)
    assert r.returncode == 0 and r.stdout.strip().endswith("same"), r.stdout + r.stderr
    assert "[gg] mul" not in r.stderr and "[gg] dense" in r.stderr  # the Mul on the host, the dense layer on the device


def test_range_guard_torch_path_on_device():
    c, xs, want = guard_case()
    g = RangeGuard(c, M7, mrs=True, device=0)
    assert not g._native_ok()  # guard.hip has no Mul: the batched torch path on the device
    assert g.submit(xs).bad_indices() == [i for i, x in enumerate(xs) if g.violations_np(x)] == \
        [i for i, w in enumerate(want) if w]
