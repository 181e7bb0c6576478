"""The ArgMax layer on the GPU: the HIP evaluator (k_argmax_mult's four level shapes) bit-exact against the host
evaluator over eager and graph-replayed rounds, the launch forms, the GPU garbler byte-identical to the host
garbler (also into an evaluator slot), the zoo model end to end and the range guard's torch path on the device
(docs/ARGMAX.md)."""
import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit, RangeGuard
from tests.test_argmax import M7, argmax_inputs, dense_argmax, guard_case, model_a_argmax
from tests.test_gpu_parity import _check, _gpu_vs_host, _same

pytestmark = pytest.mark.gpu


def _labels_equal(cpu, gpu):
    for c, g in zip(cpu, gpu):
        assert len(c) == len(g)
        for (pc, ac), (pg, ag) in zip(c, g):
            assert pc == pg
            np.testing.assert_array_equal(ac, ag)


def _run_argmax(dims, crt, mrs, M, plain=True, log=None, rounds=2):
    """Two GCs (different seeds) of one ArgMax layer on one evaluator, `rounds` rounds of two input vectors (the
    first run of an evaluator is eager, later runs replay the captured graph): labels bit-exact against the host
    evaluator and decoded outputs == plain_q_eval. Returns the launch log of the first round when `log` (the
    native module) is given."""
    from dash_amd.runtime import HipEvaluator

    c = d.Circuit([d.ArgMax(dims)])
    gcs = [GarbledCircuit(c, crt, mrs, seed=bytes([i + 1]) * 16) for i in range(2)]
    ev = HipEvaluator([g.model for g in gcs])
    xs = argmax_inputs(dims, M, rounds=2 * rounds)
    taken = None
    for r in range(0, len(xs), 2):
        pair = xs[r:r + 2]
        enc = [g.garble_inputs(x) for g, x in zip(gcs, pair)]
        cpu = [g.cpu_evaluate(e) for g, e in zip(gcs, enc)]
        if log is not None and r == 0:
            log.hip_launch_log_take()
            log.hip_launch_log(True)
            try:
                gpu = ev.evaluate(enc)
            finally:
                log.hip_launch_log(False)
            taken = log.hip_launch_log_take()
        else:
            gpu = ev.evaluate(enc)
        _labels_equal(cpu, gpu)
        if plain:
            for g, x, o in zip(gcs, pair, gpu):
                np.testing.assert_array_equal(g.decode_outputs(o), g.plain_q_eval(x))
                np.testing.assert_array_equal(g.plain_q_eval(x), np.argmax(x.reshape(dims[0], -1), axis=0))
    return taken


@pytest.mark.parametrize("dims", [(2,), (3,), (10,), (5, 7, 11), (2, 19, 27), (3, 20, 26)],
                         ids=lambda s: "x".join(map(str, s)))
def test_argmax_layer(dims):
    """One position with K = 2 (the root at level 0), 3 (a carried public index) and 10 (all four level shapes);
    (5, 7, 11): 77 positions, an odd carried slot at two levels, below a wave multiple; (2, 19, 27): 513 pair
    operations, one past a 512 tile, through the root-at-level-0 form; (3, 20, 26): 520 positions, the level-0
    and root forms past a tile. Ties and the extreme span sit on the first and last pair operations of a wave
    and of a tile (tests.test_argmax.argmax_inputs)."""
    _run_argmax(dims, 7, 100.0, M7)


def test_argmax_feeds_a_dense_layer():
    """The output is an ordinary label tensor in the layer's output buffer: a dense layer reads it (the parity
    suite's own helper, fresh evaluator, two GCs)."""
    rng = np.random.default_rng(4)
    c = d.Circuit([d.ArgMax((5, 2, 2)), d.Flatten((1, 2, 2)), d.Dense.from_quantized(rng.integers(-4, 5, (3, 4)), [1, 2, 3])])
    _check(c, 7, 100.0, argmax_inputs((5, 2, 2), M7), relu="mrs", rescale="auto")


def test_argmax_large_residue():
    """Activation bytes above 127 through the digit loops: the base [2, 131], labels only."""
    _run_argmax((3, 5, 5), [2, 131], None, 262, plain=False)


@pytest.mark.parametrize("dims,forms", [((2, 19, 27), ["root0"]), ((3, 20, 26), ["l0", "root"]),
                                        ((10, 1, 3), ["l0", "mid", "mid", "root"])],
                         ids=["K2", "K3", "K10"])
def test_argmax_mult_forms(native, dims, forms):
    """The launch log names k_argmax_mult's form at every level. Only the per-lane kernel exists (no staged
    form), so the planning CU count does not enter."""
    log = _run_argmax(dims, 7, 100.0, M7, log=native, rounds=1)
    print("\n".join(log))
    assert [l.split()[0] for l in log if l.startswith("argmax_mult.")] == ["argmax_mult." + f for f in forms], log


@pytest.mark.parametrize("case", ["dense_argmax", "5x7x11"])
def test_gpu_garbler_bit_identical_argmax(case, monkeypatch, capfd):
    """An ArgMax garbles on the device (GpuGarbler::argmax_level, one call per level: the trace names them); the
    host garbler is the reference. Dense -> ArgMax(10) has all four level shapes and a carried public index,
    (5, 7, 11) an odd carried slot at two levels."""
    from dash_amd.runtime import HipEvaluator

    monkeypatch.setenv("DASH_GG_TRACE", "1")

    rng = np.random.default_rng(3)
    if case == "dense_argmax":
        c, x = dense_argmax(rng), rng.integers(-20, 21, 12)
    else:
        c, x = d.Circuit([d.ArgMax((5, 7, 11))]), argmax_inputs((5, 7, 11), M7)[0]
    g = _gpu_vs_host(c, 7, 100.0)
    assert capfd.readouterr().err.count("[gg] argmax_level") == (4 if case == "dense_argmax" else 3)
    monkeypatch.delenv("DASH_GG_TRACE")
    ev = HipEvaluator(template=g.model, batch=1, device=0)
    ev.load(0, g.model)
    ev.encode_compressed_into(0, g, x)
    ev.upload_inputs_compressed()
    ev.run()
    ev.fetch_outputs()
    np.testing.assert_array_equal(ev.decode(0, g), g.plain_q_eval(x))


def test_gpu_garbler_argmax_into_evaluator_slot():
    """The GPU garbler writes an ArgMax's tables straight into an evaluator slot (HipEvaluator.sink); evaluate and
    decode both slots."""
    from dash_amd.runtime import HipEvaluator

    rng = np.random.default_rng(4)
    c = dense_argmax(rng)
    first = GarbledCircuit(c, 7, 100.0, seed=bytes([7]) * 16, device=0)
    ev = HipEvaluator(template=first.model, batch=2, device=0)
    ev.load(0, first.model)
    seed = bytes(range(16))
    into = GarbledCircuit(c, 7, 100.0, seed=seed, device=0, sink=ev.sink(1))
    host = GarbledCircuit(c, 7, 100.0, seed=seed)
    assert _same(into.model.serialize(), host.model.serialize())
    ev.load(1, into.model)
    xs = [rng.integers(-20, 21, 12) for _ in range(2)]
    for b, gc in enumerate((first, into)):
        ev.encode_compressed_into(b, gc, xs[b])
    ev.upload_inputs_compressed()
    ev.run()
    ev.fetch_outputs()
    for b, gc in enumerate((first, into)):
        np.testing.assert_array_equal(ev.decode(b, gc), gc.plain_q_eval(xs[b]))


def test_zoo_model_a_argmax():
    """MODEL_A_ARGMAX/SIMPLE with the GPU garbler and the HIP evaluator, batch 1: the decoded output is the class."""
    from dash_amd.runtime import HipEvaluator

    cfg, c, logits, xs = model_a_argmax()
    gc = GarbledCircuit(c, cfg["crt"], cfg["mrs"], seed=bytes(range(16)), device=0)
    ev = HipEvaluator(template=gc.model, batch=1, device=0)
    ev.load(0, gc.model)
    for x in xs:
        ev.encode_into(0, gc, x)
        ev.upload_inputs()
        ev.run()
        y = gc.decode_outputs(ev.get_outputs()[0])
        np.testing.assert_array_equal(y, gc.plain_q_eval(x))
        np.testing.assert_array_equal(y, [int(np.argmax(logits.plain_q_eval(x, False)))])


def test_range_guard_torch_path_on_device():
    c, xs, want = guard_case()
    g = RangeGuard(c, M7, mrs=True, device=0)
    assert not g._native_ok()  # guard.hip has no ArgMax: the batched torch path on the device
    assert g.submit(xs).bad_indices() == [i for i, x in enumerate(xs) if g.violations_np(x)] == \
        [i for i, w in enumerate(want) if w]
