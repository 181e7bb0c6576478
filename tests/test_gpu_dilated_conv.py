"""Dilated Conv2d on the GPU: the HIP evaluator's dilated kernel forms bit-exact against the host evaluator, the form
each layer takes read from the launch log, the VALU and im2col paths, both encodings, graph replay, the GPU garbler
byte-identical to the host garbler (and its plan key), ASPP_SEG_CIFAR end to end and the range guard's torch path on
the device (docs/DILATED_CONV.md). The shape table is tests/dilated_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit, RangeGuard
from dash_amd.ir.bases import first_primes
from tests.dilated_cases import B3, SHAPES, conv_layer, conv_rescale_relu, form_of, plan_of, undilated, weights
from tests.test_dilated_conv import M7, aspp_seg, guard_case
from tests.test_gpu_parity import _check, _gpu_vs_host, _same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASES = {"k7": first_primes(7), "b3": B3}


def _inputs(rng, c, n, lim):
    return [rng.integers(-lim, lim + 1, c.input_size) for _ in range(n)]


def _logged(native, fn):
    native.hip_launch_log_take()
    native.hip_launch_log(True)
    try:
        out = fn()
    finally:
        native.hip_launch_log(False)
    return out, [l.split()[0] for l in native.hip_launch_log_take()]


@pytest.mark.parametrize("base", sorted(BASES))
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_dilated_layer(native, name, base):
    """One layer, 2 GCs at k = 7 / 3 GCs at [5, 7, 131]: HIP labels == host labels bit for bit, decoded ==
    plain_q_eval, and the launch log names exactly the form the planner binding predicts."""
    rng = np.random.default_rng(sum(map(ord, name)))
    crt = BASES[base]
    c = d.Circuit([conv_layer(rng, SHAPES[name])])
    xs = _inputs(rng, c, 2 if base == "k7" else 3, 20 if base == "k7" else 1)
    _, log = _logged(native, lambda: _check(c, crt, None, xs, hardened=True, plain=base == "k7"))
    want = form_of(SHAPES[name], plan_of(native, SHAPES[name], crt))
    assert [f for f in log if f.startswith("conv")] == [want], log
    if name != "k1_d2":
        assert "d<" in want, want  # a dilated form


@pytest.mark.parametrize("name", ["c64_k3", "d2_valid_rgb", "dw_d2"])
def test_undilated_rows_keep_their_form_names(native, name):
    """The row with its dilation set to 1 logs the form name it had before dilation existed (mfma=False: conv.valu)."""
    rng = np.random.default_rng(2)
    shape = undilated(SHAPES[name])
    c = d.Circuit([conv_layer(rng, shape)])
    _, log = _logged(native, lambda: _check(c, 7, None, _inputs(rng, c, 2, 20), hardened=True))
    want = {"c64_k3": "conv.img2<9,0>", "d2_valid_rgb": "conv.img2<1,1>", "dw_d2": "conv.grp<3,3,1>"}[name]
    assert [f for f in log if f.startswith("conv")] == [want], log
    assert form_of(shape, plan_of(native, shape, first_primes(7))) == want
    if shape[12] == 1:
        _, log = _logged(native, lambda: _check(c, 7, None, _inputs(rng, c, 2, 20), mfma=False, hardened=True))
        assert [f for f in log if f.startswith("conv")] == ["conv.valu"], log


@pytest.mark.parametrize("name", ["d2_same", "unequal"])
def test_dilated_valu(native, name):
    """The evaluator's mfma=False switch: k_conv_valu's dilated gather."""
    rng = np.random.default_rng(3)
    c = d.Circuit([conv_layer(rng, SHAPES[name])])
    _, log = _logged(native, lambda: _check(c, 7, None, _inputs(rng, c, 2, 20), mfma=False, hardened=True))
    assert [f for f in log if f.startswith("conv")] == ["conv.valud"], log
    assert form_of(SHAPES[name], plan_of(native, SHAPES[name], first_primes(7), mfma=False), mfma=False) == "conv.valud"


def test_dilated_im2col_in_a_child_process():
    """DASH_CONV_IMG=0 is read once per process: a fresh child runs c70_f20 through k_conv_mfma's dilated gather."""
    code = (
        "import numpy as np, dash_amd as d\n"
        "from dash_amd.native import native\n"
        "from tests.dilated_cases import SHAPES, conv_layer\n"
        "from tests.test_gpu_parity import _check\n"
        "n = native()\n"
        "rng = np.random.default_rng(5)\n"
        "c = d.Circuit([conv_layer(rng, SHAPES['c70_f20'])])\n"
        "xs = [rng.integers(-20, 21, c.input_size) for _ in range(2)]\n"
        "n.hip_launch_log(True)\n"
        "_check(c, 7, None, xs, hardened=True)\n"
        "print('forms', sorted({l.split()[0] for l in n.hip_launch_log_take() if l.startswith('conv')}))\n")
    env = dict(os.environ, DASH_CONV_IMG="0")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "forms ['conv.im2cold']" in r.stdout, r.stdout


@pytest.mark.parametrize("hardened", [True, False], ids=["hardened", "reference"])
def test_both_encodings(hardened):
    """d2_same under both encodings: in the reference encoding a tap in the padding adds w * Z_p."""
    rng = np.random.default_rng(4)
    c = d.Circuit([conv_layer(rng, SHAPES["d2_same"])])
    _check(c, 7, None, _inputs(rng, c, 2, 20), hardened=hardened)
    _check(c, B3, None, _inputs(rng, c, 3, 1), hardened=hardened, plain=False)


def test_graph_replay():
    """One evaluator, an eager first round and two graph-replayed rounds of Conv2d(d2_s2) -> Rescale -> Relu."""
    from dash_amd.runtime import HipEvaluator

    rng = np.random.default_rng(6)
    c = conv_rescale_relu(rng, SHAPES["d2_s2"])
    gcs = [GarbledCircuit(c, 7, 100.0, seed=bytes([i + 1]) * 16, rescale="mrs", relu="joint", hardened=True)
           for i in range(2)]
    ev = HipEvaluator([g.model for g in gcs])
    for _ in range(3):
        xs = _inputs(rng, c, 2, 20)
        enc = [g.garble_inputs(x) for g, x in zip(gcs, xs)]
        cpu = [g.cpu_evaluate(e) for g, e in zip(gcs, enc)]
        gpu = ev.evaluate(enc)
        for cl, gl in zip(cpu, gpu):
            for (pc, ac), (pg, ag) in zip(cl, gl):
                assert pc == pg
                np.testing.assert_array_equal(ac, ag)
        for g, x, o in zip(gcs, xs, gpu):
            np.testing.assert_array_equal(g.decode_outputs(o), g.plain_q_eval(x))


@pytest.mark.parametrize("name", ["d2_same", "c70_f20", "dw_d2"])
def test_gpu_garbler_bit_identical(name):
    """Conv2d -> Rescale -> Relu with the flagship constructions: the GPU garbler's offline message and decoder are
    byte-identical to the host garbler's; then an evaluation of the GPU-garbled model."""
    from dash_amd.runtime import HipEvaluator

    rng = np.random.default_rng(7)
    c = conv_rescale_relu(rng, SHAPES[name])
    g = _gpu_vs_host(c, 7, 100.0, rescale="mrs", relu="joint", hardened=True)
    x = rng.integers(-20, 21, c.input_size)
    ev = HipEvaluator(template=g.model, batch=1, device=0)
    ev.load(0, g.model)
    ev.encode_compressed_into(0, g, x)
    ev.upload_inputs_compressed()
    ev.run()
    ev.fetch_outputs()
    np.testing.assert_array_equal(ev.decode(0, g), g.plain_q_eval(x))


@pytest.mark.parametrize("name", ["c64_k3", "dw_d2"])
def test_gpu_garbler_plan_key_tells_dilated_from_plain(name):
    """A dilated layer and the undilated layer with the same weight bytes, garbled alternately in one process: each
    stays byte-identical to its host garbling (the garbler's plan cache is keyed by dh and dw)."""
    rng = np.random.default_rng(8)
    shape = SHAPES[name]
    w, b = weights(rng, shape)
    dil, plain = conv_layer(rng, shape, w, b), conv_layer(rng, undilated(shape), w, b)
    for _ in range(2):
        _gpu_vs_host(d.Circuit([dil]), 7, None, hardened=True)
        _gpu_vs_host(d.Circuit([plain]), 7, None, hardened=True)


def test_gpu_garbler_into_evaluator_slot():
    """The GPU garbler writes the tables of Conv2d(d2_same) -> Rescale -> Relu straight into an evaluator slot
    (HipEvaluator.sink); evaluate and decode both slots."""
    from dash_amd.runtime import HipEvaluator

    rng = np.random.default_rng(10)
    c = conv_rescale_relu(rng, SHAPES["d2_same"])
    kw = dict(rescale="mrs", relu="joint", hardened=True)
    first = GarbledCircuit(c, 7, 100.0, seed=bytes([7]) * 16, device=0, **kw)
    ev = HipEvaluator(template=first.model, batch=2, device=0)
    ev.load(0, first.model)
    seed = bytes(range(16))
    into = GarbledCircuit(c, 7, 100.0, seed=seed, device=0, sink=ev.sink(1), **kw)
    host = GarbledCircuit(c, 7, 100.0, seed=seed, **kw)
    assert _same(into.model.serialize(), host.model.serialize())
    ev.load(1, into.model)
    xs = _inputs(rng, c, 2, 20)
    for b, gc in enumerate((first, into)):
        ev.encode_compressed_into(b, gc, xs[b])
    ev.upload_inputs_compressed()
    ev.run()
    ev.fetch_outputs()
    for b, gc in enumerate((first, into)):
        np.testing.assert_array_equal(ev.decode(b, gc), gc.plain_q_eval(xs[b]))


def test_zoo_aspp_seg_cifar():
    """ASPP_SEG_CIFAR/DASH GPU-garbled with the flagship constructions, evaluated at batch 1: the decoded class map."""
    from dash_amd.runtime import HipEvaluator

    cfg, c, xs = aspp_seg()
    gc = GarbledCircuit(c, cfg["crt"], cfg["mrs"], seed=bytes(range(16)), device=0, rescale="mrs")
    assert gc.hardened and gc.relu == "joint"
    ev = HipEvaluator(template=gc.model, batch=1, device=0)
    ev.load(0, gc.model)
    x = xs[0]
    ev.encode_into(0, gc, x)
    ev.upload_inputs()
    ev.run()
    y = gc.decode_outputs(ev.get_outputs()[0])
    np.testing.assert_array_equal(y, gc.plain_q_eval(x))
    assert y.shape == (32 * 32,) and set(np.unique(y)) <= {0, 1, 2, 3}


def test_range_guard_torch_path_on_device():
    c, xs = guard_case()
    g = RangeGuard(c, M7, mrs=True, device=0)
    assert not g._native_ok()  # guard.hip has no dilated conv: the batched torch path on the device
    assert g.submit(xs).bad_indices() == [i for i, x in enumerate(xs) if g.violations_np(x)] == [1, 2]
