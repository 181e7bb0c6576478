"""The ConvTranspose2d and Upsample layers on the GPU: the HIP evaluator (the sub-pixel view through launch_conv's
scatter epilogues) bit-exact against the host evaluator, the kernel forms from the launch log, graph replay, the GPU
garbler byte-identical to the host garbler, UNET_CIFAR end to end and the range guard's torch path on the device
(docs/CONV_TRANSPOSE.md).

Shapes are (W, H, C, F, kh, kw, sw, sh, pw, ph, opw, oph); each is the smallest that exercises one thing."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit, RangeGuard
from dash_amd.ir.bases import first_primes
from tests.test_conv_transpose import B3, M7, conv_up_conv, convt_layer, convt_rescale_relu, guard_case, unet
from tests.test_gpu_parity import _check, _gpu_vs_host, _same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = {
    "k2s2": (5, 4, 3, 5, 2, 2, 2, 2, 0, 0, 0, 0),             # one tap per output, odd width, unaligned rows
    "k4s2p1": (6, 5, 4, 4, 4, 4, 2, 2, 1, 1, 0, 0),           # crop on all four sides
    "k3s2p1op1": (7, 6, 5, 3, 3, 3, 2, 2, 1, 1, 1, 1),        # zero-filled view taps and output padding
    "k3s1p1": (9, 5, 4, 6, 3, 3, 1, 1, 1, 1, 0, 0),           # a single phase
    "unequal": (6, 7, 3, 4, 3, 2, 1, 2, 0, 1, 0, 0),          # non-square kernel, unequal strides
    "s3k5": (4, 4, 2, 2, 5, 5, 3, 3, 2, 2, 0, 0),             # stride 3: byte stores, 9 phases
    "s3_f10": (4, 4, 2, 10, 3, 3, 3, 3, 0, 0, 0, 0),          # 90 view filters: phases straddle the 64-filter block
    "c70_f20": (4, 3, 70, 20, 2, 2, 2, 2, 0, 0, 0, 0),        # two channel chunks; a partial second filter block
    "two_bands_c64": (32, 20, 64, 2, 2, 2, 2, 2, 0, 0, 0, 0),  # more than one row band
    "rgb_unrolled": (6, 5, 3, 4, 4, 4, 2, 2, 1, 1, 0, 0),     # the tap-unrolled view
    "aligned_w16": (16, 4, 64, 4, 2, 2, 2, 2, 0, 0, 0, 0),    # dword-aligned rows for the wide store
    # beyond the list: the two remaining scatter instantiations of k_conv_img2
    "k4_c64": (4, 3, 64, 2, 4, 4, 2, 2, 1, 1, 0, 0),          # 2x2 view taps of 64 channels: A in registers, 4 k-steps
    "ur0_c20": (5, 4, 20, 2, 4, 4, 2, 2, 1, 1, 0, 0),         # unrolled view of 80 patch bytes: two k-steps
}
BASES = {"k7": first_primes(7), "b3": B3}


def plan_of(native, shape, crt, mfma=True):
    W, H, C, F, kh, kw, sw, sh, pw, ph, opw, oph = shape
    return native.hip_convt_plan(C, H, W, F, kh, kw, sh, sw, ph, pw, oph, opw, crt, mfma)


def form_of(plan, mfma=True):
    """launch_conv's pick for a transposed layer, restated (kernels_gemm.hip)."""
    if not mfma:
        return "convt.valu"
    if plan["nbands"] == 0:
        return "convt.im2col"
    ks = plan["KS"]
    if plan["ur"]:
        return "convt.img2<1,1>" if ks == 1 else "convt.img2<0,1>"
    return "convt.img2<%d,0>" % (ks if ks in (4, 1) else 0)


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
def test_convt_layer(native, name, base):
    """One transposed layer, 2 GCs at k = 7 / 3 GCs at [5, 7, 131]: HIP labels == host labels bit for bit, decoded
    == plain_q_eval, and the launch log names the form the planner binding predicts."""
    rng = np.random.default_rng(sum(map(ord, name)))
    crt = BASES[base]
    c = d.Circuit([convt_layer(rng, SHAPES[name])])
    xs = _inputs(rng, c, 2 if base == "k7" else 3, 20 if base == "k7" else 1)
    _, log = _logged(native, lambda: _check(c, crt, None, xs, hardened=True, plain=base == "k7"))
    want = form_of(plan_of(native, SHAPES[name], crt))
    assert [f for f in log if f.startswith("conv")] == [want], log


def test_form_coverage(native):
    """Across the table: the scatter form with A in registers, the generic one, the unrolled view, more than one
    band, and both store paths (the wide one where sw = 2)."""
    plans = {n: plan_of(native, s, BASES["k7"]) for n, s in SHAPES.items()}
    forms = {n: form_of(p) for n, p in plans.items()}
    assert {"convt.img2<1,0>", "convt.img2<4,0>", "convt.img2<0,0>", "convt.img2<1,1>", "convt.img2<0,1>"} == \
        set(forms.values()), forms
    assert forms["k2s2"] == "convt.img2<1,0>" and forms["c70_f20"] == "convt.img2<0,0>"
    assert forms["rgb_unrolled"] == "convt.img2<1,1>" and plans["rgb_unrolled"]["ur"] == 1
    assert plans["two_bands_c64"]["nbands"] > 1
    for n, s in SHAPES.items():
        assert plans[n]["tsc"] == (2 if s[6] == 2 else 1), n  # sw = 2: the wide store
    assert {p["tsc"] for p in plans.values()} == {1, 2}
    # the wide store's dword path needs a dword-aligned row somewhere, its byte path an unaligned one
    assert plans["aligned_w16"]["OW"] % 4 == 0 and plans["k2s2"]["OW"] % 4 == 2
    assert plans["s3_f10"]["VF"] == 90 and plans["c70_f20"]["VF"] == 80 and plans["c70_f20"]["Cpad"] == 128


@pytest.mark.parametrize("name", ["k4s2p1", "s3_f10"])
def test_convt_valu(native, name):
    """The evaluator's mfma=False switch: k_conv_valu's scatter."""
    rng = np.random.default_rng(3)
    c = d.Circuit([convt_layer(rng, SHAPES[name])])
    _, log = _logged(native, lambda: _check(c, 7, None, _inputs(rng, c, 2, 20), mfma=False, hardened=True))
    assert [f for f in log if f.startswith("conv")] == ["convt.valu"], log


def test_convt_im2col_in_a_child_process():
    """DASH_CONV_IMG=0 is read once per process: a fresh child runs one shape through k_conv_mfma's scatter."""
    code = (
        "import numpy as np, dash_amd as d\n"
        "from dash_amd.native import native\n"
        "from tests.test_conv_transpose import convt_layer\n"
        "from tests.test_gpu_parity import _check\n"
        "from tests.test_gpu_conv_transpose import SHAPES\n"
        "n = native()\n"
        "rng = np.random.default_rng(5)\n"
        "c = d.Circuit([convt_layer(rng, SHAPES['c70_f20'])])\n"
        "xs = [rng.integers(-20, 21, c.input_size) for _ in range(2)]\n"
        "n.hip_launch_log(True)\n"
        "_check(c, 7, None, xs, hardened=True)\n"
        "print('forms', sorted({l.split()[0] for l in n.hip_launch_log_take() if l.startswith('conv')}))\n")
    env = dict(os.environ, DASH_CONV_IMG="0")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "forms ['convt.im2col']" in r.stdout, r.stdout


def test_convt_graph_replay():
    """One evaluator, an eager first round and graph-replayed later rounds, ConvTranspose2d -> Rescale -> Relu."""
    from dash_amd.runtime import HipEvaluator

    rng = np.random.default_rng(6)
    c = convt_rescale_relu(rng, SHAPES["k3s2p1op1"])
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


@pytest.mark.parametrize("name", ["k2s2", "k3s2p1op1", "c70_f20"])
def test_gpu_garbler_bit_identical_convt(name):
    """ConvTranspose2d -> Rescale -> Relu with the flagship constructions: the GPU garbler's offline message and
    decoder are byte-identical to the host garbler's; then an evaluation of the GPU-garbled model."""
    from dash_amd.runtime import HipEvaluator

    rng = np.random.default_rng(7)
    c = convt_rescale_relu(rng, SHAPES[name])
    g = _gpu_vs_host(c, 7, 100.0, rescale="mrs", relu="joint", hardened=True)
    x = rng.integers(-20, 21, c.input_size)
    ev = HipEvaluator(template=g.model, batch=1, device=0)
    ev.load(0, g.model)
    ev.encode_compressed_into(0, g, x)
    ev.upload_inputs_compressed()
    ev.run()
    ev.fetch_outputs()
    np.testing.assert_array_equal(ev.decode(0, g), g.plain_q_eval(x))


def test_gpu_garbler_plan_key_tells_convt_from_conv():
    """A transposed layer (k1 s1: its view is a 1x1 conv of the same geometry) and that plain conv, with the same
    weight bytes, garbled in one process: each is byte-identical to its host garbling."""
    rng = np.random.default_rng(8)
    w, b = rng.integers(-6, 7, (4, 4, 1, 1)), rng.integers(-9, 10, 4)
    ct = d.ConvTranspose2d.from_quantized(w, b, 5, 4, 4, 4, 1, 1)
    cv = d.Conv2d.from_quantized(w, b, 5, 4, 4, 4, 1, 1)
    for _ in range(2):
        _gpu_vs_host(d.Circuit([cv]), 7, None, hardened=True)
        _gpu_vs_host(d.Circuit([ct]), 7, None, hardened=True)


@pytest.mark.parametrize("hardened", [True, False], ids=["hardened", "reference"])
def test_gpu_garbler_bit_identical_upsample(hardened):
    rng = np.random.default_rng(9)
    c = conv_up_conv(rng)
    c = d.Circuit(list(c.layers) + [d.Relu(c.output_dims)])
    kw = dict(hardened=True, relu="mrs") if hardened else dict(hardened=False, rescale="legacy", relu="approx")
    _gpu_vs_host(c, 7, 100.0, **kw)


def test_gpu_garbler_into_evaluator_slot():
    """The GPU garbler writes the tables of ConvTranspose2d -> Rescale -> Relu -> Upsample straight into an
    evaluator slot (HipEvaluator.sink); evaluate and decode both slots."""
    from dash_amd.runtime import HipEvaluator

    rng = np.random.default_rng(10)
    c = convt_rescale_relu(rng, SHAPES["k4s2p1"])
    c = d.Circuit(list(c.layers) + [d.Upsample(c.output_dims, 2, 1)])
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


@pytest.mark.parametrize("hardened", [True, False], ids=["hardened", "reference"])
def test_upsample_labels(hardened):
    """Upsample (5, 3, 4) by (2, 3): HIP labels against the host under both encodings."""
    rng = np.random.default_rng(11)
    c = d.Circuit([d.Upsample((5, 3, 4), 2, 3)])
    _check(c, 7, None, _inputs(rng, c, 2, 1000), hardened=hardened)
    _check(c, B3, None, _inputs(rng, c, 3, 1000), hardened=hardened)


def test_zoo_unet_cifar():
    """UNET_CIFAR/DASH GPU-garbled with the flagship constructions, evaluated at batch 1: the decoded class map."""
    from dash_amd.runtime import HipEvaluator

    cfg, c, xs = unet()
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
    assert not g._native_ok()  # guard.hip has no ConvTranspose2d: the batched torch path on the device
    assert g.submit(xs).bad_indices() == [i for i, x in enumerate(xs) if g.violations_np(x)] == [1, 2]
