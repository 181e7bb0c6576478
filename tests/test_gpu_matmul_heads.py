"""The multi-head MatMul layer on the GPU (docs/MATMUL.md, Heads): the HIP evaluator's two kernel forms with the head
index, bit-exact against the host evaluator over eager and graph-replayed rounds; the unchanged grids of a G = 1
layer; the GPU garbler byte-identical to the host garbler (also into an evaluator slot); RELU_ATTN_CIFAR end to end.
Circuits and inputs: tests/matmul_heads_cases.py."""
import numpy as np
import pytest

from dash_amd.garbling import GarbledCircuit
from tests.matmul_heads_cases import (M7, expected, gram_heads_circuit, gram_heads_expected, gram_heads_inputs,
                                      heads_circuit, heads_inputs)
from tests.test_gpu_matmul import _run
from tests.test_gpu_parity import _gpu_vs_host, _same

pytestmark = pytest.mark.gpu

K, GCS, BS, TILE = 7, 2, 256, 16  # residues, GCs of a _run, lanes per block, the blocked form's tile edge


def _grid(form, G, M, N):
    """The launch grid, from the rule in docs/MATMUL.md: the lane form runs over the flat G M N outputs in blocks of
    256 lanes, the blocked form over G times the head's 16 x 16 tiles; y = residues, z = GCs."""
    x = -(-G * M * N // BS) if form == "lane" else G * (-(-M // TILE)) * (-(-N // TILE))
    return f"matmul.{form} grid=({x},{K},{GCS}) block={BS}"


def _run_case(G, M, T, N, ta=False, tb=False, log=None, rounds=3):
    return _run(heads_circuit(G, M, T, N, ta, tb), heads_inputs(G, M, T, N, ta, tb, rounds=2 * rounds), log=log,
                want=lambda x: expected(G, M, T, N, x, ta, tb))


# (G, M, T, N), trans_a, trans_b, the form the rule picks: blocked where a head has M >= 16 and N >= 16 (the two GCs
# of a case are far too few blocks for the fill rule of half-full tiles, see test_half_full_tiles_follow_the_device_fill)
CASES = [((3, 5, 3, 7), False, False, "lane"), ((2, 13, 4, 20), False, True, "lane"), ((4, 8, 16, 16), False, True, "lane"),
         ((2, 16, 16, 16), True, True, "blocked"), ((3, 17, 5, 18), True, False, "blocked"),
         ((4, 16, 8, 16), True, False, "blocked")]


@pytest.mark.parametrize("shape,ta,tb,form", CASES, ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)[0])
def test_heads_shapes(native, shape, ta, tb, form):
    """Lane form: (3, 5, 3, 7) has 105 outputs, its two head boundaries (35, 70) inside waves;
    (2, 13, 4, 20) 520 outputs, the head boundary at 260 and the block edges at 256 and 512; (4, 8, 16, 16) is the
    zoo's mix. Blocked form: (2, 16, 16, 16) full tiles; (3, 17, 5, 18) 2 x 2 tiles per head with one live row and
    two live columns on the edges of every head, and a t chunk of 5; (4, 16, 8, 16) the zoo's scores. All four flag
    pairs appear. (2, 16, 17, 15), forced blocked, runs in test_heads_forms_off_their_rule."""
    log = _run_case(*shape, ta, tb, log=native)
    print("\n".join(log))
    G, M, T, N = shape
    assert [l for l in log if l.startswith("matmul.")] == [_grid(form, G, M, N)], log


@pytest.mark.parametrize("cus,form", [(0, "lane"), (16, "blocked"), (28, "blocked"), (29, "lane"), (5, "lane"),
                                      (6, "blocked")], ids=lambda v: str(v))
def test_half_full_tiles_follow_the_device_fill(native, cus, form):
    """The rule for G > 1 (docs/MATMUL.md, Heads): heads whose tiles are half full in M, here the zoo's mix
    (4, 8, 16, 16), take the blocked form while the lane grid, ceil(512 / 256) * 7 residues * 2 GCs = 28 blocks,
    has at least one block per CU and fewer than five: CUs in 6 .. 28. The planning CU count is set for the test
    (0 = the device's own, 256 on an MI355X: 28 blocks are below one per CU, the per-head rule stands)."""
    assert cus or native.hip_planning_cus() > 28
    native.hip_set_planning_cus(cus)
    try:
        log = _run_case(4, 8, 16, 16, False, True, log=native, rounds=1)
    finally:
        native.hip_set_planning_cus(0)
    assert [l for l in log if l.startswith("matmul.")] == [_grid(form, 4, 8, 16)], log


def test_the_fill_rule_is_for_half_full_tiles_of_heads_only(native):
    """Under a CU count that puts every small grid in the partly filled range, a single-head (8, 16, 16), heads
    thinner than half a tile (2, 7, 3, 16) and heads of N below a tile (2, 8, 3, 15) keep the lane form."""
    native.hip_set_planning_cus(3)
    try:
        logs = [_run_case(*shape, log=native, rounds=1) for shape in [(1, 8, 16, 16), (2, 7, 3, 16), (2, 8, 3, 15)]]
    finally:
        native.hip_set_planning_cus(0)
    for log in logs:
        assert [l.split()[0] for l in log if l.startswith("matmul.")] == ["matmul.lane"], log


@pytest.mark.parametrize("form", ["lane", "blocked"])
def test_heads_forms_off_their_rule(form):
    """DASH_MATMUL_FORM (read when an evaluator is planned) forces the lane form on tiled heads and the blocked form
    on heads thinner than a tile, in a freshly started child process each. Blocked: (2, 16, 17, 15) has N below a
    tile and T one above a chunk; (3, 5, 3, 7) and (2, 13, 4, 20) are a single mostly idle tile and 1 x 2 tiles per
    head. Lane: the blocked cases above."""
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = str(Path(__file__).resolve().parents[1])
    cases = [((3, 17, 5, 18), True, False), ((4, 16, 8, 16), True, False)] if form == "lane" else \
        [((2, 16, 17, 15), False, False), ((3, 5, 3, 7), False, True), ((2, 13, 4, 20), True, True)]
    code = FORCED_FORM_SCRIPT.format(root=root, cases=cases, form=form)
    env = dict(os.environ, DASH_MATMUL_FORM=form)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env, cwd=root)
    assert r.returncode == 0 and r.stdout.strip().endswith("same"), r.stdout + r.stderr


FORCED_FORM_SCRIPT = """
import sys
sys.path.insert(0, {root!r})
from dash_amd.native import native
from tests.test_gpu_matmul_heads import _grid, _run_case
for shape, ta, tb in {cases!r}:
    log = _run_case(*shape, ta, tb, log=native())
    G, M, T, N = shape
    assert [l for l in log if l.startswith("matmul.")] == [_grid({form!r}, G, M, N)], log
print("same")
"""


def test_heads_gram(native):
    """x_g x_g^T per head: src is the layer's own input (with trans_b), keyed once; ky aliases kx. (3, 4, 5, 4) by
    rule takes the lane form."""
    G, M, T = 3, 4, 5
    log = _run(gram_heads_circuit(G, M, T), gram_heads_inputs(G, M, T, rounds=6), log=native,
               want=lambda x: gram_heads_expected(G, M, T, x))
    assert [l for l in log if l.startswith("matmul.")] == [_grid("lane", G, M, M)], log


@pytest.mark.parametrize("shape,form,grid_x", [((13, 4, 20), "lane", 2), ((17, 3, 16), "blocked", 2),
                                               ((33, 18, 35), "blocked", 9)], ids=["lane", "blocked", "3x3"])
def test_single_head_launches_are_unchanged(native, shape, form, grid_x):
    """G = 1 launches what the single-head layer always did: the lane form over ceil(M N / 256) blocks (260 outputs:
    2), the blocked form over ceil(M / 16) ceil(N / 16) tiles (2 x 1 and 3 x 3), y = 7 residues, z = 2 GCs, 256
    lanes; one key pre-pass and one contraction per layer. The numbers are written out here from those formulas."""
    M, T, N = shape
    log = _run_case(1, M, T, N, log=native)
    assert [l for l in log if l.startswith("matmul.")] == [f"matmul.{form} grid=({grid_x},7,2) block=256"], log


@pytest.mark.parametrize("shape,ta,tb", [((3, 5, 3, 7), False, True), ((2, 16, 16, 16), True, False),
                                         ((2, 3, 37, 4), False, False)], ids=["lane", "blocked", "T37"])
def test_gpu_garbler_bit_identical_heads(shape, ta, tb, monkeypatch, capfd):
    """GpuGarbler::matmul_dev with the slab offsets in its operand maps, byte for byte against the host garbler (T =
    37: three term groups of the segmented sum); one trace line per layer. Then the device-garbled model evaluates
    to the per-head product."""
    from dash_amd.runtime import HipEvaluator

    monkeypatch.setenv("DASH_GG_TRACE", "1")
    c = heads_circuit(*shape, ta, tb)
    g = _gpu_vs_host(c, 7, 100.0)
    err = capfd.readouterr().err
    assert err.count("[gg] matmul") == 1 and "[gg] mul" not in err
    monkeypatch.delenv("DASH_GG_TRACE")
    x = heads_inputs(*shape, ta, tb)[0]
    ev = HipEvaluator(template=g.model, batch=1, device=0)
    ev.load(0, g.model)
    ev.encode_compressed_into(0, g, x)
    ev.upload_inputs_compressed()
    ev.run()
    ev.fetch_outputs()
    np.testing.assert_array_equal(ev.decode(0, g), expected(*shape, x, ta, tb))


def test_gpu_garbler_gram_heads_bit_identical():
    _gpu_vs_host(gram_heads_circuit(3, 4, 5), 7, 100.0)


def test_gpu_garbler_heads_into_evaluator_slot():
    """The GPU garbler writes a multi-head MatMul's tables straight into an evaluator slot (HipEvaluator.sink)."""
    from dash_amd.runtime import HipEvaluator

    shape = (3, 5, 3, 7)
    c = heads_circuit(*shape)
    first = GarbledCircuit(c, 7, 100.0, seed=bytes([7]) * 16, device=0)
    ev = HipEvaluator(template=first.model, batch=2, device=0)
    ev.load(0, first.model)
    seed = bytes(range(16))
    into = GarbledCircuit(c, 7, 100.0, seed=seed, device=0, sink=ev.sink(1))
    host = GarbledCircuit(c, 7, 100.0, seed=seed)
    assert _same(into.model.serialize(), host.model.serialize())
    ev.load(1, into.model)
    xs = heads_inputs(*shape)
    for b, gc in enumerate((first, into)):
        ev.encode_compressed_into(b, gc, xs[b])
    ev.upload_inputs_compressed()
    ev.run()
    ev.fetch_outputs()
    for b, gc in enumerate((first, into)):
        np.testing.assert_array_equal(ev.decode(b, gc), expected(*shape, xs[b]))


def test_relu_attn_cifar_end_to_end(native, monkeypatch, capfd):
    """RELU_ATTN_CIFAR at batch 1: GPU garbler (both contractions on the device, one trace line each) plus the HIP
    evaluator, exact against the plaintext quantized model; the scores take the blocked form and the mix the lane
    form, each over all four heads."""
    from dash_amd.ir.quant import QuantizationMethod as Q
    from dash_amd.models import zoo
    from dash_amd.runtime import HipEvaluator

    c = zoo.build_circuit("RELU_ATTN_CIFAR", Q.ScaleQuant, 5, seed=0)
    xs = zoo.quantized_inputs("RELU_ATTN_CIFAR", 2, Q.ScaleQuant, 5, seed=7)
    c.calibrate(xs, M7)
    assert c.required_crt_modulus() <= M7
    monkeypatch.setenv("DASH_GG_TRACE", "1")
    gc = GarbledCircuit(c, 7, 100.0, seed=bytes(range(16)), device=0)
    assert capfd.readouterr().err.count("[gg] matmul") == 2
    monkeypatch.delenv("DASH_GG_TRACE")
    ev = HipEvaluator(template=gc.model, batch=1, device=0)
    ev.load(0, gc.model)
    for r, x in enumerate(xs):
        ev.encode_compressed_into(0, gc, x)
        ev.upload_inputs_compressed()
        if r == 0:
            native.hip_launch_log_take()
            native.hip_launch_log(True)
        try:
            ev.run()
        finally:
            native.hip_launch_log(False)
        ev.fetch_outputs()
        np.testing.assert_array_equal(ev.decode(0, gc), c.plain_q_eval(x, False, M7))
        if r == 0:
            log = native.hip_launch_log_take()
            assert [l for l in log if l.startswith("matmul.")] == \
                ["matmul.blocked grid=(4,7,1) block=256", "matmul.lane grid=(2,7,1) block=256"], log
