"""Every conv and dense GEMM kernel form at the smallest shapes that reach it (tests/gemm_cases.py; the table itself
is asserted on the CPU in test_conv_plan.py).

Each case garbles B GCs of a one-layer circuit on the host (one seed per GC, the second GC's input a permutation
of the first, the third a rotation) and runs a fresh HipEvaluator, whose first run is eager and logged. It asserts
  * form: the launch log is exactly the kernel, grid and block that the plan gives (restated here in Python);
  * host oracle: the labels are bit-identical to GarbledCircuit.cpu_evaluate for genuinely garbled inputs;
  * plain reference: the decoded integers equal plain_q_eval and a direct NumPy int64 convolution / product written
    here (reduced into the decoder's range: the crafted filters below are as large as the CRT modulus);
  * worst-case labels: crafted label arrays (every component p - 1, half, half + 1, 0, and uniform random), which
    need not decode, give the same labels on the host and on the GPU, bit for bit.

The kernels act on label components, uniform mod p whatever the plaintext is, so the accumulator bounds that
off, sh24 / m24 and modq_conv are derived from can only be approached by crafted labels against crafted weights:
filter (output row) 0 is +half in every residue's centered form, filter 1 is -half, filter 2 alternates, filter 3 is
all zero (the zero-count term zc * Z at its maximum); the other filters are small and random. The reference
encoding (hardened=False) is the one with a non-zero Z and bias labels.
"""
import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit
from tests.gemm_cases import CASE, CONV_CASES, ceil_div, plan_of

pytestmark = pytest.mark.gpu


def _line(form, grid, block=256):
    return "%s grid=(%d,%d,%d) block=%d" % (form, grid[0], grid[1], grid[2], block)


# ------------------------------------------------------------------------------------------------ crafted data
def _crt_solve(residues, mods):
    """The integer in [0, M) with the given residues (pairwise coprime moduli)."""
    M = int(np.prod(mods))
    return sum(r * (M // p) * pow(M // p, -1, p) for r, p in zip(residues, mods)) % M


def _crafted_rows(K, O, mods, rng):
    """[O][K] integer weights: rows 0 .. 3 crafted (module docstring), the rest in [-2, 2]."""
    plus = _crt_solve([p // 2 for p in mods], mods)
    minus = _crt_solve([(p - p // 2) % p for p in mods], mods)
    w = rng.integers(-2, 3, (O, K)).astype(np.int64)
    w[0], w[1], w[3] = plus, minus, 0
    w[2] = np.where(np.arange(K) % 2 == 0, plus, minus)
    return w


def _crafted_labels(enc, rng):
    """Label sets of the encoded input's own shape and dtype, one per pattern."""
    def const(f):
        return [(p, np.full_like(a, f(p) % p)) for p, a in enc]

    rand = [[(p, rng.integers(0, p, a.shape).astype(a.dtype)) for p, a in enc] for _ in range(2)]
    return [const(lambda p: p - 1), const(lambda p: p // 2), const(lambda p: p // 2 + 1), const(lambda p: 0)] + rand


def _wrap(v, M):
    """Into the decoder's range (evaluator.cpp crt_combine): [0, M / 2) as is, the rest negative."""
    v = np.asarray(v, dtype=np.int64) % M
    return np.where(v >= M // 2, v - M, v)


def _conv_numpy(c, w, b, x):
    xp = np.pad(x.reshape(c["C"], c["H"], c["W"]), ((0, 0), (c["ph"], c["ph"]), (c["pw"], c["pw"])))
    win = np.lib.stride_tricks.sliding_window_view(xp, (c["kh"], c["kw"]), axis=(1, 2))[:, ::c["sh"], ::c["sw"]]
    return (np.einsum("fcij,cyxij->fyx", w, win) + b[:, None, None]).reshape(-1)


def _dense_numpy(w, b, x, channel_tf):
    K = x.size
    if channel_tf:  # input i of the layer is element (i mod ch) of channel-last position i // ch
        x = x.reshape(channel_tf, K // channel_tf).T.reshape(-1)
    return w @ x + b


# ------------------------------------------------------------------------------------------------------ circuits
_BUILT = {}


def _garble(key, circuit, crt, xs, closed, hardened):
    """Garbled once per case and module: GCs, genuine and crafted inputs, the host oracle's labels for both."""
    if key in _BUILT:
        return _BUILT[key]
    rng = np.random.default_rng(len(_BUILT) + 77)
    gcs = [GarbledCircuit(circuit, crt, None, seed=bytes([i + 1, len(crt)]) * 8, hardened=hardened)
           for i in range(len(xs))]
    assert all(g.hardened == (hardened is not False) for g in gcs)
    enc = [g.garble_inputs(x) for g, x in zip(gcs, xs)]
    M = gcs[0].crt_modulus
    for g, x, ref in zip(gcs, xs, closed):
        np.testing.assert_array_equal(g.plain_q_eval(x), ref)  # the project's IR == the NumPy form written here
    crafted = _crafted_labels(enc[0], rng)
    # round r gives GC i pattern r + i: every pattern meets every GC's tables
    rounds = [[crafted[(r + i) % len(crafted)] for i in range(len(gcs))] for r in range(len(crafted))]
    built = dict(gcs=gcs, enc=enc, cpu=[g.cpu_evaluate(e) for g, e in zip(gcs, enc)], closed=[_wrap(v, M) for v in closed],
                 rounds=rounds, cpu_rounds=[[g.cpu_evaluate(l) for g, l in zip(gcs, rnd)] for rnd in rounds])
    _BUILT[key] = built
    return built


def _same_labels(want, got):
    assert len(want) == len(got)
    for w, g in zip(want, got):
        assert len(w) == len(g)
        for (pw, aw), (pg, ag) in zip(w, g):
            assert pw == pg
            np.testing.assert_array_equal(aw, ag)


def _run(native, built, B, expected_log, mfma=True):
    from dash_amd.runtime import HipEvaluator

    gcs = built["gcs"][:B]
    native.hip_launch_log_take()
    ev = HipEvaluator([g.model for g in gcs], mfma=mfma)
    native.hip_launch_log(True)
    try:
        gpu = ev.evaluate(built["enc"][:B])  # the first run of an evaluator is eager
    finally:
        native.hip_launch_log(False)
    log = native.hip_launch_log_take()
    print("\n".join(log))
    assert log == expected_log
    _same_labels(built["cpu"][:B], gpu)
    for g, o, ref in zip(gcs, gpu, built["closed"]):
        np.testing.assert_array_equal(g.decode_outputs(o), ref)
    for rnd, want in zip(built["rounds"], built["cpu_rounds"]):
        _same_labels(want[:B], ev.evaluate(rnd[:B]))


# ---------------------------------------------------------------------------------------------------------- conv
def _conv_built(name, hardened=None):
    c = CASE[name]
    rng = np.random.default_rng(sum(name.encode()))
    K = c["C"] * c["kh"] * c["kw"]
    w = _crafted_rows(K, c["F"], c["crt"], rng).reshape(c["F"], c["C"], c["kh"], c["kw"])
    b = rng.integers(-2, 3, c["F"]).astype(np.int64)
    layer = d.Conv2d.from_quantized(w, b, c["W"], c["H"], c["C"], c["F"], c["kw"], c["kh"], c["sw"], c["sh"],
                                    pad_width=c["pw"], pad_height=c["ph"])
    x = rng.integers(-2, 3, c["C"] * c["H"] * c["W"]).astype(np.int64)
    xs = [x, x[::-1].copy()]
    return _garble(("conv", name, hardened), d.Circuit([layer]), c["crt"], xs, [_conv_numpy(c, w, b, v) for v in xs],
                   hardened)


def _conv_log(native, c, B, mfma=True):
    plan = plan_of(native, c, mfma)
    ns = [native.nr_comps(p) for p in c["crt"]]
    fy = ceil_div(c["F"], 64)
    if not mfma:
        return [_line("conv.valu", (ceil_div(plan["OH"] * plan["OW"], 256), c["F"], B * sum(ns)))]
    if plan["nbands"] == 0:
        return [_line("conv.im2col", (ceil_div(B * n * plan["OH"] * plan["OW"], 64), fy, 1)) for n in ns]
    return [_line(c["form"], (B * sum(ns) * plan["nbands"], fy, 1))]


@pytest.mark.parametrize("name", [c["name"] for c in CONV_CASES])
def test_conv_form(native, name):
    _run(native, _conv_built(name), 2, _conv_log(native, CASE[name], 2))


@pytest.mark.parametrize("name", ["k9_c58_w13", "k0_c128", "ur1_w7"])
def test_conv_reference_encoding(native, name):
    """hardened=False: the bias comes from the uploaded label rows and Z is a real label, so the padding positions
    and the zc * Z term are live (both are zero in the hardened encoding). k0_c128 is the 32-bit reduction at
    Kpad = 1152 with p = 251; k9_c58_w13 has p = 131 on the 24-bit reduction within a factor 2 of its limit."""
    _run(native, _conv_built(name, hardened=False), 2, _conv_log(native, CASE[name], 2))


@pytest.mark.parametrize("hardened", [None, False], ids=["hardened", "reference"])
def test_conv_valu(native, hardened):
    c = CASE["k9_c58_w13"]
    _run(native, _conv_built(c["name"], hardened), 2, _conv_log(native, c, 2, mfma=False), mfma=False)


# --------------------------------------------------------------------------------------------------------- dense
D7, D2 = [7, 127, 131], [2, 3, 5, 7]  # D2: 128 .. 45 components per residue, so some residues' blocks return early


def _dense_built(K, O, crt, channel_tf=0, first=0, hardened=None):
    """One dense layer K -> O; first > 0: a dense first -> K in front of it (the layer's input then sits in the
    evaluator's second activation buffer, not in the input buffer)."""
    rng = np.random.default_rng(1000 * K + O + channel_tf)
    w = _crafted_rows(K, O, crt, rng)
    b = rng.integers(-2, 3, O).astype(np.int64)
    layers, w0 = [d.Dense.from_quantized(w, b, channel_tf=channel_tf)], None
    if first:
        w0, b0 = rng.integers(-1, 2, (K, first)).astype(np.int64), rng.integers(-2, 3, K).astype(np.int64)
        layers.insert(0, d.Dense.from_quantized(w0, b0))
    x = rng.integers(-2, 3, first or K).astype(np.int64)
    xs = [x, x[::-1].copy(), np.roll(x, 5)]

    def ref(v):
        if first:
            v = _dense_numpy(w0, b0, v, 0)
        return _dense_numpy(w, b, v, channel_tf)

    return _garble(("dense", K, O, tuple(crt), channel_tf, first, hardened), d.Circuit(layers), crt, xs,
                   [ref(v) for v in xs], hardened)


def _dense_log(native, K, O, crt, B, mfma=True):
    ns = [native.nr_comps(p) for p in crt]
    if mfma:
        return _line("dense.mfma", (ceil_div(B * max(ns), 64), ceil_div(O, 64), len(crt)))
    return _line("dense.valu", (ceil_div(O, 256), 1, B * sum(ns)))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("crt", [D7, D2], ids=["p131", "p2"])
@pytest.mark.parametrize("K,O", [(65, 70), (127, 17), (192, 64), (30, 5)])
def test_dense_form(native, K, O, crt, B):
    """O > 64 (a second output tile), K not a multiple of 64 (K = 65: the last k-step reads 63 bytes past every
    column, for the last column of the last GC into the buffer's slack), a centered residue (p = 131)."""
    _run(native, _dense_built(K, O, crt), B, [_dense_log(native, K, O, crt, B)])


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hardened", [None, False], ids=["hardened", "reference"])
def test_dense_overread_second_layer(native, hardened, B):
    """The K = 65 layer as the last of two: its input is the first layer's output buffer."""
    built = _dense_built(65, 70, D7, first=40, hardened=hardened)
    _run(native, built, B, [_dense_log(native, 40, 65, D7, B), _dense_log(native, 65, 70, D7, B)])


@pytest.mark.parametrize("mfma", [True, False], ids=["mfma", "valu"])
@pytest.mark.parametrize("channel_tf", [0, 3])
@pytest.mark.parametrize("crt", [D7, D2], ids=["p131", "p2"])
def test_dense_channel_tf(native, crt, channel_tf, mfma):
    """channel_tf (a dense after a channel-last flatten) through both kernels: a.src in k_dense, the folded column
    order of the int8 weights in k_dense_mfma; decoded against the permutation restated in _dense_numpy."""
    built = _dense_built(96, 33, crt, channel_tf=channel_tf, hardened=False)
    _run(native, built, 3, [_dense_log(native, 96, 33, crt, 3, mfma)], mfma=mfma)


# --------------------------------------------------------------------------------------------------- GPU garbler
@pytest.mark.parametrize("name", ["k9_c58_w13", "k0_fallback", "im2col_3x3"])
def test_gpu_garbler_conv_forms(native, name):
    """The GPU garbler plans with its own cache (garble_gpu.hip conv_plans) and calls the same launchers, one GC
    per launch: the same form as the evaluator's, and a model byte-identical to the host garbler's."""
    import hashlib

    c = CASE[name]
    built = _conv_built(name)
    host = built["gcs"][0]
    native.hip_launch_log_take()
    native.hip_launch_log(True)
    try:
        gpu = GarbledCircuit(host.circuit, c["crt"], None, seed=host.seed, device=0)
    finally:
        native.hip_launch_log(False)
    log = [ln for ln in native.hip_launch_log_take() if ln.startswith("conv.")]
    print("\n".join(log))
    assert log == _conv_log(native, c, 1)
    for a, b in ((gpu.model.serialize(), host.model.serialize()), (gpu.decoder.serialize(), host.decoder.serialize())):
        assert len(a) == len(b) and hashlib.sha256(a).digest() == hashlib.sha256(b).digest()
