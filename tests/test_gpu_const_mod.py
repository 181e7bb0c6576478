"""The constant-modulus kernel forms (csrc/hip/dev.h ModK): the joint output kernels' per-residue walks
(k_rescale_relu_out_t, k_rescale_leaky_out_t, k_rescale_clip_out_t) and the staged chain of a first-primes base of
seven residues (k_mrs_chain_s<7, MODE, true>, modes 0 and 2), against the native host evaluator and the plaintext
model, in each mode of the switch in the same process: hip_set_const_mod(2) every constant form, 1 the output
kernels' only (the default), 0 none (the DASH_CONST_MOD values).

Circuits (host garbler, 3 GCs, a different permutation of the inputs per GC, as tests/test_gpu_chain_lds.py):
R = Rescale (chain mode 0, the plain rescale), J = Rescale + Relu joint (mode 2 + relu_out.tput), L = Rescale +
LeakyRelu joint (leaky_out.tput), C = Rescale + Clip joint (modes 2 and 1 + clip_out.tput). The joint-fuse knob
is forced on so that 3 GCs take the throughput output kernels, and the launches are planned for one CU, which makes
these small shapes staged (as the headline's are).

Shapes: N = 512 is one full 512-lane chain tile and two 256-lane output tiles; 528 ends in a tile of 16 live
lanes, whose spare lanes read zero rows and store nothing; 1040 = 2 * 512 + 16 is a partial tile behind full ones
(three chain blocks, five output tiles). Planned for one CU the chain's grid is capped at four blocks, so these
three sizes never send a block round its tile loop: test_chain_tile_loop adds 2576 = 5 * 512 + 16, six tiles on
four blocks, for the first-primes chain.

Bases: the first 7 primes (constant chain and constant output walks for 3 .. 17); {2, 3, 5, 7, 11, 13, 19}, seven
residues that are not the first primes (the generic chain; the output kernel's residue 19 falls back to the
run-time form beside constant ones); the first 6 primes (no first-primes chain is compiled for K = 6: the flag's
absence).

Edge conditions these cases already hold: every odd residue's label width n leaves a shorter last chunk, n % c != 0
(3: 80 / 19, 5: 55 / 13, 7: 45 / 11, 11: 37 / 8, 13: 34 / 8, 17: 31 / 7, 19: 30 / 7), so both the full-chunk and
the tail-chunk code run everywhere; and residue 3's 80 components do not fit one 64-row staging pass of the chain
(57 rows = 3 chunks, then 23 = 1 chunk + the tail of 4), so the pass loop carries its chunk state across a pass.

Each case asserts the launches from the launch log (staged chain, throughput output kernel; its lines are the
same in every mode), which of them took a constant form from hip_const_mod_launches (the host-side count of
constant-form launches: a silent fallback to the run-time forms would fail here), labels bit-identical to
GarbledCircuit.cpu_evaluate in all three modes, and decoded integers equal to plain_q_eval.

test_digit_helpers runs ModK's helpers alone (k_modk_test) against Python integers.
"""
import os
import sys

import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_clip_joint as cj  # noqa: E402
import test_gpu_joint_fused as jf  # noqa: E402
from leaky_cases import rescale_leaky  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [512, 528, 1040]
BASES = {"first7": 7, "other7": [2, 3, 5, 7, 11, 13, 19], "first6": 6}
EDGE_AT = [0, 15, 16, 63, 64, 255, 256, 511, 512, 527, 528, 1023, 1024, 2559, 2560, -17, -16, -1]
L_BITS = 5
Q_HI = 6
B = 3


def _build(kind, base, N):
    crt = BASES[base]
    l, S = L_BITS, 1 << L_BITS
    kw = dict(rescale="mrs")
    if kind == "R":
        circ = d.Circuit([d.Rescale(l, (N,))])
    elif kind == "J":
        circ, kw = d.Circuit([d.Rescale(l, (N,)), d.Relu((N,))]), dict(rescale="mrs", relu="joint")
    elif kind == "L":
        circ, kw = rescale_leaky(7, N, l, True), dict(rescale="mrs", relu="joint")
    else:
        circ, kw = cj.pair_circuit(N, l, Q_HI), dict(rescale="mrs", clip="joint")
    gcs = [GarbledCircuit(circ, crt, 100.0, seed=bytes([len(kind) + 40, i + 3]) * 8, **kw) for i in range(B)]
    M = gcs[0].crt_modulus
    h = M // 2
    lo, hi = -h, h - S  # the rescale's non-wrapping domain
    if kind == "C":
        _, _, lo, hi = cj.pair_domain(M, l, Q_HI)
    x = np.random.default_rng(31 * N + len(gcs[0].crt_base)).integers(lo, hi, N).astype(np.int64)
    edges = [v for v in [lo, hi - 1, 0, -1, 1, -S, S, -S - 1, S + 1, -S + 1, Q_HI * S, (Q_HI - 1) * S + 1] if lo <= v < hi]
    for n, i in enumerate(EDGE_AT):
        if -N <= i < N:
            x[i] = edges[n % len(edges)]
    xs = [x, x[::-1].copy(), np.roll(x, 7)]
    enc = [g.garble_inputs(v) for g, v in zip(gcs, xs)]
    return dict(gcs=gcs, enc=enc, cpu=[g.cpu_evaluate(e) for g, e in zip(gcs, enc)],
                plain=[g.plain_q_eval(v) for g, v in zip(gcs, xs)], crt=gcs[0].crt_base)


def _evaluate(native, c, mode):
    """One eager run in const-mod `mode`: (log, labels, constant-form launches of (the chain, an output kernel))."""
    base = native.hip_const_mod()
    native.hip_set_const_mod(mode)
    try:
        before = native.hip_const_mod_launches()
        log, out = jf._evaluate(native, c["gcs"], c["enc"], 1, 1)  # planned for one CU, the fusion forced on
        after = native.hip_const_mod_launches()
    finally:
        native.hip_set_const_mod(base)
    return log, out, (after[0] - before[0], after[1] - before[1])


def _want_counts(kind, base, mode):
    # one staged chain in mode 0 or 2 per circuit (a Clip's second chain is mode 1: generic), one output kernel
    return (1 if mode >= 2 and base == "first7" else 0, 1 if mode >= 1 and kind != "R" else 0)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("base", list(BASES))
@pytest.mark.parametrize("kind", ["R", "J", "L", "C"])
def test_const_mod_forms(native, kind, base, N):
    c = _build(kind, base, N)
    k = len(c["crt"])
    assert native.hip_chain_const_mod_pick(c["crt"]) == (base == "first7")
    log, on, n_on = _evaluate(native, c, 2)
    print("\n".join(log))
    log_out, out_only, n_out = _evaluate(native, c, 1)
    log_off, off, n_off = _evaluate(native, c, 0)
    assert log == log_off == log_out  # the same launches: the switch picks among forms of one launch
    assert [n_on, n_out, n_off] == [_want_counts(kind, base, m) for m in (2, 1, 0)]
    tiles = -(-N // 512)
    chains = [ln for ln in log if ln.startswith("chain.")]
    modes = {"R": [0], "J": [2], "L": [2], "C": [2, 1]}[kind]
    assert chains == ["chain.staged K=%d mode=%d grid=(%d,1,3) block=512" % (k, m, min(tiles, 4)) for m in modes], log
    if kind != "R":
        out = {"J": "relu_out.tput", "L": "leaky_out.tput", "C": "clip_out.tput"}[kind]
        assert log[-1] == "%s grid=(%d,%d,3) block=256" % (out, -(-N // 256), k), log
    jf._same_labels(c["cpu"], on)
    jf._same_labels(off, on)
    jf._same_labels(out_only, on)
    for g, o, ref in zip(c["gcs"], on, c["plain"]):
        np.testing.assert_array_equal(g.decode_outputs(o), ref)


@pytest.mark.parametrize("kind", ["R", "J"])
def test_chain_tile_loop(native, kind):
    """Six tiles on four blocks: blocks 0 and 1 walk two tiles, so the constant chain restarts its chunk state, its
    pair slots and its accumulators tile after tile."""
    N = 2576
    c = _build(kind, "first7", N)
    log, on, n_on = _evaluate(native, c, 2)
    assert [ln for ln in log if ln.startswith("chain.")] == [
        "chain.staged K=7 mode=%d grid=(4,1,3) block=512" % (0 if kind == "R" else 2)], log
    assert n_on == _want_counts(kind, "first7", 2)
    _, off, n_off = _evaluate(native, c, 0)
    assert n_off == (0, 0)
    jf._same_labels(c["cpu"], on)
    jf._same_labels(off, on)
    for g, o, ref in zip(c["gcs"], on, c["plain"]):
        np.testing.assert_array_equal(g.decode_outputs(o), ref)


PRIMES = [3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37]  # the odd primes of the shipped first-primes bases (K <= 12)


@pytest.mark.parametrize("q", PRIMES)
def test_digit_helpers(native, q):
    """Every helper of ModK<q> on chunk remainders r in [0, D): 0, 1, Q - 1, Q, Q^2 - 1, Q^2, D - Q, D - 1 and 2^16
    seeded random values, against Python integers: digit2 / digit, the chunk compress, the 24-bit reduction at each
    range the kernels use it at (the digit sums' Q^2 + 3 Q, the chain's lazy fold (I + 1) Q for I = 1 .. 6, the leaky
    digit's (Q - 1)(3 Q - 2) + 1, the leaky multiplier's Q^2; operands r mod the range, so every value of the small
    ranges occurs), and divmod on a numerator of 128 bits and on one below 2^64 (its two-step branch)."""
    _, n, c, D, _, _, _ = (int(v) for v in native.hip_modk_constants(q))
    fixed = [0, 1, q - 1, q, q * q - 1, q * q, D - q, D - 1]
    r = np.concatenate([np.array(fixed, dtype=np.uint32),
                        np.random.default_rng(1000 + q).integers(0, D, 1 << 16, dtype=np.uint32)])
    out = native.hip_modk_digits(q, r)
    assert out.shape == (r.size, 64) and not out[:, 63].any()
    ri = r.astype(np.int64)
    want = np.stack([(ri // q ** t) % q for t in range(c)], axis=1)
    np.testing.assert_array_equal(out[:, :c], want)            # two digits per extraction
    np.testing.assert_array_equal(out[:, 20:20 + c], want)     # one digit per extraction
    np.testing.assert_array_equal(out[:, 40], r)               # the digits recompressed
    X = q * q + 3 * q
    np.testing.assert_array_equal(out[:, 41], (ri % X) % q)    # the 24-bit reduction
    for I in range(1, 7):
        np.testing.assert_array_equal(out[:, 48 + I - 1], (ri % ((I + 1) * q)) % q)
    np.testing.assert_array_equal(out[:, 54], (ri % ((q - 1) * (3 * q - 2) + 1)) % q)
    np.testing.assert_array_equal(out[:, 55], (ri % (q * q)) % q)
    S = ri * ((1 << 32) + 1)  # < 2^63
    np.testing.assert_array_equal(out[:, 56], S % D)
    np.testing.assert_array_equal(out[:, 57].astype(np.int64) | (out[:, 58].astype(np.int64) << 32), S // D)
    mult = (1 << 96) + (1 << 45) + 1
    for i in list(range(len(fixed))) + list(range(len(fixed), r.size, 257)):
        P = (int(r[i]) * mult) % (1 << 128)
        quo, rem = divmod(P, D)
        assert int(out[i, 42]) == rem
        assert sum(int(out[i, 43 + w]) << (32 * w) for w in range(4)) == quo
