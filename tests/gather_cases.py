"""Shared circuits and inputs of the Gather tests (tests/test_gather.py on the host, tests/test_gpu_gather.py on the
GPU).

A plain case is one Gather layer on a flat tensor, named by its (Nin, Nout) and its map. The HIP evaluator's dword
form (k_gather4) gives a lane four consecutive outputs and a block 1024 of them, and is the planner's pick where
Nout % 4 == 0; the shapes are the smallest that reach each edge of that:

    perm1024   (1024, 1024)  a random permutation: exactly one block
    rev1020    (1020, 1020)  the reversal: the last block is one lane short
    rot1028    (1028, 1028)  a rotation by 5: one live lane in a second block
    rep1028    (7, 1028)     seven inputs read 1028 times (heavy repeats)
    few4       (2048, 4)     one live lane, most inputs unread
    odd1025    (1023, 1025)  Nout % 4 == 1: the byte form by the rule
    odd3       (5, 3)        the byte form below one lane's four outputs

A Gather moves labels and computes nothing, so any signed CRT value passes through: the inputs are drawn from the
whole range [-M7 / 2, M7 / 2) and carry both extremes and 0 on their first and last elements.

The composite cases put the layer where its surroundings matter: an in_src source read in place, the zoo's
shuffle unit on a (4, 4, 4) tensor, the index labels of an ArgMax, and repeats in front of a ReLU (one gate per
copy)."""
from __future__ import annotations

import numpy as np

import dash_amd as d
from dash_amd.ir.bases import crt_modulus, first_primes
from tests.matmul_cases import tiny_arch

M7 = crt_modulus(first_primes(7))

DWORD = ("perm1024", "rev1020", "rot1028", "rep1028", "few4")
BYTE = ("odd1025", "odd3")
SHAPES = {"perm1024": (1024, 1024), "rev1020": (1020, 1020), "rot1028": (1028, 1028), "rep1028": (7, 1028),
          "few4": (2048, 4), "odd1025": (1023, 1025), "odd3": (5, 3)}


def gather_index(name: str) -> np.ndarray:
    nin, nout = SHAPES[name]
    rng = np.random.default_rng(sum(SHAPES[name]))
    if name == "perm1024":
        return rng.permutation(nin)
    if name == "rev1020":
        return np.arange(nin)[::-1].copy()
    if name == "rot1028":
        return (np.arange(nout) + 5) % nin
    if name == "few4":
        return np.array([nin - 1, 0, 1023, 1024])  # the last and the first input, and both sides of element 1024
    idx = rng.integers(0, nin, nout)
    idx[0], idx[-1] = nin - 1, 0
    return idx


def gather_circuit(name: str) -> d.Circuit:
    return d.Circuit([d.Gather((SHAPES[name][0],), gather_index(name))])


def full_range_inputs(n: int, rounds: int = 6, seed: int = 1, M: int = M7) -> list:
    rng = np.random.default_rng(seed)
    lo, hi = -(M // 2), M - M // 2  # [lo, hi)
    out = []
    for r in range(rounds):
        x = rng.integers(lo, hi, n)
        edge = (lo, hi - 1, 0)
        x[0], x[-1] = edge[r % 3], edge[(r + 1) % 3]
        out.append(x.astype(np.int64))
    return out


def gather_inputs(name: str, rounds: int = 6) -> list:
    return full_range_inputs(SHAPES[name][0], rounds)


# ---------------------------------------------------------------- composite cases
def in_src_case(rounds: int = 6):
    """Conv -> Relu -> Gather(in_src = the conv) -> Add(the Relu): a permutation of the conv's (2, 4, 4) output, read
    from its saved copy, plus the ReLU of the same output."""
    rng = np.random.default_rng(7)
    conv = d.Conv2d.from_quantized(rng.integers(-3, 4, (2, 2, 3, 3)), rng.integers(-3, 4, 2), 4, 4, 2, 2, 3, 3, 1, 1,
                                   pad_width=1, pad_height=1)
    idx = rng.permutation(32)
    g = d.Gather((2, 4, 4), idx, (2, 4, 4))
    g.in_src = 0
    c = d.Circuit([conv, d.Relu((2, 4, 4)), g, d.Add((2, 4, 4), 1)])
    xs = [rng.integers(-9, 10, 32) for _ in range(rounds)]

    def want(x):
        y = conv.plain_q_eval(x, False)
        return y[idx] + np.maximum(y, 0)

    return c, xs, want


def repeats_relu_case(rounds: int = 6):
    """Five inputs fanned out to 12 wires, then a ReLU: every copy is a wire of its own with its own gate."""
    idx = np.array([0, 0, 1, 4, 4, 4, 2, 3, 3, 0, 1, 4])
    c = d.Circuit([d.Gather((5,), idx), d.Relu((12,))])
    xs = full_range_inputs(5, rounds, seed=3)
    return c, xs, lambda x: np.maximum(np.asarray(x)[idx], 0)


def argmax_case(rounds: int = 6):
    """ArgMax over 3 channels of a (3, 2, 4) tensor, then a Gather of the 8 index labels to 12 (reversed, with
    repeats): the layer moves whatever labels the walk carries behind an ArgMax."""
    idx = np.array([7, 6, 5, 4, 3, 2, 1, 0, 0, 7, 3, 3])
    c = d.Circuit([d.ArgMax((3, 2, 4)), d.Gather((1, 2, 4), idx)])
    rng = np.random.default_rng(5)
    xs = [rng.integers(-1000, 1000, 24) for _ in range(rounds)]
    return c, xs, lambda x: np.argmax(np.asarray(x).reshape(3, 8), axis=0)[idx]


SHUFFLE_UNIT = {"input": (4, 4, 4), "ops": [("shuffle_unit",)]}


def shuffle_unit_case(n_inputs: int = 6):
    """The zoo's ShuffleNetV2 unit on a (4, 4, 4) tensor under ScaleQuant(5), calibrated at k = 7."""
    return tiny_arch("_TINY_SHUFFLE_UNIT", SHUFFLE_UNIT, n_inputs=n_inputs)


def numpy_shuffle_unit(x, layers):
    """A ShuffleNetV2 basic unit in numpy on a float (C, H, W) tensor, written from the paper and not from the
    layer: split the channels in halves, right half through 1x1 conv + ReLU, depthwise 3x3 (pad 1), 1x1 conv + ReLU
    with the float weights of `layers` (the unit's three Conv2d layers), concat, channel shuffle with 2 groups."""
    C, H, W = x.shape
    h = C // 2
    left, r = x[:h], x[h:]
    pw1, dw, pw2 = layers

    def pointwise(t, l):
        return np.einsum("fc,chw->fhw", l.weights.reshape(h, h), t) + l.biases[:, None, None]

    r = np.maximum(pointwise(r, pw1), 0)
    p = np.pad(r, ((0, 0), (1, 1), (1, 1)))
    acc = np.zeros_like(r)
    for dy in range(3):
        for dx in range(3):
            acc += dw.weights.reshape(h, 3, 3)[:, dy, dx][:, None, None] * p[:, dy:dy + H, dx:dx + W]
    r = acc + dw.biases[:, None, None]
    r = np.maximum(pointwise(r, pw2), 0)
    cat = np.concatenate([left, r])
    return cat.reshape(2, h, H, W).transpose(1, 0, 2, 3).reshape(C, H, W)


def numpy_pixel_shuffle(x, r: int):
    """torch.nn.PixelShuffle on a (C r^2, H, W) tensor: out[c, h r + i, w r + j] = x[c r^2 + i r + j, h, w]."""
    C, H, W = x.shape
    c = C // (r * r)
    out = np.zeros((c, H * r, W * r), dtype=x.dtype)
    for i in range(r):
        for j in range(r):
            out[:, i::r, j::r] = x[i * r + j::r * r]
    return out
