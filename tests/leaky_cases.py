"""Shared circuits and inputs of the LeakyRelu tests (tests/test_leaky_relu.py on the host,
tests/test_gpu_leaky_relu.py on the GPU).

A LeakyRelu(slope_bits = s) multiplies by up to 2^s, so its input x must keep 2^s |x| a signed CRT value:
|x| <= lim(k, s) = (M_k / 2 - 1) >> s. The edge values 0, -1, 1 and +-lim sit on the first and last element of a
wave (64) and of a tile (256), next to every channel boundary, and on the last element.
"""
from __future__ import annotations

import numpy as np

import dash_amd as d
from dash_amd.ir.bases import crt_modulus, first_primes

M7 = crt_modulus(first_primes(7))
EDGES = (0, 1, 63, 64, 255, 256, -1)


def _size(dims) -> int:
    return int(np.prod(dims, dtype=np.int64))


def lim(k: int, s: int) -> int:
    return (crt_modulus(first_primes(k)) // 2 - 1) >> s


def expected(x, n, s: int, bc: int = 0) -> np.ndarray:
    """The quantized leaky ReLU written out: 2^s x for x >= 0, n_c x below, channel c = e // bc (numpy only,
    independent of the layer's code)."""
    x = np.asarray(x, dtype=np.int64).reshape(-1)
    n = np.asarray(n, dtype=np.int64).reshape(-1)
    ne = np.full(x.size, n[0]) if n.size == 1 else n[np.arange(x.size) // bc]
    y = np.empty_like(x)
    pos = x >= 0
    y[pos] = x[pos] * (1 << s)
    y[~pos] = x[~pos] * ne[~pos]
    return y


def slopes(C: int, s: int) -> list:
    """Per-channel numerators that include n = 0 and n = 2^s - 1."""
    top = (1 << s) - 1
    base = [0, top, 1, top // 2 + 1, 2]
    return [base[c % len(base)] % (top + 1) for c in range(C)]


def leaky_layer(dims, s: int = 4, per_channel: bool = False, n: int = 3):
    dims = tuple(dims)
    return d.LeakyRelu.from_quantized(dims, slopes(dims[0], s) if per_channel else n % (1 << s), s)


def leaky_circuit(dims, s: int = 4, per_channel: bool = False):
    """The layer alone: its input is the circuit input."""
    return d.Circuit([leaky_layer(dims, s, per_channel)])


def leaky_inputs(dims, k: int = 7, s: int = 4, rounds: int = 2, seed: int = 1) -> list:
    N = _size(dims)
    L = lim(k, s)
    bc = N // dims[0] if len(dims) > 1 else N
    rng = np.random.default_rng(seed)
    cardinal = [0, -1, 1, -L, L, -2, 2]
    at = sorted({e % N for e in EDGES if -N <= e < N} |
                {b + o for b in range(bc, N, bc) for o in (-1, 0) if 0 <= b + o < N})
    out = []
    for r in range(rounds):
        x = rng.integers(-L, L + 1, N)
        for i, e in enumerate(at):
            x[e] = cardinal[(i + r) % len(cardinal)]
        out.append(x.astype(np.int64))
    return out


def conv_chain(l: int = 3, s: int = 3, per_channel: bool = True, second: bool = False, seed: int = 4):
    """conv(1 -> 2 channels, 1x1) on a (1, 8, 17) image -> Rescale(l) -> LeakyRelu(s) on (2, 8, 17) = 272 elements;
    with `second`, -> conv(2 -> 2, 1x1, in_scale_bits = s) -> Rescale(l + s). Quantized parameters given directly."""
    rng = np.random.default_rng(seed)
    conv = d.Conv2d.from_quantized(np.array([3, -5]).reshape(2, 1, 1, 1), np.array([2, -1]), 17, 8, 1, 2, 1, 1)
    dims = (2, 8, 17)
    layers = [conv, d.Rescale(l, dims), leaky_layer(dims, s, per_channel)]
    if second:
        from dash_amd.ir.quant import QuantizationMethod as Q

        # float parameters that quantize exactly: w 2^l in [-3, 3], b 2^(2l + s) = (5, -7) 2^s
        w = rng.integers(-3, 4, (2, 2, 1, 1)).astype(np.float32) / (1 << l)
        b = np.array([5, -7], dtype=np.float32) / (1 << (2 * l))
        conv2 = d.Conv2d(w, b, 17, 8, 2, 2, 1, 1, q_parameter=l, q_method=Q.ScaleQuant, in_scale_bits=s)
        assert conv2.q_biases.tolist() == [5 << s, -(7 << s)]
        layers += [conv2, d.Rescale(l + s, dims)]
    return d.Circuit(layers)


def conv_chain_inputs(rounds: int = 2, amp: int = 2000, seed: int = 6) -> list:
    rng = np.random.default_rng(seed)
    out = []
    for r in range(rounds):
        x = rng.integers(-amp, amp + 1, 136)
        x[[0, 63, 64, 135]] = [0, -1, 1, (-amp, amp)[r % 2]]
        out.append(x.astype(np.int64))
    return out


def rescale_leaky(k: int, N: int, l: int, per_channel: bool):
    """Rescale(l) + LeakyRelu(s = min(l, 4)) on the circuit input, the joint construction's smallest circuit.
    2^s ceil(x / 2^l) stays a signed CRT value for every x of the rescale's domain because s <= l."""
    s = min(l, 4)
    C = 3 if N % 3 == 0 else (5 if N % 5 == 0 else 1)
    dims = (C, N // C) if per_channel and C > 1 else (N,)
    return d.Circuit([d.Rescale(l, dims), leaky_layer(dims, s, per_channel and C > 1, n=1)])


# ---------------------------------------------------------------- the kernel's digit formula on the host
def modc_magic(p: int) -> int:
    """ModC.mq of csrc/hip/dev.h: floor(2^32 / q)."""
    return (1 << 32) // p


def modq(x: np.ndarray, p: int) -> np.ndarray:
    """dev.h modq for an odd modulus on uint32 lanes: d = mulhi(x, mq), r = x - d q, one correction."""
    x = np.asarray(x, dtype=np.uint64)
    dq = (x * np.uint64(modc_magic(p))) >> np.uint64(32)
    r = x - dq * np.uint64(p)
    return np.where(r >= p, r - np.uint64(p), r)
