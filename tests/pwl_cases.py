"""Shared layers, circuits and inputs of the PiecewiseLinear tests (tests/test_pwl.py on the host,
tests/test_gpu_pwl.py on the GPU).

A layer's input x must keep every sign input x - T_i and the output y a signed CRT value: |x| <= lim(layer, k).
The inputs hold every breakpoint, its two neighbours, one value inside every segment and both range ends, on the
first and last element of a wave (64) and of a tile (256) and on the last element.
"""
from __future__ import annotations

import numpy as np

import dash_amd as d
from dash_amd.ir.bases import crt_modulus, first_primes

M7 = crt_modulus(first_primes(7))
EDGES = (0, 1, 63, 64, 255, 256, -1)

# name -> (T, A, V, slope_bits). "m2": a hard-sigmoid shape (a positive and a negative step); "m8": the default
# sigmoid's integers at l = 5 (steps of both signs); "drop": the middle breakpoint's step is 0 and is dropped from
# the garbled form, the outer slopes are not 0; "k2" / "k4": layers small enough for the CRT bases 2 * 3 and
# 2 * 3 * 5 * 7.
SHAPES = {
    "m1": ([3], [0, 200], 17, 8),
    "m2": ([-50, 70], [0, 77, 0], -300, 8),
    "m8": ([-160, -96, -64, -32, 32, 64, 96, 160], [0, 5, 18, 38, 59, 38, 18, 5, 0], 55, 8),
    "drop": ([-40, 10, 33], [-30, 100, 100, -256], 1234, 7),
    "k2": ([-1, 1], [0, 1, 0], 0, 1),
    "k4": ([-5, 7], [0, 3, -1], 2, 2),
}


def _size(dims) -> int:
    return int(np.prod(dims, dtype=np.int64))


def shape_for(k: int, name: str = "m2") -> str:
    """The named shape, or the small layer that fits the base when k is small."""
    return "k2" if k <= 3 else ("k4" if k <= 4 else name)


def pwl_layer(dims, name: str = "m2"):
    T, A, V, s = SHAPES[name]
    return d.PiecewiseLinear.from_quantized(tuple(dims), T, A, V, s)


def pwl_circuit(dims, name: str = "m2"):
    """The layer alone: its input is the circuit input."""
    return d.Circuit([pwl_layer(dims, name)])


def expected(x, T, A, V) -> np.ndarray:
    """The quantized function segment by segment (numpy only, independent of the layer's ReLU sum): the knot values
    Y_1 = V, Y_(i+1) = Y_i + A_i (T_(i+1) - T_i); left of T_1 the line of slope A_0 through (T_1, V), in segment
    j >= 1 (T_j <= x < T_(j+1)) the line of slope A_j through (T_j, Y_j)."""
    x = np.asarray(x, dtype=np.int64).reshape(-1)
    T = [int(v) for v in T]
    A = [int(v) for v in A]
    Y = [int(V)]
    for i in range(1, len(T)):
        Y.append(Y[-1] + A[i] * (T[i] - T[i - 1]))
    out = np.empty_like(x)
    for n, v in enumerate(x):
        v = int(v)
        j = sum(1 for t in T if t <= v)  # breakpoints at or below v
        out[n] = V + A[0] * (v - T[0]) if j == 0 else Y[j - 1] + A[j] * (v - T[j - 1])
    return out


def want_of(layer):
    return lambda x: expected(x, layer.T, layer.A, layer.V)


def lim(layer, k: int) -> int:
    """The largest X such that for every |x| <= X all x - T_i and y(x) lie in [-M/2 + 1, M/2 - 1]."""
    h = crt_modulus(first_primes(k)) // 2 - 1
    T, A, V = layer.T, layer.A, layer.V
    tmax = int(np.abs(T).max())

    def ok(X):
        pts = np.array([-X, X] + [int(t) for t in T if abs(int(t)) <= X])
        return X + tmax <= h and int(np.abs(expected(pts, T, A, V)).max()) <= h

    lo, hi = 0, h
    assert ok(0), "the layer does not fit the base"
    while lo < hi:  # ok is monotone: the end segments are lines
        mid = (lo + hi + 1) // 2
        if ok(mid):
            lo = mid
        else:
            hi = mid - 1
    return lo


def cardinal(layer, k: int) -> list:
    """Every breakpoint, its two neighbours, one value inside every segment and both range ends."""
    L = lim(layer, k)
    T = [int(t) for t in layer.T]
    vals = [-L, L]
    for t in T:
        vals += [t - 1, t, t + 1]
    inner = [-L] + T + [L]
    vals += [(a + b) // 2 for a, b in zip(inner[:-1], inner[1:])]
    return [v for v in dict.fromkeys(vals) if -L <= v <= L]


def pwl_inputs(dims, layer, k: int = 7, rounds: int = 2, seed: int = 1) -> list:
    N = _size(dims)
    L = lim(layer, k)
    rng = np.random.default_rng(seed)
    card = cardinal(layer, k)
    at = sorted({e % N for e in EDGES if -N <= e < N})
    out = []
    for r in range(rounds):
        x = rng.integers(-L, L + 1, N)
        # the cardinal values: on the edge elements first, the rest from element 2 on where there is room
        for i, e in enumerate(at):
            x[e] = card[(i + r) % len(card)]
        free = [e for e in range(N) if e not in at][:len(card)]
        for i, e in enumerate(free):
            x[e] = card[(i + r) % len(card)]
        out.append(x.astype(np.int64))
    return out


def conv_chain(name: str = "m2", l: int = 3):
    """conv(1 -> 2 channels, 1x1) on a (1, 8, 17) image -> Rescale(l) -> PiecewiseLinear on (2, 8, 17) = 272
    elements. Quantized parameters given directly."""
    conv = d.Conv2d.from_quantized(np.array([3, -5]).reshape(2, 1, 1, 1), np.array([2, -1]), 17, 8, 1, 2, 1, 1)
    dims = (2, 8, 17)
    return d.Circuit([conv, d.Rescale(l, dims), pwl_layer(dims, name)])


def conv_chain_inputs(rounds: int = 2, amp: int = 400, seed: int = 6) -> list:
    """Inputs of conv_chain: after the conv and Rescale(3) the layer sees about +-amp * 5 / 8, which covers the
    m2 and m8 breakpoints."""
    rng = np.random.default_rng(seed)
    out = []
    for r in range(rounds):
        x = rng.integers(-amp, amp + 1, 136)
        x[[0, 63, 64, 135]] = [0, -1, 1, (-amp, amp)[r % 2]]
        out.append(x.astype(np.int64))
    return out


# ---------------------------------------------------------------- the kernel's digit formula on the host
def modq(x: np.ndarray, p: int) -> np.ndarray:
    """dev.h modq for an odd modulus on uint32 lanes: d = mulhi(x, mq), mq = floor(2^32 / q), r = x - d q, one
    correction."""
    x = np.asarray(x, dtype=np.uint64)
    dq = (x * np.uint64((1 << 32) // p)) >> np.uint64(32)
    r = x - dq * np.uint64(p)
    return np.where(r >= p, r - np.uint64(p), r)
