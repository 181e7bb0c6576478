"""Shared circuits and inputs of the MatMul tests (tests/test_matmul.py on the host, tests/test_gpu_matmul.py on the
GPU).

At k = 7 the CRT modulus is M7 = 510510. A case (M, T, N) draws its operands from [-lim, lim] with
lim = floor(sqrt((M7 // 2 - 1) / T)), so T lim^2 < M7 / 2 and every sum of T products is a signed CRT value.

A case's circuit reads one input tensor, x itself (dims (M, T), or (T, M) with trans_a). The second operand y is a
public selection of x through a 0 / 1 dense layer (layer 0): y's flat element e is x's flat element
(M T - 1 - e) mod (M T), in y's stored layout ((T, N), or (N, T) with trans_b). Both operands are secret label
tensors under the test's control; the MatMul reads x through in_src = -1 and y through src = 0.

Full rows of x and columns of y are set to (+lim, +lim), (-lim, +lim), zeros and their mirror images on the first
and last output of a wave (64) and of a tile (256) and on the last output, so an output's T products all have the
extreme value lim^2, -lim^2 or 0 wherever the row and the column fall on different elements of x; where they share
elements (y is a selection of x) the row's write wins, and with M = 1 only the same-sign extremes are reachable.
"""
from __future__ import annotations

import math

import numpy as np

import dash_amd as d
from dash_amd.ir.bases import crt_modulus, first_primes

M7 = crt_modulus(first_primes(7))
EDGES = (0, 63, 64, 255, 256, -1)
# (x row, y column) signs on the edge outputs, in turn
PAIRS = ((1, 1), (-1, 1), (0, 0), (-1, -1), (1, -1), (0, 1), (1, 0))


def lim_of(T: int, M: int = M7) -> int:
    lim = math.isqrt((M // 2 - 1) // T)
    assert T * lim * lim <= M // 2 - 1 < T * (lim + 1) * (lim + 1)  # floor(sqrt((M // 2 - 1) / T)): nothing wraps
    return lim


def x_dims(M, T, N, ta=False, tb=False):
    return (T, M) if ta else (M, T)


def y_dims(M, T, N, ta=False, tb=False):
    return (N, T) if tb else (T, N)


def y_index(M, T, N, ta=False, tb=False) -> np.ndarray:
    """Index into flat x of every flat element of y (see the module docstring)."""
    return (M * T - 1 - np.arange(T * N)) % (M * T)


def _xf(M, T, ta, i, t):
    return t * M + i if ta else i * T + t


def _yf(T, N, tb, t, l):
    return l * T + t if tb else t * N + l


def matmul_circuit(M, T, N, ta=False, tb=False, out_dims=None):
    idx = y_index(M, T, N, ta, tb)
    w = np.zeros((idx.size, M * T), dtype=np.int64)
    w[np.arange(idx.size), idx] = 1
    sel = d.Dense.from_quantized(w, np.zeros(idx.size, dtype=np.int64))
    mm = d.MatMul(x_dims(M, T, N, ta, tb), 0, y_dims(M, T, N, ta, tb), trans_a=ta, trans_b=tb, out_dims=out_dims)
    mm.in_src = -1
    return d.Circuit([sel, mm])


def matmul_inputs(M, T, N, ta=False, tb=False, rounds: int = 2, lim=None, seed: int = 1) -> list:
    """`rounds` input vectors; every sum of T products stays within T lim^2."""
    lim = lim_of(T) if lim is None else lim
    rng = np.random.default_rng(seed)
    idx = y_index(M, T, N, ta, tb)
    edges = sorted({e % (M * N) for e in EDGES if -(M * N) <= e < M * N})
    out = []
    for r in range(rounds):
        x = rng.integers(-lim, lim + 1, M * T)
        for n, o in enumerate(edges):
            a, b = PAIRS[(n + r) % len(PAIRS)]
            i, l = divmod(o, N)
            for t in range(T):
                x[idx[_yf(T, N, tb, t, l)]] = b * lim  # the element y[t, l] reads
            for t in range(T):
                x[_xf(M, T, ta, i, t)] = a * lim       # the later write wins where both fall on one element
        out.append(x.astype(np.int64))
    return out


def expected(M, T, N, x, ta=False, tb=False) -> np.ndarray:
    """The contraction by numpy's @ on int64, independent of the layer's own code."""
    x = np.asarray(x, dtype=np.int64)
    y = x[y_index(M, T, N, ta, tb)].reshape(y_dims(M, T, N, ta, tb))
    a = x.reshape(x_dims(M, T, N, ta, tb))
    return ((a.T if ta else a) @ (y.T if tb else y)).reshape(-1)


def gram_circuit(M, T):
    """x x^T: src names the layer's own input (the circuit input) with trans_b."""
    return d.Circuit([d.MatMul((M, T), -1, (M, T), trans_b=True)])


def gram_inputs(M, T, rounds: int = 2, seed: int = 4) -> list:
    lim = lim_of(T)
    rng = np.random.default_rng(seed)
    out = []
    for r in range(rounds):
        x = rng.integers(-lim, lim + 1, (M, T))
        x[0] = lim          # out[0, 0] = T lim^2, the largest value
        x[M - 1] = -lim     # out[0, M - 1] = -T lim^2, out[M - 1, M - 1] = T lim^2
        if M > 2:
            x[1] = 0
        out.append(x.reshape(-1).astype(np.int64))
    return out


def gram_expected(M, T, x) -> np.ndarray:
    a = np.asarray(x, dtype=np.int64).reshape(M, T)
    return (a @ a.T).reshape(-1)


# ---------------------------------------------------------------- a small architecture for the zoo tests
# 8 x 8 input, pooled to 4 x 4 (H W = 16), a non-local block on 4 channels with reduction 2
TINY_NONLOCAL = {"input": (1, 8, 8), "ops": [("conv", 4, 3, 2, 1), ("relu",), ("nonlocal", 2), ("relu",), ("gap",),
                                             ("flatten",), ("fc", 3)]}


def tiny_arch(name: str, arch: dict, n_inputs: int = 2):
    """The circuit of a test-only architecture (registered in zoo.ARCHS for the call, as tests/test_clip.py does)
    under ScaleQuant(5), with inputs, calibrated at k = 7."""
    from dash_amd.ir.quant import QuantizationMethod as Q
    from dash_amd.models import zoo

    zoo.ARCHS[name] = arch
    try:
        c = zoo.build_circuit(name, Q.ScaleQuant, 5, seed=2)
        xs = zoo.quantized_inputs(name, n_inputs, Q.ScaleQuant, 5, seed=5)
    finally:
        del zoo.ARCHS[name]
    c.calibrate(xs, M7)
    assert c.required_crt_modulus() <= M7, "the tiny architecture must fit k = 7"
    return c, xs


# ---------------------------------------------------------------- range guard
def _four_squares(s: int):
    """Non-negative (a, b, c, e) with a^2 + b^2 + c^2 + e^2 = s (Lagrange), the largest a first."""
    for a in range(math.isqrt(s), -1, -1):
        ra = s - a * a
        for b in range(math.isqrt(ra), -1, -1):
            rb = ra - b * b
            for c in range(math.isqrt(rb), -1, -1):
                e = math.isqrt(rb - c * c)
                if e * e == rb - c * c:
                    return a, b, c, e
    raise AssertionError(s)


def guard_case(M: int = M7):
    """MatMul((1, 4)) of x with itself as a column (y = x through an identity dense layer), then Rescale(1): the sum
    of squares is first read by the rescale. Inputs: one whose sum is the largest value below the rescale's limit,
    one whose sum is M / 2 exactly, one beyond it."""
    sel = d.Dense.from_quantized(np.eye(4, dtype=np.int64), np.zeros(4, dtype=np.int64))
    mm = d.MatMul((1, 4), 0, (4, 1), out_dims=(1,))
    mm.in_src = -1
    c = d.Circuit([sel, mm, d.Rescale(1, (1,))])
    lim = c.layers[2].mrs_limit(M)
    assert lim <= M // 2
    inside = np.array(_four_squares(lim - 1)) * np.array([1, -1, 1, -1])
    reach = np.array(_four_squares(M // 2)) * np.array([-1, 1, 1, 1])
    beyond = np.array(_four_squares(M // 2 + 7))
    assert int((inside * inside).sum()) == lim - 1 and int((reach * reach).sum()) == M // 2
    return c, [inside, reach, beyond], [False, True, True]
