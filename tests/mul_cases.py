"""Shared circuits and inputs of the Mul tests (tests/test_mul.py on the host, tests/test_gpu_mul.py on the GPU).

At k = 7 the CRT modulus is M = 510510. Operands come from [-505, 505]: 505^2 = 255025 < M / 2 = 255255, so every
product is a signed CRT value. The pairs (+-505, +-505), (-505, 505) and zeros sit on the first and last element of
a wave (64) and of a tile (256) and on the last element.

A case's circuit reads one input tensor x of the layer's dims. The second operand y is a public selection of x
through a 0 / 1 dense layer (layer 0), so both operands are secret label tensors and both are under the test's
control; the Mul reads x itself through in_src = -1 and y through src = 0:
  elementwise  y[e] = x[N - 1 - e]
  broadcast    y[c] = x[c * bc]          (the first element of channel c)
  square       no second operand, the circuit is the Mul alone.
"""
from __future__ import annotations

import numpy as np

import dash_amd as d
from dash_amd.ir.bases import crt_modulus, first_primes

M7 = crt_modulus(first_primes(7))
LIM = 505
assert LIM * LIM < M7 // 2
EDGES = (0, 63, 64, 255, 256, -1)
# (x, y) on the edge elements, in turn
PAIRS = ((LIM, LIM), (-LIM, -LIM), (-LIM, LIM), (0, LIM), (LIM, 0), (LIM, -LIM), (0, 0))


def _size(dims) -> int:
    return int(np.prod(dims, dtype=np.int64))


def y_index(dims, kind: str) -> np.ndarray:
    """Index into x of every element of y (see the module docstring)."""
    N = _size(dims)
    if kind == "elem":
        return np.arange(N)[::-1].copy()
    bc = _size(dims[1:])
    return np.arange(dims[0]) * bc


def mul_circuit(dims, kind: str):
    """kind: "elem", "bc1" (src_dims (C,)), "bc3" (src_dims (C, 1, 1)) or "sq"."""
    dims = tuple(dims)
    if kind == "sq":
        return d.Circuit([d.Mul.square(dims)])
    N = _size(dims)
    idx = y_index(dims, kind)
    w = np.zeros((idx.size, N), dtype=np.int64)
    w[np.arange(idx.size), idx] = 1
    sel = d.Dense.from_quantized(w, np.zeros(idx.size, dtype=np.int64))
    sd = None if kind == "elem" else ((dims[0],) if kind == "bc1" else (dims[0], 1, 1))
    mul = d.Mul(dims, 0, sd)
    mul.in_src = -1
    return d.Circuit([sel, mul])


def mul_inputs(dims, kind: str, rounds: int = 2, lim: int = LIM, seed: int = 1) -> list:
    """`rounds` input vectors; every product stays within lim^2."""
    N = _size(dims)
    rng = np.random.default_rng(seed)
    pairs = [(np.sign(a) * lim, np.sign(b) * lim) for a, b in PAIRS]
    out = []
    for r in range(rounds):
        x = rng.integers(-lim, lim + 1, N)
        edges = sorted({e % N for e in EDGES if -N <= e < N})
        if kind == "sq":
            for n, e in enumerate(edges):
                x[e] = pairs[(n + r) % len(pairs)][0]
        else:
            idx = y_index(dims, kind)
            rep = N // idx.size
            for n, e in enumerate(edges):
                a, b = pairs[(n + r) % len(pairs)]
                x[idx[e // rep]] = b  # the element y reads for output e
                x[e] = a              # the later write wins where both fall on one element
        out.append(x.astype(np.int64))
    return out


def expected(dims, kind: str, x: np.ndarray) -> np.ndarray:
    """The product by plain numpy, independent of the layer's own code."""
    x = np.asarray(x, dtype=np.int64)
    if kind == "sq":
        return x * x
    idx = y_index(dims, kind)
    return x * np.repeat(x[idx], x.size // idx.size)


# ---------------------------------------------------------------- small architectures for the zoo tests
TINY_SE = {"input": (2, 6, 6), "ops": [("conv", 4, 3, 1, 1), ("se", 2), ("relu",), ("gap",), ("flatten",), ("fc", 3)]}
TINY_SQUARE = {"input": (1, 6, 6), "ops": [("conv", 2, 3, 2, 1), ("square",), ("flatten",), ("fc", 6), ("square",),
                                           ("fc", 3)]}


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
def guard_case(M: int = M7):
    """Mul((4,)) square then Rescale(1): the product is first read by the rescale. Inputs: just inside (the largest
    product below the rescale's limit), and one whose product reaches M / 2."""
    c = d.Circuit([d.Mul.square((4,)), d.Rescale(1, (4,))])
    lim = c.layers[1].mrs_limit(M)
    a = int(np.floor(np.sqrt(lim - 1)))
    b = int(np.ceil(np.sqrt(M // 2)))
    assert a * a < lim <= M // 2 <= b * b
    xs = [np.array([a, -a, 0, 3]), np.array([1, b, 0, 3]), np.array([-b, 1, 2, 3])]
    return c, xs, [False, True, True]
