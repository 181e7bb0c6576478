"""Shared circuits and inputs of the multi-head MatMul tests (tests/test_matmul_heads.py on the host,
tests/test_gpu_matmul_heads.py on the GPU), built like tests/matmul_cases.py.

A case is (G, M, T, N): G heads, each an M x T by T x N contraction. Its circuit reads one input tensor, x itself
(dims (G M, T), or (G T, M) with trans_a: G slabs). The second operand y is a public selection of x through a 0 / 1
dense layer (layer 0): y's flat element e is x's flat element (G M T - 1 - e) mod (G M T), in y's stored layout
((G T, N), or (G N, T) with trans_b). The MatMul reads x through in_src = -1 and y through src = 0.

Operands come from [-lim, lim] with lim = floor(sqrt((M7 // 2 - 1) / T)), so every sum of T products is a signed CRT
value at k = 7. Full rows of x and columns of y are set to +-lim and zeros on the first and last output of every
head (where a kernel's head arithmetic can go wrong) and on the last output overall; where a row and a column share
elements of x the row's write wins.
"""
from __future__ import annotations

import numpy as np

import dash_amd as d
from tests.matmul_cases import M7, PAIRS, lim_of  # noqa: F401


def x_dims(G, M, T, N, ta=False, tb=False):
    return (G * T, M) if ta else (G * M, T)


def y_dims(G, M, T, N, ta=False, tb=False):
    return (G * N, T) if tb else (G * T, N)


def y_index(G, M, T, N) -> np.ndarray:
    """Index into flat x of every flat element of y."""
    return (G * M * T - 1 - np.arange(G * T * N)) % (G * M * T)


def _xf(M, T, ta, g, i, t):
    return g * M * T + (t * M + i if ta else i * T + t)


def _yf(T, N, tb, g, t, l):
    return g * T * N + (l * T + t if tb else t * N + l)


def heads_circuit(G, M, T, N, ta=False, tb=False, out_dims=None, **kw):
    """kw: heads=G unless the caller leaves the keyword out on purpose (G = 1 built without it)."""
    idx = y_index(G, M, T, N)
    w = np.zeros((idx.size, G * M * T), dtype=np.int64)
    w[np.arange(idx.size), idx] = 1
    sel = d.Dense.from_quantized(w, np.zeros(idx.size, dtype=np.int64))
    kw.setdefault("heads", G)
    if kw["heads"] is None:
        del kw["heads"]
    mm = d.MatMul(x_dims(G, M, T, N, ta, tb), 0, y_dims(G, M, T, N, ta, tb), trans_a=ta, trans_b=tb, out_dims=out_dims,
                  **kw)
    mm.in_src = -1
    return d.Circuit([sel, mm])


def edge_outputs(G, M, N) -> list:
    """The first and last output of every head; the last of the last head is the last output overall."""
    return sorted({g * M * N + e for g in range(G) for e in (0, M * N - 1)})


def heads_inputs(G, M, T, N, ta=False, tb=False, rounds: int = 2, seed: int = 1) -> list:
    lim = lim_of(T)
    rng = np.random.default_rng(seed)
    idx = y_index(G, M, T, N)
    out = []
    for r in range(rounds):
        x = rng.integers(-lim, lim + 1, G * M * T)
        for n, o in enumerate(edge_outputs(G, M, N)):
            a, b = PAIRS[(n + r) % len(PAIRS)]
            g, rem = divmod(o, M * N)
            i, l = divmod(rem, N)
            for t in range(T):
                x[idx[_yf(T, N, tb, g, t, l)]] = b * lim  # the element y_g[t, l] reads
            for t in range(T):
                x[_xf(M, T, ta, g, i, t)] = a * lim       # the later write wins where both fall on one element
        out.append(x.astype(np.int64))
    return out


def operands(G, M, T, N, x, ta=False, tb=False):
    """x and y as [G][M][T] and [G][T][N] int64, by plain reshapes of the flat tensors."""
    x = np.asarray(x, dtype=np.int64)
    y = x[y_index(G, M, T, N)]
    a = x.reshape((G, T, M) if ta else (G, M, T))
    b = y.reshape((G, N, T) if tb else (G, T, N))
    return (a.transpose(0, 2, 1) if ta else a), (b.transpose(0, 2, 1) if tb else b)


def expected(G, M, T, N, x, ta=False, tb=False) -> np.ndarray:
    """The per-head contraction by numpy's einsum on int64, independent of the layer's own code."""
    a, b = operands(G, M, T, N, x, ta, tb)
    return np.einsum("git,gtl->gil", a, b).reshape(-1)


def gram_heads_circuit(G, M, T):
    """x_g x_g^T per head: src names the layer's own input (the circuit input) with trans_b."""
    return d.Circuit([d.MatMul((G * M, T), -1, (G * M, T), trans_b=True, heads=G)])


def gram_heads_inputs(G, M, T, rounds: int = 2, seed: int = 4) -> list:
    lim = lim_of(T)
    rng = np.random.default_rng(seed)
    out = []
    for r in range(rounds):
        x = rng.integers(-lim, lim + 1, (G, M, T))
        x[:, 0] = lim        # out[g, 0, 0] = T lim^2, the largest value
        x[:, M - 1] = -lim   # out[g, 0, M - 1] = -T lim^2
        if M > 2:
            x[:, 1] = 0
        out.append(x.reshape(-1).astype(np.int64))
    return out


def gram_heads_expected(G, M, T, x) -> np.ndarray:
    a = np.asarray(x, dtype=np.int64).reshape(G, M, T)
    return np.einsum("git,glt->gil", a, a).reshape(-1)


# ---------------------------------------------------------------- head isolation: x and y as separate slices
def split_circuit(G, M, T, N):
    """The circuit input is x (G M T elements) followed by y (G T N); two 0 / 1 dense layers select them, so a
    test controls both operands of every head independently. G = 1: the single-head layer, built without the
    keyword."""
    nx, ny = G * M * T, G * T * N
    wy = np.zeros((ny, nx + ny), dtype=np.int64)
    wy[np.arange(ny), nx + np.arange(ny)] = 1
    wx = np.zeros((nx, nx + ny), dtype=np.int64)
    wx[np.arange(nx), np.arange(nx)] = 1
    sel_y = d.Dense.from_quantized(wy, np.zeros(ny, dtype=np.int64))
    sel_x = d.Dense.from_quantized(wx, np.zeros(nx, dtype=np.int64))
    sel_x.in_src = -1
    mm = d.MatMul((G * M, T), 0, (G * T, N), heads=G) if G > 1 else d.MatMul((M, T), 0, (T, N))
    return d.Circuit([sel_y, sel_x, mm])


# ---------------------------------------------------------------- a small architecture for the zoo tests
# 8 x 8 input, strided to 4 x 4 (L = 16), a 2-head attention block on 4 channels (dh = 2)
TINY_ATTENTION = {"input": (1, 8, 8), "ops": [("conv", 4, 3, 2, 1), ("relu",), ("attention", 2), ("relu",), ("gap",),
                                              ("flatten",), ("fc", 3)]}


# ---------------------------------------------------------------- range guard
def guard_heads_case():
    """Two heads of a (1, 2) x (2, 1) contraction, y = x through an identity dense layer: out_g = x_g0^2 + x_g1^2,
    first read by a Rescale(1). Inputs: in range; head 1 alone beyond M7 / 2; head 0 alone beyond it."""
    sel = d.Dense.from_quantized(np.eye(4, dtype=np.int64), np.zeros(4, dtype=np.int64))
    mm = d.MatMul((2, 2), 0, (4, 1), heads=2, out_dims=(2,))
    mm.in_src = -1
    c = d.Circuit([sel, mm, d.Rescale(1, (2,))])
    big = 400  # 2 * 400^2 = 320000 > M7 / 2 = 255255 > 400^2 + 3^2
    return c, [np.array([3, -4, 5, 6]), np.array([3, -4, big, -big]), np.array([big, big, 1, 2]),
               np.array([big, 3, -3, big])], [False, True, True, False]
