"""Circuits and inputs shared by tests/test_bilinear.py (host) and tests/test_gpu_bilinear.py (GPU): docs/BILINEAR.md.

SHAPES: name -> (input dims, Bilinear keywords). The GPU shapes are the smallest at which each kernel form can go
wrong (tests/test_gpu_bilinear.py says what each is for)."""
import numpy as np

import dash_amd as d
from dash_amd.ir.bases import crt_modulus, first_primes

M7 = crt_modulus(first_primes(7))
B3 = [5, 7, 131]
SEED = bytes(range(16))

SHAPES = {
    "dword1080": ((3, 9, 10), dict(factors=2)),                         # (3, 18, 20): OW % 4 == 0, Nout = 1080
    "byte_f2x3": ((2, 3, 5), dict(factors=(2, 3))),                     # (2, 6, 15): OW % 4 != 0, fx = 3 non-dyadic
    "one_row": ((4, 1, 4), dict(factors=2)),                            # (4, 2, 8): both row taps are the same row
    "corners7x8": ((1, 4, 4), dict(size=(7, 8), mode="align_corners")),  # non-integer factor, weights 0 and 2^b
}
DWORD = ["dword1080", "one_row", "corners7x8"]
BYTE = ["byte_f2x3"]


def layer(name):
    dims, kw = SHAPES[name]
    return d.Bilinear(dims, **kw)


def bilinear_circuit(name):
    return d.Circuit([layer(name)])


def inputs(c, n, lim=20, seed=1):
    rng = np.random.default_rng(seed)
    return [rng.integers(-lim, lim + 1, c.input_size) for _ in range(n)]


def conv_bilinear_conv(rng, relu=True, **kw):
    """Conv2d 3x3 -> Bilinear(**kw) -> Conv2d 1x1 (in_scale_bits = s) -> Rescale(2 + s) [-> Relu] on a (2, 4, 5)
    input: the second conv's bias sits at the scale of its products, 2^s above the first conv's, and the rescale
    takes the pending bits out again."""
    c1 = d.Conv2d.from_quantized(rng.integers(-4, 5, (3, 2, 3, 3)), rng.integers(-5, 6, 3), 5, 4, 2, 3, 3, 3,
                                 pad_width=1, pad_height=1)
    bl = d.Bilinear(c1.out_dims, **(kw or dict(factors=2)))
    s = bl.scale_bits
    c2 = d.Conv2d.from_quantized(rng.integers(-4, 5, (2, 3, 1, 1)), rng.integers(-5, 6, 2) << s, bl.out_dims[2],
                                 bl.out_dims[1], 3, 2, 1, 1)
    c2.in_scale_bits = s
    layers = [c1, bl, c2, d.Rescale(2 + s, c2.out_dims)]
    if relu:
        layers.append(d.Relu(c2.out_dims))
    return d.Circuit(layers)


def bilinear_argmax(dims=(4, 3, 3), f=2):
    bl = d.Bilinear(dims, f)
    return d.Circuit([bl, d.ArgMax(bl.out_dims)])


def torch_bilinear(x, l):
    """F.interpolate of the (C, H, W) tensor x in float64, flat."""
    import torch

    t = torch.tensor(np.asarray(x, dtype=np.float64).reshape(l.in_dims))[None]
    y = torch.nn.functional.interpolate(t, size=(l.OH, l.OW), mode="bilinear", align_corners=l.mode == "align_corners")
    return y[0].numpy().reshape(-1)
