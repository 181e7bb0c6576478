"""Model zoo: the paper's architectures (models/train_pytorch.ipynb, SURVEY
Appendix B) plus LeNet-5, VGG-16 and ResNet-18 for CIFAR-10, built directly in
the IR with random (PyTorch-default) initialisation and quantized with one of
Dash's three schemes. Rescale layers are auto-inserted after every linear
layer exactly like the ONNX loader does (onnx_modelloader.h:263-270, :334-341).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np

from ..ir.circuit import Circuit
from ..ir.layers import (Add, ArgMax, Bilinear, Clip, Concat, Conv2d, ConvTranspose2d, Dense, Flatten, Gather, LeakyRelu, MatMul, MaxPool2d, Mul,
                         PiecewiseLinear, Relu,
                         Rescale, Sign, SumPool2d, Upsample)
from ..ir.quant import QuantizationMethod, quantize_input

# architecture ops: ("conv", out_ch, k, stride, pad) | ("relu",) | ("sign",) | ("flatten",) | ("fc", out)
#                   | ("maxpool", k, s) | ("res", [ops...]) residual block | ("sumpool", k)
#                   | ("dwconv", k, stride, pad) depthwise conv (groups = channels, F = C)
#                   | ("maxpool", k, s, pad, ceil_mode) | ("gap",) global sum pool (the average's 1/K is left to
#                   the next linear layer) | ("fire", squeeze, e1, e3) SqueezeNet fire module: 1x1 squeeze + ReLU,
#                   then a 1x1 and a padded 3x3 expand (each + ReLU) that both read the squeeze output, then Concat
#                   | ("relu6",) = Clip(0, 6) | ("clip", lo, hi) clamp with float bounds (quantized with the
#                   scheme's activation scale; refused under SimpleQuant)
#                   | ("argmax",) index of the largest value along the first axis (the class of a logit vector,
#                   the per-pixel class of a (C, H, W) score map); scale-free
#                   | ("convt", out_ch, k, stride, pad, out_pad) transposed conv (+ the scheme's rescale, as conv)
#                   | ("up", f) nearest-neighbour upsampling by f
#                   | ("conv", out_ch, k, stride, pad, dilation) and ("dwconv", k, stride, pad, dilation): the
#                   optional last element dilates the kernel (atrous conv)
#                   | ("aspp", out_ch, rates) atrous spatial pyramid: one padded 3x3 conv per rate with
#                   pad = dilation = rate (same size out), each + ReLU, all reading the same tensor, then Concat
#                   | ("skip",) remember the current tensor | ("cat",) channel concat of the most recent open skip
#                   with the current tensor, skip first (an encoder-decoder's skip connection)
#                   | ("leaky", alpha) LeakyRelu with the dyadic slope round(alpha 2^s) / 2^s, s = leaky_bits, and
#                   ("prelu",) the same with one slope per channel (PyTorch's initial 0.25): ScaleQuant only; the
#                   output's 2^s passes through relu / maxpool / sumpool / gap / flatten / up to the next conv or fc,
#                   which quantizes its bias at 2^(2l + s) and rescales by l + s (docs/LEAKY_RELU.md)
#                   | ("square",) x^2 (a polynomial activation) + the scheme's rescale, as after a conv
#                   | ("se", r) squeeze-and-excitation: the current (C, H, W) tensor is kept, then gap, a 1x1 conv to
#                   C / r + ReLU, a 1x1 conv to C, Clip(0, 1) (a hard sigmoid's range) and the channel-broadcast Mul
#                   of the kept tensor with that gate + the scheme's rescale (refused under SimpleQuant, as a clip)
#                   | ("nonlocal", r) the dot-product non-local block of Wang et al. (normaliser 1 / N, no softmax) on
#                   a (C, H, W) tensor with H W <= 64: 1x1 convs phi, g, theta to C / r channels (each + the scheme's
#                   rescale), f = MatMul(theta^T, phi) of dims (H W, H W) + rescale, y = MatMul(g, f^T) of dims
#                   (C / r, H, W) + rescale, a 1x1 conv back to C whose weights carry the 1 / (H W), and the Add of
#                   the block's input (docs/MATMUL.md)
#                   | ("attention", heads) softmax-free multi-head attention, relu(Q K^T / sqrt(dh)) / L V (Wortsman et
#                   al. 2023), on a (C, H, W) tensor with heads | C and L = H W <= 64: 1x1 convs k, v, q to C channels
#                   (each + the scheme's rescale; q's weights carry 1 / sqrt(dh), dh = C / heads), the scores
#                   S = MatMul(q^T, k) per head of dims (heads L, L) + rescale + ReLU, the mix O = MatMul(v, S^T) per
#                   head of dims (C, H, W) + rescale, a 1x1 conv back to C whose weights carry the 1 / L, and the Add
#                   of the block's input (docs/MATMUL.md, Heads)
#                   | ("sigmoid",) | ("tanh",) | ("hsigmoid", alpha, beta) piecewise-linear activations
#                   (PiecewiseLinear.sigmoid / .tanh / .hard_sigmoid, slope bits pwl_bits): ScaleQuant only, no
#                   pending scale on their input; the output's 2^pwl_bits travels like a leaky ReLU's (docs/PWL.md)
#                   | ("se", r, "sigmoid") the same block gated by the piecewise-linear sigmoid instead of
#                   Clip(0, 1): the Mul's rescale is then l + pwl_bits (ScaleQuant only)
#                   | ("shuffle", g) channel shuffle with g groups and ("d2s", r) depth-to-space by r (PixelShuffle, the
#                   ONNX mode CRD; ("d2s", r, "DCR") for the other): Gather layers, free and value-preserving
#                   | ("shuffle_unit",) the ShuffleNetV2 basic unit on a (C, H, W) tensor with C even: the first half
#                   of the channels is kept (a Gather), the second half (a Gather reading the unit's input) goes
#                   through a 1x1 conv + ReLU, a depthwise 3x3 and a 1x1 conv + ReLU (each conv + the scheme's
#                   rescale), then the Concat of both and a shuffle with 2 groups (docs/GATHER.md)
#                   | ("bilinear", f) bilinear upsampling by f in mode half_pixel (PyTorch's align_corners=False), or
#                   ("bilinear", f, mode) with mode align_corners / asymmetric: ScaleQuant only; the output's
#                   2^(by + bx) travels like a leaky ReLU's to the next conv or fc, an ("argmax",) or ("sign",) drops
#                   it, and a ("cat",) needs the same pending bits on both operands (docs/BILINEAR.md)
ARCHS: dict[str, dict] = {
    "MODEL_A": {"input": (1, 28, 28), "ops": [("flatten",), ("fc", 128), ("relu",), ("fc", 128), ("relu",), ("fc", 10)]},
    # MODEL_A whose decoded output is the class alone, not the ten logits
    "MODEL_A_ARGMAX": {"input": (1, 28, 28), "ops": [("flatten",), ("fc", 128), ("relu",), ("fc", 128), ("relu",), ("fc", 10),
                                                     ("argmax",)]},
    "MODEL_B_POOL_REPL": {"input": (1, 28, 28), "ops": [
        ("conv", 5, 5, 1, 0), ("relu",), ("conv", 5, 3, 3, 0), ("relu",), ("conv", 10, 3, 1, 0), ("relu",),
        ("conv", 10, 3, 3, 0), ("flatten",), ("fc", 100), ("relu",), ("fc", 10)]},
    "MODEL_C": {"input": (1, 28, 28), "ops": [
        ("conv", 5, 4, 2, 0), ("relu",), ("flatten",), ("fc", 100), ("relu",), ("fc", 10)]},
    "MODEL_D_POOL_REPL": {"input": (1, 28, 28), "ops": [
        ("conv", 16, 6, 2, 0), ("relu",), ("conv", 16, 6, 2, 0), ("relu",), ("flatten",), ("fc", 100), ("relu",),
        ("fc", 10)]},
    "MODEL_E_30": {"input": (1, 28, 28), "ops": [("flatten",), ("fc", 30), ("sign",), ("fc", 10)]},
    "MODEL_E_100": {"input": (1, 28, 28), "ops": [("flatten",), ("fc", 100), ("sign",), ("fc", 10)]},
    "MODEL_F_MINIONN_POOL_REPL": {"input": (3, 32, 32), "ops": [
        ("conv", 64, 3, 1, 0), ("relu",), ("conv", 64, 3, 1, 0), ("relu",), ("conv", 64, 2, 2, 0),
        ("conv", 64, 3, 1, 0), ("relu",), ("conv", 64, 3, 1, 0), ("relu",), ("conv", 64, 2, 2, 0),
        ("conv", 64, 3, 1, 0), ("relu",), ("conv", 64, 1, 1, 0), ("relu",), ("conv", 16, 1, 1, 0), ("relu",),
        ("flatten",), ("fc", 10)]},
    "MODEL_F_GNNP_POOL_REPL": {"input": (3, 32, 32), "ops": [
        ("conv", 32, 3, 1, 0), ("relu",), ("conv", 32, 3, 1, 0), ("relu",), ("conv", 32, 2, 2, 0),
        ("conv", 64, 3, 1, 0), ("relu",), ("conv", 64, 3, 1, 0), ("relu",), ("conv", 64, 2, 2, 0),
        ("conv", 128, 3, 1, 0), ("relu",), ("conv", 128, 3, 1, 0), ("relu",), ("flatten",), ("fc", 10)]},
    # beyond the reference (BASELINE configs 2, 4, 5)
    "LENET5": {"input": (1, 28, 28), "ops": [
        ("conv", 6, 5, 1, 2), ("relu",), ("maxpool", 2, 2), ("conv", 16, 5, 1, 0), ("relu",), ("maxpool", 2, 2),
        ("flatten",), ("fc", 120), ("relu",), ("fc", 84), ("relu",), ("fc", 10)]},
    "VGG16": {"input": (3, 32, 32), "ops": [
        ("conv", 64, 3, 1, 1), ("relu",), ("conv", 64, 3, 1, 1), ("relu",), ("maxpool", 2, 2),
        ("conv", 128, 3, 1, 1), ("relu",), ("conv", 128, 3, 1, 1), ("relu",), ("maxpool", 2, 2),
        ("conv", 256, 3, 1, 1), ("relu",), ("conv", 256, 3, 1, 1), ("relu",), ("conv", 256, 3, 1, 1), ("relu",),
        ("maxpool", 2, 2),
        ("conv", 512, 3, 1, 1), ("relu",), ("conv", 512, 3, 1, 1), ("relu",), ("conv", 512, 3, 1, 1), ("relu",),
        ("maxpool", 2, 2),
        ("conv", 512, 3, 1, 1), ("relu",), ("conv", 512, 3, 1, 1), ("relu",), ("conv", 512, 3, 1, 1), ("relu",),
        ("maxpool", 2, 2), ("flatten",), ("fc", 512), ("relu",), ("fc", 10)]},
    "RESNET18": {"input": (3, 32, 32), "ops": [
        ("conv", 64, 3, 1, 1), ("relu",),
        ("res", 64, 1), ("res", 64, 1), ("res", 128, 2), ("res", 128, 1),
        ("res", 256, 2), ("res", 256, 1), ("res", 512, 2), ("res", 512, 1),
        ("sumpool", 4), ("flatten",), ("fc", 10)]},
    # depthwise-separable CIFAR net (MobileNet style): dense stem, then depthwise 3x3 / 1x1 blocks
    "MODEL_DWSEP_CIFAR": {"input": (3, 32, 32), "ops": [
        ("conv", 16, 3, 1, 1), ("relu",),
        ("dwconv", 3, 2, 1), ("relu",), ("conv", 32, 1, 1, 0), ("relu",),
        ("dwconv", 3, 2, 1), ("relu",), ("conv", 64, 1, 1, 0), ("relu",),
        ("dwconv", 3, 1, 1), ("relu",), ("conv", 64, 1, 1, 0), ("relu",),
        ("sumpool", 4), ("flatten",), ("fc", 10)]},
    # MODEL_DWSEP_CIFAR's topology with the MobileNet family's ReLU6 activations and a global-average head
    "MOBILENET_CIFAR": {"input": (3, 32, 32), "ops": [
        ("conv", 16, 3, 1, 1), ("relu6",),
        ("dwconv", 3, 2, 1), ("relu6",), ("conv", 32, 1, 1, 0), ("relu6",),
        ("dwconv", 3, 2, 1), ("relu6",), ("conv", 64, 1, 1, 0), ("relu6",),
        ("dwconv", 3, 1, 1), ("relu6",), ("conv", 64, 1, 1, 0), ("relu6",),
        ("gap",), ("flatten",), ("fc", 10)]},
    # a small CIFAR net with one dot-product non-local block (reduction 2) on its 8 x 8 stage: f is a
    # (64, 16, 64) contraction, y a (16, 64, 64) one
    "NONLOCAL_CIFAR": {"input": (3, 32, 32), "ops": [
        ("conv", 16, 3, 1, 1), ("relu",), ("maxpool", 2, 2), ("conv", 32, 3, 2, 1), ("relu",), ("nonlocal", 2),
        ("relu",), ("gap",), ("flatten",), ("fc", 10)]},
    # a small CIFAR net with one 4-head ReLU-attention block on its 4 x 4 stage of 32 channels (dh = 8, L = 16): the
    # scores are a (16, 8, 16) contraction per head (the blocked kernel form), the mix an (8, 16, 16) one (the lane form)
    "RELU_ATTN_CIFAR": {"input": (3, 32, 32), "ops": [
        ("conv", 16, 3, 2, 1), ("relu",), ("conv", 32, 3, 2, 1), ("relu",), ("maxpool", 2, 2), ("attention", 4),
        ("relu",), ("gap",), ("flatten",), ("fc", 10)]},
    # MOBILENET_CIFAR with a squeeze-and-excitation gate (reduction 4) behind every pointwise conv
    "SE_MOBILENET_CIFAR": {"input": (3, 32, 32), "ops": [
        ("conv", 16, 3, 1, 1), ("relu6",),
        ("dwconv", 3, 2, 1), ("relu6",), ("conv", 32, 1, 1, 0), ("se", 4), ("relu6",),
        ("dwconv", 3, 2, 1), ("relu6",), ("conv", 64, 1, 1, 0), ("se", 4), ("relu6",),
        ("dwconv", 3, 1, 1), ("relu6",), ("conv", 64, 1, 1, 0), ("se", 4), ("relu6",),
        ("gap",), ("flatten",), ("fc", 10)]},
    # the CryptoNets MNIST network: squares are the only non-linearity (no sign anywhere)
    # DarkNet-style CIFAR net (the tiny-YOLO backbone's pattern): 3x3 convs with LeakyReLU(0.1) and 2x2 max pools
    # (32 -> 16 -> 8 -> 4 -> 2), a 1x1 classifier conv, a global average and a dense head
    "DARKNET_TINY_CIFAR": {"input": (3, 32, 32), "ops": [
        ("conv", 8, 3, 1, 1), ("leaky", 0.1), ("maxpool", 2, 2),
        ("conv", 16, 3, 1, 1), ("leaky", 0.1), ("maxpool", 2, 2),
        ("conv", 32, 3, 1, 1), ("leaky", 0.1), ("maxpool", 2, 2),
        ("conv", 32, 3, 1, 1), ("leaky", 0.1), ("maxpool", 2, 2),
        ("conv", 16, 1, 1, 0), ("leaky", 0.1), ("gap",), ("flatten",), ("fc", 10)]},
    # LeNet-5 in its original form: tanh activations (piecewise-linear, docs/PWL.md) instead of ReLUs
    "LENET5_TANH_MNIST": {"input": (1, 28, 28), "ops": [
        ("conv", 6, 5, 1, 2), ("tanh",), ("maxpool", 2, 2), ("conv", 16, 5, 1, 0), ("tanh",), ("maxpool", 2, 2),
        ("flatten",), ("fc", 120), ("tanh",), ("fc", 84), ("tanh",), ("fc", 10)]},
    # a small squeeze-and-excitation CIFAR net whose gates are sigmoids, as in the SE paper
    "SE_SIGMOID_CIFAR": {"input": (3, 32, 32), "ops": [
        ("conv", 8, 3, 2, 1), ("relu",), ("conv", 16, 3, 2, 1), ("se", 4, "sigmoid"), ("relu",),
        ("conv", 16, 3, 2, 1), ("se", 4, "sigmoid"), ("relu",), ("gap",), ("flatten",), ("fc", 10)]},
    "CRYPTONETS_MNIST": {"input": (1, 28, 28), "ops": [
        ("conv", 5, 5, 2, 1), ("square",), ("flatten",), ("fc", 100), ("square",), ("fc", 10)]},
    # SqueezeNet-style CIFAR net: a stride-2 stem (32 -> 16), ceil-mode 3x3/2 max pools whose last window is cut at
    # the edge (16 -> 8 -> 4), two fire modules, a 1x1 classifier conv and a global average over the 4x4 plane
    "SQUEEZENET_CIFAR": {"input": (3, 32, 32), "ops": [
        ("conv", 16, 3, 2, 1), ("relu",), ("maxpool", 3, 2, 0, True),
        ("fire", 8, 16, 16), ("maxpool", 3, 2, 0, True), ("fire", 8, 16, 16),
        ("conv", 10, 1, 1, 0), ("gap",), ("flatten",)]},
    # small U-Net: two stride-2 encoder steps (32 -> 16 -> 8), a transposed-conv and a nearest-neighbour decoder
    # step, each concatenated with the encoder tensor of its size, and a per-pixel class map (1, 32, 32) of 4 classes
    "UNET_CIFAR": {"input": (3, 32, 32), "ops": [
        ("conv", 8, 3, 1, 1), ("relu",), ("skip",),
        ("conv", 16, 3, 2, 1), ("relu",), ("skip",),
        ("conv", 32, 3, 2, 1), ("relu",),
        ("convt", 16, 2, 2, 0, 0), ("relu",), ("cat",),
        ("conv", 16, 3, 1, 1), ("relu",),
        ("up", 2), ("cat",),
        ("conv", 8, 3, 1, 1), ("relu",),
        ("conv", 4, 1, 1, 0), ("argmax",)]},
    # atrous segmentation head: a stride-2 stem (32 -> 16), one 3x3, an ASPP of rates 1, 2, 4 (3 x 16 channels), a
    # 1x1 fuse, the 4-class 1x1 scores, the per-pixel class and its upsampling back to the (1, 32, 32) input grid
    "ASPP_SEG_CIFAR": {"input": (3, 32, 32), "ops": [
        ("conv", 16, 3, 2, 1), ("relu",),
        ("conv", 16, 3, 1, 1), ("relu",),
        ("aspp", 16, (1, 2, 4)),
        ("conv", 16, 1, 1, 0), ("relu",),
        ("conv", 4, 1, 1, 0), ("argmax",), ("up", 2)]},
    # UNET_CIFAR with both decoder steps written as the up-conv: bilinear upsampling, then a 3x3 conv (which absorbs
    # the upsampling's pending scale bits before the concat) + ReLU
    "UNET_BILINEAR_CIFAR": {"input": (3, 32, 32), "ops": [
        ("conv", 8, 3, 1, 1), ("relu",), ("skip",),
        ("conv", 16, 3, 2, 1), ("relu",), ("skip",),
        ("conv", 32, 3, 2, 1), ("relu",),
        ("bilinear", 2), ("conv", 16, 3, 1, 1), ("relu",), ("cat",),
        ("conv", 16, 3, 1, 1), ("relu",),
        ("bilinear", 2), ("conv", 8, 3, 1, 1), ("relu",), ("cat",),
        ("conv", 8, 3, 1, 1), ("relu",),
        ("conv", 4, 1, 1, 0), ("argmax",)]},
    # ASPP_SEG_CIFAR with DeepLab's head: the 4-class scores are upsampled bilinearly to the input grid, then the
    # per-pixel class (1, 32, 32) is taken (the ArgMax drops the upsampling's scale)
    "DEEPLAB_HEAD_CIFAR": {"input": (3, 32, 32), "ops": [
        ("conv", 16, 3, 2, 1), ("relu",),
        ("conv", 16, 3, 1, 1), ("relu",),
        ("aspp", 16, (1, 2, 4)),
        ("conv", 16, 1, 1, 0), ("relu",),
        ("conv", 4, 1, 1, 0), ("bilinear", 2), ("argmax",)]},
    # ShuffleNetV2-style CIFAR net: a strided stem (32 -> 16 -> 8), two basic units on the (16, 8, 8) stage, a global
    # average and a dense head
    "SHUFFLENET_V2_CIFAR": {"input": (3, 32, 32), "ops": [
        ("conv", 8, 3, 2, 1), ("relu",), ("conv", 16, 3, 2, 1), ("relu",),
        ("shuffle_unit",), ("shuffle_unit",), ("gap",), ("flatten",), ("fc", 10)]},
    # sub-pixel segmentation head: a stride-2 encoder (32 -> 16), a 1x1 conv to 4 r^2 = 16 channels, PixelShuffle by
    # r = 2 back to the (4, 32, 32) score map of 4 classes and the per-pixel class (1, 32, 32)
    "SUBPIXEL_SEG_CIFAR": {"input": (3, 32, 32), "ops": [
        ("conv", 8, 3, 2, 1), ("relu",), ("conv", 16, 3, 1, 1), ("relu",),
        ("conv", 16, 1, 1, 0), ("d2s", 2), ("argmax",)]},
}

ALIASES = {"MINIONN": "MODEL_F_MINIONN_POOL_REPL", "GNNP": "MODEL_F_GNNP_POOL_REPL", "MLP": "MODEL_A",
           "MNIST_MLP": "MODEL_A", "LENET": "LENET5", "VGG": "VGG16", "RESNET": "RESNET18"}


@dataclass
class ModelConfig:
    name: str
    q_method: QuantizationMethod = QuantizationMethod.ScaleQuant
    q_parameter: int = 5
    q_const: float = 0.02
    seed: int = 0
    width_mult: float = 1.0


def canonical(name: str) -> str:
    n = name.upper()
    return ALIASES.get(n, n)


def _init(rng, shape, fan_in):
    bound = 1.0 / np.sqrt(fan_in)
    return rng.uniform(-bound, bound, size=shape).astype(np.float32)


def build_circuit(name: str, q_method: QuantizationMethod = QuantizationMethod.ScaleQuant, q_parameter: int = 5,
                  q_const: float = 0.02, seed: int = 0, weights: Optional[dict] = None, leaky_bits: int = 4,
                  pwl_bits: int = 8) -> Circuit:
    """Random-init (or given float weights) circuit with Dash quantization. leaky_bits: the slope bits of the
    ("leaky", alpha) and ("prelu",) ops; pwl_bits: those of the ("sigmoid",), ("tanh",), ("hsigmoid", ...) ops and
    of a sigmoid-gated ("se", r, "sigmoid")."""
    arch = ARCHS[canonical(name)]
    rng = np.random.default_rng(seed)
    C, H, W = arch["input"]
    dims = (C, H, W)
    layers = []
    qm = QuantizationMethod(q_method)

    pend = [0]  # pending scale bits of the current tensor (a LeakyRelu's 2^s, docs/LEAKY_RELU.md)

    def rescale_after(d, e=0):
        if qm == QuantizationMethod.ScaleQuant:
            layers.append(Rescale(q_parameter + e, d))
        elif qm == QuantizationMethod.ScaleQuantPlus:
            layers.append(Rescale([q_parameter], d))

    def conv(cout, k, s, p, cin, h, w, groups=1, dil=1, wscale=1.0):
        fan_in = cin // groups * k * k
        wt = _init(rng, (cout, cin // groups, k, k), fan_in) * np.float32(wscale)
        bs = _init(rng, (cout,), fan_in)
        c = Conv2d(wt, bs, w, h, cin, cout, k, k, s, s, q_parameter, qm, q_const, pad_width=p, pad_height=p,
                   groups=groups, dilation_width=dil, dilation_height=dil, in_scale_bits=pend[0])
        layers.append(c)
        rescale_after(c.out_dims, pend[0])
        pend[0] = 0
        return c.out_dims

    skips = []  # open ("skip",) marks: (layer index, dims, pending scale bits)
    for op in arch["ops"]:
        kind = op[0]
        if pend[0] and kind not in ("conv", "dwconv", "fc", "relu", "leaky", "prelu", "maxpool", "sumpool", "gap",
                                    "flatten", "up", "shuffle", "d2s", "bilinear", "argmax", "sign", "skip", "cat"):
            raise NotImplementedError(f"{name}: op {len(layers)} ({kind}): a leaky ReLU's 2^{pend[0]} scale reaches it "
                                      "before a conv or fc could absorb it")
        if kind == "convt":
            _, cout, k, s, p, op_ = op
            fan_in = cout * k * k  # PyTorch's ConvTranspose2d default: fan-in of the [C][F][k][k] weight's axis 1
            wt = _init(rng, (dims[0], cout, k, k), fan_in)
            bs = _init(rng, (cout,), fan_in)
            ct = ConvTranspose2d(wt, bs, dims[2], dims[1], dims[0], cout, k, k, s, s, q_parameter, qm, q_const,
                                 pad_width=p, pad_height=p, out_pad_width=op_, out_pad_height=op_)
            layers.append(ct)
            dims = ct.out_dims
            rescale_after(dims)
        elif kind == "up":
            up = Upsample(dims, op[1])
            layers.append(up)
            dims = up.out_dims
        elif kind == "bilinear":
            if qm != QuantizationMethod.ScaleQuant:
                raise ValueError(f"{name}: op {len(layers)} (bilinear): a bilinear resize exists under ScaleQuant only "
                                 "(its 2^s output scale needs a power-of-two rescale behind it)")
            bl = Bilinear(dims, op[1], mode=op[2] if len(op) > 2 else "half_pixel")
            layers.append(bl)
            dims = bl.out_dims
            pend[0] += bl.scale_bits
        elif kind == "shuffle":
            layers.append(Gather.channel_shuffle(dims, op[1]))
        elif kind == "d2s":
            ps = Gather.depth_to_space(dims, op[1], op[2] if len(op) > 2 else "CRD")
            layers.append(ps)
            dims = ps.out_dims
        elif kind == "shuffle_unit":
            if len(dims) != 3 or dims[0] % 2:
                raise ValueError(f"{name}: op {len(layers)} (shuffle_unit): needs a (C, H, W) tensor of an even channel "
                                 f"count, got {dims}")
            cin, h, w = dims
            src, half = len(layers) - 1, cin // 2
            keep = Gather.slice(dims, 0, 0, half)
            layers.append(keep)
            left = len(layers) - 1
            right = Gather.slice(dims, 0, half, cin)
            right.in_src = src  # both halves read the tensor the unit was given
            layers.append(right)
            d_b = conv(half, 1, 1, 0, half, h, w)
            layers.append(Relu(d_b))
            d_b = conv(half, 3, 1, 1, half, h, w, groups=half)
            d_b = conv(half, 1, 1, 0, half, h, w)
            layers.append(Relu(d_b))
            cat = Concat([keep.out_dims, d_b], [left, len(layers) - 1])
            layers.append(cat)
            layers.append(Gather.channel_shuffle(cat.out_dims, 2))
        elif kind == "skip":
            skips.append((len(layers) - 1, dims, pend[0]))
        elif kind == "cat":
            if not skips:
                raise ValueError(f"{name}: ('cat',) without an open ('skip',)")
            src, sd, sbits = skips.pop()
            if sbits != pend[0]:
                raise NotImplementedError(f"{name}: op {len(layers)} (cat): the skip tensor carries 2^{sbits} pending "
                                          f"scale and the current tensor 2^{pend[0]}: a Concat needs equal bits")
            cat = Concat([sd, dims], [src, len(layers) - 1])
            layers.append(cat)
            dims = cat.out_dims
        elif kind == "flatten":
            layers.append(Flatten(dims))
            dims = (int(np.prod(dims)),)
        elif kind == "fc":
            fin = int(np.prod(dims))
            wt = _init(rng, (op[1], fin), fin)
            bs = _init(rng, (op[1],), fin)
            d = Dense(wt, bs, q_parameter, qm, q_const, in_scale_bits=pend[0])
            layers.append(d)
            dims = d.out_dims
            rescale_after(dims, pend[0])
            pend[0] = 0
        elif kind == "conv":
            _, cout, k, s, p = op[:5]
            dims = conv(cout, k, s, p, dims[0], dims[1], dims[2], dil=op[5] if len(op) > 5 else 1)
        elif kind == "dwconv":
            _, k, s, p = op[:4]
            dims = conv(dims[0], k, s, p, dims[0], dims[1], dims[2], groups=dims[0], dil=op[4] if len(op) > 4 else 1)
        elif kind == "aspp":
            _, cout, rates = op
            src = len(layers) - 1  # every branch reads the tensor the module was given
            cin, h, w = dims
            ends, bdims = [], []
            for bi, rate in enumerate(rates):
                first = len(layers)
                d_b = conv(cout, 3, 1, rate, cin, h, w, dil=rate)
                if bi:  # the first branch reads the previous layer anyway
                    layers[first].in_src = src
                layers.append(Relu(d_b))
                ends.append(len(layers) - 1)
                bdims.append(d_b)
            cat = Concat(bdims, ends)
            layers.append(cat)
            dims = cat.out_dims
        elif kind == "relu":
            layers.append(Relu(dims))
        elif kind in ("leaky", "prelu"):
            if qm != QuantizationMethod.ScaleQuant:
                raise ValueError(f"{name}: op {len(layers)} ({kind}): a leaky ReLU exists under ScaleQuant only (its "
                                 "2^s output scale needs a power-of-two rescale behind it)")
            alpha = float(op[1]) if kind == "leaky" else np.full(dims[0], 0.25, np.float32)
            layers.append(LeakyRelu(dims, alpha, leaky_bits))
            pend[0] += leaky_bits
        elif kind in ("sigmoid", "tanh", "hsigmoid"):
            if qm != QuantizationMethod.ScaleQuant:
                raise ValueError(f"{name}: op {len(layers)} ({kind}): a piecewise-linear activation exists under "
                                 "ScaleQuant only (its 2^s output scale needs a power-of-two rescale behind it)")
            if kind == "hsigmoid":
                layers.append(PiecewiseLinear.hard_sigmoid(dims, op[1], op[2], pwl_bits, q_parameter, qm))
            else:
                layers.append(getattr(PiecewiseLinear, kind)(dims, pwl_bits, q_parameter, qm))
            pend[0] += pwl_bits
        elif kind == "sign":
            layers.append(Sign(dims))
            pend[0] = 0  # scale-free: a pending 2^e ends here
        elif kind in ("relu6", "clip"):
            lo, hi = (0.0, 6.0) if kind == "relu6" else (op[1], op[2])
            if qm == QuantizationMethod.SimpleQuant:
                raise ValueError(f"{name}: op {len(layers)} ({kind}): a clip layer has no quantization under "
                                 "SimpleQuant (no single activation scale); use ScaleQuant or ScaleQuantPlus")
            layers.append(Clip(dims, lo, hi, q_parameter, qm))
        elif kind == "square":
            layers.append(Mul.square(dims))
            rescale_after(dims)
        elif kind == "se":
            if len(dims) != 3 or dims[0] % op[1]:
                raise ValueError(f"{name}: op {len(layers)} (se): needs a (C, H, W) tensor whose channels {op[1]} divides")
            gate = op[2] if len(op) > 2 else "clip"
            if gate not in ("clip", "sigmoid"):
                raise ValueError(f"{name}: op {len(layers)} (se): the gate is 'clip' or 'sigmoid', got {gate!r}")
            if gate == "sigmoid" and qm != QuantizationMethod.ScaleQuant:
                raise ValueError(f"{name}: op {len(layers)} (se): a sigmoid gate exists under ScaleQuant only (its 2^s "
                                 "output scale needs a power-of-two rescale behind it)")
            if qm == QuantizationMethod.SimpleQuant:
                raise ValueError(f"{name}: op {len(layers)} (se): its Clip(0, 1) gate has no quantization under "
                                 "SimpleQuant (no single activation scale); use ScaleQuant or ScaleQuantPlus")
            full, fd = len(layers) - 1, dims
            sp = SumPool2d(fd[2], fd[1], fd[0], fd[2], fd[1])
            layers.append(sp)
            d_sq = conv(fd[0] // op[1], 1, 1, 0, fd[0], 1, 1)
            layers.append(Relu(d_sq))
            d_ex = conv(fd[0], 1, 1, 0, d_sq[0], 1, 1)
            if gate == "sigmoid":
                layers.append(PiecewiseLinear.sigmoid(d_ex, pwl_bits, q_parameter, qm))
            else:
                layers.append(Clip(d_ex, 0.0, 1.0, q_parameter, qm))
            mul = Mul(fd, len(layers) - 1, (fd[0], 1, 1))
            mul.in_src = full  # the full tensor is the Mul's input, the gate its operand
            layers.append(mul)
            rescale_after(fd, pwl_bits if gate == "sigmoid" else 0)  # the gate's 2^s leaves with the product's
        elif kind == "nonlocal":
            r = op[1]
            if len(dims) != 3 or dims[0] % r:
                raise ValueError(f"{name}: op {len(layers)} (nonlocal): needs a (C, H, W) tensor whose channels {r} "
                                 "divides")
            cin, h, w = dims
            if h * w > 64:
                raise ValueError(f"{name}: op {len(layers)} (nonlocal): the affinity matrix has (H W)^2 entries of C / r "
                                 f"products each; pool first so that H W <= 64, got {h} x {w}")
            src, cr = len(layers) - 1, cin // r
            d_e = conv(cr, 1, 1, 0, cin, h, w)  # phi reads the previous layer
            phi = len(layers) - 1
            first = len(layers)
            conv(cr, 1, 1, 0, cin, h, w)
            layers[first].in_src = src
            g_out = len(layers) - 1
            first = len(layers)
            conv(cr, 1, 1, 0, cin, h, w)
            layers[first].in_src = src
            # f = theta^T phi, (H W, H W): the pairwise affinities
            f = MatMul(d_e, phi, d_e, trans_a=True)
            layers.append(f)
            rescale_after(f.out_dims)
            # y = g f^T, back to (C / r, H, W)
            y = MatMul(d_e, len(layers) - 1, f.out_dims, trans_b=True, out_dims=d_e)
            y.in_src = g_out
            layers.append(y)
            rescale_after(d_e)
            conv(cin, 1, 1, 0, cr, h, w, wscale=1.0 / (h * w))  # the normaliser 1 / N rides on the weights
            layers.append(Add(dims, src))
        elif kind == "attention":
            nh = int(op[1])
            if len(dims) != 3 or nh < 1 or dims[0] % nh:
                raise ValueError(f"{name}: op {len(layers)} (attention): needs a (C, H, W) tensor whose channels "
                                 f"{nh} heads divide, got {dims}")
            cin, h, w = dims
            L_ = h * w
            if L_ > 64:
                raise ValueError(f"{name}: op {len(layers)} (attention): the scores have heads (H W)^2 entries of C / "
                                 f"heads products each; pool first so that H W <= 64, got {h} x {w}")
            src, dh = len(layers) - 1, cin // nh
            conv(cin, 1, 1, 0, cin, h, w)  # k reads the previous layer
            k_out = len(layers) - 1
            first = len(layers)
            conv(cin, 1, 1, 0, cin, h, w)
            layers[first].in_src = src
            v_out = len(layers) - 1
            first = len(layers)
            conv(cin, 1, 1, 0, cin, h, w, wscale=1.0 / np.sqrt(dh))  # q carries the 1 / sqrt(dh)
            layers[first].in_src = src
            # S_g = q_g^T k_g, (L, L) per head: row = query token, column = key token
            sc = MatMul(dims, k_out, dims, trans_a=True, heads=nh, out_dims=(nh * L_, L_))
            layers.append(sc)
            rescale_after(sc.out_dims)
            layers.append(Relu(sc.out_dims))
            # O_g = v_g S_g^T, (dh, L) per head, back to (C, H, W)
            mix = MatMul(dims, len(layers) - 1, sc.out_dims, trans_b=True, heads=nh, out_dims=dims)
            mix.in_src = v_out
            layers.append(mix)
            rescale_after(dims)
            conv(cin, 1, 1, 0, cin, h, w, wscale=1.0 / L_)  # the normaliser 1 / L rides on the weights
            layers.append(Add(dims, src))
        elif kind == "argmax":
            am = ArgMax(dims)
            layers.append(am)
            dims = am.out_dims
            pend[0] = 0  # scale-free: a pending 2^e ends here
        elif kind == "maxpool":
            k, s = op[1], op[2]
            pad, ceil = (op[3], op[4]) if len(op) > 3 else (0, False)
            mp = MaxPool2d(dims[2], dims[1], dims[0], k, k, s, s, pad_width=pad, pad_height=pad, ceil_mode=ceil)
            layers.append(mp)
            dims = mp.out_dims
        elif kind == "sumpool":
            sp = SumPool2d(dims[2], dims[1], dims[0], op[1], op[1])
            layers.append(sp)
            dims = sp.out_dims
        elif kind == "gap":
            sp = SumPool2d(dims[2], dims[1], dims[0], dims[2], dims[1])
            layers.append(sp)
            dims = sp.out_dims
        elif kind == "fire":
            _, sq, e1, e3 = op
            d_sq = conv(sq, 1, 1, 0, dims[0], dims[1], dims[2])
            layers.append(Relu(d_sq))
            squeeze = len(layers) - 1
            d1 = conv(e1, 1, 1, 0, sq, d_sq[1], d_sq[2])
            layers.append(Relu(d1))
            left = len(layers) - 1
            first3 = len(layers)
            d3 = conv(e3, 3, 1, 1, sq, d_sq[1], d_sq[2])
            layers[first3].in_src = squeeze  # the 3x3 expand reads the squeeze output, not the 1x1 expand
            layers.append(Relu(d3))
            cat = Concat([d1, d3], [left, len(layers) - 1])
            layers.append(cat)
            dims = cat.out_dims
        elif kind == "res":
            _, cout, stride = op
            cin = dims[0]
            src = len(layers) - 1  # index of the layer whose output feeds the block
            d1 = conv(cout, 3, stride, 1, cin, dims[1], dims[2])
            layers.append(Relu(d1))
            d2 = conv(cout, 3, 1, 1, cout, d1[1], d1[2])
            if stride != 1 or cin != cout:
                # projection shortcut: 1x1 conv reading the block input (in_src), then add the main path
                main_last = len(layers) - 1
                sc = len(layers)
                conv(cout, 1, stride, 0, cin, dims[1], dims[2])
                layers[sc].in_src = src
                layers.append(Add(d2, main_last))
            else:
                layers.append(Add(d2, src))
            layers.append(Relu(d2))
            dims = d2
        else:
            raise ValueError(f"unknown op {kind}")
    if pend[0]:
        raise NotImplementedError(f"{name}: the output carries a pending 2^{pend[0]} scale that no conv or fc absorbed")
    return Circuit(layers, q_parameter)


def input_dims(name: str):
    return ARCHS[canonical(name)]["input"]


def synthetic_inputs(name: str, n: int, seed: int = 1) -> list[np.ndarray]:
    """CIFAR/MNIST-shaped normalized synthetic images (no dataset download)."""
    rng = np.random.default_rng(seed)
    C, H, W = input_dims(name)
    return [np.clip(rng.standard_normal(C * H * W), -2.5, 2.5).astype(np.float32) for _ in range(n)]


def quantized_inputs(name: str, n: int, q_method=QuantizationMethod.ScaleQuant, q_parameter: int = 5,
                     q_const: float = 0.02, seed: int = 1) -> list[np.ndarray]:
    return [quantize_input(x, QuantizationMethod(q_method), q_parameter, q_const) for x in synthetic_inputs(name, n, seed)]


# Benchmark configurations (benchmarks/model_benchmarks/non_sgx/main.cpp:227-335)
BENCH_CONFIGS = {
    "MODEL_F_MINIONN_POOL_REPL/DASH": dict(model="MODEL_F_MINIONN_POOL_REPL", q_method=QuantizationMethod.ScaleQuant,
                                          q_parameter=5, crt=7, mrs=100.0),
    "MODEL_F_GNNP_POOL_REPL/DASH": dict(model="MODEL_F_GNNP_POOL_REPL", q_method=QuantizationMethod.ScaleQuant,
                                       q_parameter=5, crt=7, mrs=100.0),
    "MODEL_F_MINIONN_POOL_REPL/REDASH_OPT": dict(model="MODEL_F_MINIONN_POOL_REPL",
                                                q_method=QuantizationMethod.ScaleQuantPlus, q_parameter=32,
                                                crt=[32, 97, 107], mrs=[22, 19, 15, 13]),
    "MODEL_F_GNNP_POOL_REPL/REDASH_OPT": dict(model="MODEL_F_GNNP_POOL_REPL",
                                             q_method=QuantizationMethod.ScaleQuantPlus, q_parameter=32,
                                             crt=[32, 167, 173], mrs=[26, 25, 21, 13]),
    "MODEL_F_MINIONN_POOL_REPL/REDASH_CPM": dict(model="MODEL_F_MINIONN_POOL_REPL",
                                                q_method=QuantizationMethod.ScaleQuantPlus, q_parameter=32,
                                                crt=[32, 3, 5, 7, 11, 13, 17], mrs=[10, 9, 9, 8, 7, 7, 6]),
    "MODEL_DWSEP_CIFAR/DASH": dict(model="MODEL_DWSEP_CIFAR", q_method=QuantizationMethod.ScaleQuant, q_parameter=5,
                                   crt=7, mrs=100.0),
    "MOBILENET_CIFAR/DASH": dict(model="MOBILENET_CIFAR", q_method=QuantizationMethod.ScaleQuant, q_parameter=5,
                                 crt=7, mrs=100.0),
    "SQUEEZENET_CIFAR/DASH": dict(model="SQUEEZENET_CIFAR", q_method=QuantizationMethod.ScaleQuant, q_parameter=5,
                                  crt=7, mrs=100.0),
    "UNET_CIFAR/DASH": dict(model="UNET_CIFAR", q_method=QuantizationMethod.ScaleQuant, q_parameter=5, crt=7,
                            mrs=100.0),
    "ASPP_SEG_CIFAR/DASH": dict(model="ASPP_SEG_CIFAR", q_method=QuantizationMethod.ScaleQuant, q_parameter=5, crt=7,
                                mrs=100.0),
    "UNET_BILINEAR_CIFAR/DASH": dict(model="UNET_BILINEAR_CIFAR", q_method=QuantizationMethod.ScaleQuant,
                                     q_parameter=5, crt=7, mrs=100.0),
    "DEEPLAB_HEAD_CIFAR/DASH": dict(model="DEEPLAB_HEAD_CIFAR", q_method=QuantizationMethod.ScaleQuant, q_parameter=5,
                                    crt=7, mrs=100.0),
    "MODEL_A_ARGMAX/SIMPLE": dict(model="MODEL_A_ARGMAX", q_method=QuantizationMethod.SimpleQuant, q_parameter=-1, crt=8,
                                  mrs=100.0),
    "MODEL_A/SIMPLE": dict(model="MODEL_A", q_method=QuantizationMethod.SimpleQuant, q_parameter=-1, crt=8, mrs=100.0),
}
