"""Training pipeline for the model zoo (reference: models/train_pytorch.ipynb, C48).

Builds a PyTorch `nn.Sequential` from a zoo architecture, trains it (optionally
with the reference's fake quantization: x -> round(x / c) * c with a
straight-through gradient, notebook cell 7), converts the trained network to
a float `Circuit` with the requested Dash quantization and exports ONNX
through the built-in writer (the notebook used torch.onnx.export; the onnx
package is not available on the target image).

Data: `--data-dir` with the MNIST / CIFAR-10 files, otherwise a synthetic
stand-in with the same shapes (useful to exercise the pipeline offline).

    python -m dash_amd.models.train --model MODEL_A --epochs 2 --out MODEL_A.onnx
"""
from __future__ import annotations

import argparse
from typing import Optional

import numpy as np

from ..ir.circuit import Circuit
from ..ir.layers import (Bilinear, Clip, Conv2d, ConvTranspose2d, Dense, Flatten, LeakyRelu, MaxPool2d, Mul, PiecewiseLinear, Relu, Rescale, Sign, SumPool2d,
                         Upsample, _pool_out)
from ..ir.quant import QuantizationMethod
from .zoo import ARCHS, canonical


def _torch():
    import torch
    import torch.nn as nn

    return torch, nn


_SQUARE = None


def _square_module():
    """nn.Module of the zoo's ("square",) op, x -> x * x (one class per process, so to_circuit recognises it)."""
    global _SQUARE
    if _SQUARE is None:
        _, nn = _torch()

        class Square(nn.Module):
            def forward(self, x):
                return x * x

        _SQUARE = Square
    return _SQUARE


class _FakeQuant:
    """round(x / c) * c with an identity gradient (straight-through)."""

    def __init__(self, c: float):
        self.c = c

    def __call__(self, x):
        if not self.c:
            return x
        return x + (x / self.c).round().mul(self.c).sub(x).detach()


def build_torch_model(name: str, fake_quant: float = 0.0):
    torch, nn = _torch()
    arch = ARCHS[canonical(name)]
    C, H, W = arch["input"]
    dims = [C, H, W]
    mods = []
    fq = _FakeQuant(fake_quant)

    class FQLinear(nn.Linear):
        def forward(self, x):
            return nn.functional.linear(fq(x), fq(self.weight), fq(self.bias))

    class FQConvT(nn.ConvTranspose2d):
        def forward(self, x):
            return nn.functional.conv_transpose2d(fq(x), fq(self.weight), fq(self.bias), self.stride, self.padding,
                                                  self.output_padding)

    class FQConv(nn.Conv2d):  # nn.Conv2d's own `groups` and `dilation` keywords (depthwise: groups = in channels)
        def forward(self, x):
            return self._conv_forward(fq(x), fq(self.weight), fq(self.bias))

    for op in arch["ops"]:
        k = op[0]
        if k == "flatten":
            mods.append(nn.Flatten())
            dims = [int(np.prod(dims))]
        elif k == "fc":
            mods.append(FQLinear(int(np.prod(dims)), op[1]))
            dims = [op[1]]
        elif k == "conv":
            _, cout, ks, s, p = op[:5]
            d = op[5] if len(op) > 5 else 1  # optional dilation
            ke = (ks - 1) * d + 1
            mods.append(FQConv(dims[0], cout, ks, stride=s, padding=p, dilation=d))
            dims = [cout, (dims[1] + 2 * p - ke) // s + 1, (dims[2] + 2 * p - ke) // s + 1]
        elif k == "dwconv":
            _, ks, s, p = op[:4]
            d = op[4] if len(op) > 4 else 1
            ke = (ks - 1) * d + 1
            mods.append(FQConv(dims[0], dims[0], ks, stride=s, padding=p, groups=dims[0], dilation=d))
            dims = [dims[0], (dims[1] + 2 * p - ke) // s + 1, (dims[2] + 2 * p - ke) // s + 1]
        elif k == "convt":
            _, cout, ks, s, p, opad = op
            mods.append(FQConvT(dims[0], cout, ks, stride=s, padding=p, output_padding=opad))
            dims = [cout, (dims[1] - 1) * s - 2 * p + ks + opad, (dims[2] - 1) * s - 2 * p + ks + opad]
        elif k == "up":
            mods.append(nn.Upsample(scale_factor=int(op[1]), mode="nearest"))
            dims = [dims[0], dims[1] * int(op[1]), dims[2] * int(op[1])]
        elif k == "bilinear":
            mode = op[2] if len(op) > 2 else "half_pixel"
            if mode == "asymmetric":
                raise NotImplementedError("training: nn.Upsample(mode='bilinear') has no asymmetric coordinate mode")
            mods.append(nn.Upsample(scale_factor=op[1], mode="bilinear", align_corners=mode == "align_corners"))
            dims = [dims[0], int(dims[1] * op[1]), int(dims[2] * op[1])]
        elif k in ("skip", "cat"):
            raise NotImplementedError(f"training: op {k} (skip connections) not supported by the sequential trainer")
        elif k == "relu":
            mods.append(nn.ReLU())
        elif k == "leaky":
            mods.append(nn.LeakyReLU(float(op[1])))
        elif k == "prelu":
            mods.append(nn.PReLU(dims[0]))
        elif k == "square":
            mods.append(_square_module()())
        elif k == "se":
            raise NotImplementedError(f"training: op {k} (squeeze-and-excitation reads its input twice) not supported "
                                      "by the sequential trainer")
        elif k == "nonlocal":
            raise NotImplementedError(f"training: op {k} (a non-local block reads its input four times) not supported "
                                      "by the sequential trainer")
        elif k == "attention":
            raise NotImplementedError(f"training: op {k} (an attention block reads its input four times) not supported "
                                      "by the sequential trainer")
        elif k in ("shuffle", "d2s", "shuffle_unit"):
            raise NotImplementedError(f"training: op {k} (a Gather layer: channel shuffle, depth-to-space and the "
                                      "ShuffleNet unit's split have no module here) not supported by the sequential "
                                      "trainer")
        elif k == "relu6":
            mods.append(nn.ReLU6())
        elif k == "clip":
            mods.append(nn.Hardtanh(float(op[1]), float(op[2])))
        elif k == "sigmoid":
            mods.append(nn.Sigmoid())
        elif k == "hsigmoid":
            if abs(float(op[1]) - 1.0 / 6.0) > 1e-6 or float(op[2]) != 0.5:
                raise NotImplementedError("training: nn.Hardsigmoid is hard_sigmoid(alpha=1/6, beta=1/2) only")
            mods.append(nn.Hardsigmoid())
        elif k == "tanh":
            raise NotImplementedError("training: nn.Tanh stands for the sign activation here (trained as tanh, garbled "
                                      "as sign); the piecewise-linear tanh op has no module of its own")
        elif k == "sign":
            mods.append(nn.Tanh())  # trained as tanh, garbled as sign (onnx_modelloader.h Tanh -> Sign)
        elif k == "maxpool":
            pad, ceil = (op[3], bool(op[4])) if len(op) > 3 else (0, False)  # ("maxpool", k, s[, pad, ceil_mode])
            mods.append(nn.MaxPool2d(op[1], op[2], padding=pad, ceil_mode=ceil))
            dims = [dims[0], _pool_out(dims[1], op[1], op[2], pad, ceil), _pool_out(dims[2], op[1], op[2], pad, ceil)]
        elif k == "sumpool":
            mods.append(nn.AvgPool2d(op[1]))
            dims = [dims[0], dims[1] // op[1], dims[2] // op[1]]
        elif k == "argmax":
            # to_circuit maps modules to layers one to one and the loss needs the logits: no module stands for an
            # index, so the model is refused instead of silently training something else
            raise NotImplementedError(f"training: {name} ends in an argmax, which has no gradient; train the model "
                                      "without the op (MODEL_A for MODEL_A_ARGMAX) and append ArgMax to its circuit")
        else:
            raise NotImplementedError(f"training: op {k} (residual blocks, fire / aspp modules, global pooling) not supported "
                                      "by the sequential trainer")
    seq = nn.Sequential(*mods)
    seq.fq = fq  # set seq.fq.c = 0 to evaluate the float network
    return seq


def to_circuit(model, name: str, q_method=QuantizationMethod.ScaleQuant, q_parameter: int = 5,
               q_const: float = 0.02, leaky_bits: int = 4, pwl_bits: int = 8) -> Circuit:
    """Convert a trained sequential model to a Dash circuit (float weights, quantized per q_method). A LeakyReLU /
    PReLU becomes a LeakyRelu(slope_bits=leaky_bits); the next linear layer absorbs its 2^s (docs/LEAKY_RELU.md).
    An nn.Sigmoid / nn.Hardsigmoid becomes a PiecewiseLinear(slope_bits=pwl_bits) under the same scale rule
    (docs/PWL.md); an nn.Tanh stays the sign activation."""
    torch, nn = _torch()
    arch = ARCHS[canonical(name)]
    C, H, W = arch["input"]
    dims = (C, H, W)
    qm = QuantizationMethod(q_method)
    layers = []

    pend = [0]  # pending scale bits of the current tensor

    def rescale(d):  # consumes the pending bits
        if qm == QuantizationMethod.ScaleQuant:
            layers.append(Rescale(q_parameter + pend[0], d))
        elif qm == QuantizationMethod.ScaleQuantPlus:
            layers.append(Rescale([q_parameter], d))
        pend[0] = 0

    for m in model:
        if pend[0] and isinstance(m, (nn.ConvTranspose2d, nn.Hardtanh, nn.Tanh, nn.Sigmoid, nn.Hardsigmoid,
                                      _square_module())):
            raise NotImplementedError(f"training: a leaky ReLU's 2^{pend[0]} scale reaches {type(m).__name__} before a "
                                      "Linear or Conv2d could absorb it")
        if isinstance(m, (nn.LeakyReLU, nn.PReLU)):
            if qm != QuantizationMethod.ScaleQuant:
                raise ValueError("training: a leaky ReLU exists under ScaleQuant only")
            alpha = float(m.negative_slope) if isinstance(m, nn.LeakyReLU) else m.weight.detach().cpu().numpy()
            if not isinstance(alpha, float) and alpha.size == 1:
                alpha = float(alpha.reshape(-1)[0])
            layers.append(LeakyRelu(dims, alpha, leaky_bits))
            pend[0] += leaky_bits
        elif isinstance(m, (nn.Sigmoid, nn.Hardsigmoid)):
            if qm != QuantizationMethod.ScaleQuant:
                raise ValueError("training: a piecewise-linear activation exists under ScaleQuant only")
            if isinstance(m, nn.Sigmoid):
                layers.append(PiecewiseLinear.sigmoid(dims, pwl_bits, q_parameter, qm))
            else:  # relu6(x + 3) / 6
                layers.append(PiecewiseLinear.hard_sigmoid(dims, 1.0 / 6.0, 0.5, pwl_bits, q_parameter, qm))
            pend[0] += pwl_bits
        elif isinstance(m, nn.Flatten):
            layers.append(Flatten(dims))
            dims = (int(np.prod(dims)),)
        elif isinstance(m, nn.Linear):
            d = Dense(m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy(), q_parameter, qm, q_const,
                      in_scale_bits=pend[0])
            layers.append(d)
            dims = d.out_dims
            rescale(dims)
        elif isinstance(m, nn.Conv2d):
            w = m.weight.detach().cpu().numpy()
            F, Cg, kh, kw = w.shape  # [F][C/groups][kh][kw]
            c = Conv2d(w, m.bias.detach().cpu().numpy(), dims[2], dims[1], Cg * m.groups, F, kw, kh, m.stride[1],
                       m.stride[0], q_parameter, qm, q_const, pad_width=m.padding[1], pad_height=m.padding[0],
                       groups=m.groups, dilation_width=m.dilation[1], dilation_height=m.dilation[0],
                       in_scale_bits=pend[0])
            layers.append(c)
            dims = c.out_dims
            rescale(dims)
        elif isinstance(m, nn.ConvTranspose2d):
            w = m.weight.detach().cpu().numpy()  # [C][F/groups][kh][kw]
            Cin, Fo, kh, kw = w.shape
            c = ConvTranspose2d(w, m.bias.detach().cpu().numpy(), dims[2], dims[1], Cin, Fo, kw, kh, m.stride[1],
                                m.stride[0], q_parameter, qm, q_const, pad_width=m.padding[1],
                                pad_height=m.padding[0], out_pad_width=m.output_padding[1],
                                out_pad_height=m.output_padding[0], groups=m.groups, dilation=max(m.dilation))
            layers.append(c)
            dims = c.out_dims
            rescale(dims)
        elif isinstance(m, nn.Upsample):
            if m.mode not in ("nearest", "bilinear") or m.scale_factor is None:
                raise NotImplementedError("training: only nn.Upsample(scale_factor=f, mode='nearest' | 'bilinear') maps "
                                          "to a layer")
            sf = m.scale_factor if isinstance(m.scale_factor, (tuple, list)) else (m.scale_factor, m.scale_factor)
            if m.mode == "bilinear":  # docs/BILINEAR.md: half_pixel is PyTorch's align_corners=False
                if qm != QuantizationMethod.ScaleQuant:
                    raise ValueError("training: a bilinear upsampling exists under ScaleQuant only")
                bl = Bilinear(dims, (sf[0], sf[1]), mode="align_corners" if m.align_corners else "half_pixel")
                layers.append(bl)
                dims = bl.out_dims
                pend[0] += bl.scale_bits
                continue
            if any(float(f) != int(f) for f in sf):
                raise NotImplementedError("training: nn.Upsample needs integer scale factors")
            up = Upsample(dims, int(sf[0]), int(sf[1]))
            layers.append(up)
            dims = up.out_dims
        elif isinstance(m, nn.ReLU):
            layers.append(Relu(dims))
        elif isinstance(m, _square_module()):
            layers.append(Mul.square(dims))
            rescale(dims)
        elif isinstance(m, nn.Hardtanh):  # nn.ReLU6 is a Hardtanh(0, 6)
            layers.append(Clip(dims, float(m.min_val), float(m.max_val), q_parameter, qm))
        elif isinstance(m, nn.Tanh):
            layers.append(Sign(dims))
        elif isinstance(m, nn.MaxPool2d):
            k, s, pad = int(m.kernel_size), int(m.stride), int(m.padding)
            mp = MaxPool2d(dims[2], dims[1], dims[0], k, k, s, s, pad_width=pad, pad_height=pad,
                           ceil_mode=bool(m.ceil_mode))
            layers.append(mp)
            dims = mp.out_dims
        elif isinstance(m, nn.AvgPool2d):
            k = int(m.kernel_size)
            sp = SumPool2d(dims[2], dims[1], dims[0], k, k)
            layers.append(sp)
            dims = sp.out_dims
        elif isinstance(m, nn.Dropout):
            continue
    return Circuit(layers, q_parameter)


def train(name: str, epochs: int = 1, data_dir: Optional[str] = None, fake_quant: float = 0.0, lr: float = 1e-3,
          batch_size: int = 128, n_synthetic: int = 2048, seed: int = 0, device: Optional[str] = None,
          log=print):
    torch, nn = _torch()
    torch.manual_seed(seed)
    arch = ARCHS[canonical(name)]
    shape = arch["input"]
    if data_dir:
        from .. import data

        ds = data.load("mnist" if shape[0] == 1 else "cifar10", data_dir)
        xtr, ytr = ds.train_images, ds.train_labels
        xte, yte = ds.test_images, ds.test_labels
    else:
        rng = np.random.default_rng(seed)
        # synthetic, learnable: the label is the argmax of a fixed random projection
        proj = rng.standard_normal((int(np.prod(shape)), 10)).astype(np.float32)
        xtr = rng.standard_normal((n_synthetic, *shape)).astype(np.float32)
        ytr = np.argmax(xtr.reshape(len(xtr), -1) @ proj, axis=1)
        xte = rng.standard_normal((n_synthetic // 4, *shape)).astype(np.float32)
        yte = np.argmax(xte.reshape(len(xte), -1) @ proj, axis=1)
    dev = torch.device(device or ("cuda" if torch.cuda.is_available() else "cpu"))
    model = build_torch_model(name, fake_quant).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    lossf = nn.CrossEntropyLoss()
    Xtr, Ytr = torch.from_numpy(np.asarray(xtr)), torch.from_numpy(np.asarray(ytr, np.int64))
    for ep in range(epochs):
        model.train()
        perm = torch.randperm(len(Xtr))
        tot = 0.0
        for s in range(0, len(Xtr), batch_size):
            idx = perm[s:s + batch_size]
            xb, yb = Xtr[idx].to(dev), Ytr[idx].to(dev)
            opt.zero_grad()
            loss = lossf(model(xb), yb)
            loss.backward()
            opt.step()
            tot += float(loss.detach()) * len(idx)
        acc = evaluate(model, xte, yte, dev)
        log(f"epoch {ep + 1}/{epochs}: loss {tot / len(Xtr):.4f}  test acc {acc:.4f}")
    return model.cpu(), (xte, yte)


def evaluate(model, x, y, dev=None) -> float:
    torch, _ = _torch()
    model.eval()
    with torch.no_grad():
        xt = torch.from_numpy(np.asarray(x))
        if dev is not None:
            xt = xt.to(dev)
        pred = model(xt).argmax(1).cpu().numpy()
    return float(np.mean(pred == np.asarray(y)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="MODEL_A")
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--data-dir", default=None)
    ap.add_argument("--fake-quant", type=float, default=0.0)
    ap.add_argument("--out", default=None, help="ONNX output path")
    args = ap.parse_args()
    model, _ = train(args.model, args.epochs, args.data_dir, args.fake_quant)
    if args.out:
        from ..ir.onnx import save_onnx_model

        save_onnx_model(args.out, to_circuit(model, args.model, QuantizationMethod.SimpleQuant, -1),
                        producer="pytorch")
        print("wrote", args.out)


if __name__ == "__main__":
    main()
