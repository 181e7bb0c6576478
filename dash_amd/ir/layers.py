"""Plaintext layer IR (float + quantized semantics, range tracking).

Reference: circuit/layer/*.h (C08-C11 in SURVEY §2.1). Tensors are numpy
arrays; images are laid out [C][H][W] (width fastest), which is the memory
order of the reference's dim_t {W, H, C} (dims[0] fastest).

Every layer knows how to describe itself to the native garbler
(`garble_spec`), which keeps the kind numbering of csrc/model.h.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import numpy as np

from .quant import QuantizationMethod, ceil_div, quantize_params, quantize_scale

Q_MAX = np.iinfo(np.int64).max
Q_MIN = np.iinfo(np.int64).min


class Kind:
    DENSE = 0
    CONV = 1
    RELU = 2
    SIGN = 3
    RESCALE = 4
    MAXPOOL = 5
    FLATTEN = 6
    PROJ = 7
    MULT = 8
    MMULT = 9
    MAX = 10
    BASEEXT = 11
    ADD = 12
    SUMPOOL = 13
    CONCAT = 14
    CLIP = 15
    ARGMAX = 16
    CONVT = 17
    UPSAMPLE = 18
    MUL = 19
    LEAKY = 20
    PWL = 21
    MATMUL = 22
    GATHER = 23
    BILINEAR = 24


def _size(d: Sequence[int]) -> int:
    s = 1
    for v in d:
        s *= int(v)
    return s


class Layer:
    kind: int = -1
    name: str = "layer"

    # index of the layer whose output this layer reads (-1 = circuit input);
    # None = the previous layer (sequential). Used for projection shortcuts.
    in_src = None

    def __init__(self, in_dims: Sequence[int], out_dims: Sequence[int]):
        self.in_dims = tuple(int(d) for d in in_dims)
        self.out_dims = tuple(int(d) for d in out_dims)
        self.reset_ranges()

    # ---- geometry
    @property
    def in_size(self) -> int:
        return _size(self.in_dims)

    @property
    def out_size(self) -> int:
        return _size(self.out_dims)

    # ---- range tracking (reference layer.h:13-77)
    def reset_ranges(self):
        self.min_q = Q_MAX
        self.max_q = Q_MIN
        self.min_f = np.inf
        self.max_f = -np.inf

    def _track_q(self, *arrs):
        for a in arrs:
            a = np.asarray(a)
            if a.size:
                self.min_q = min(self.min_q, int(a.min()))
                self.max_q = max(self.max_q, int(a.max()))

    def _track_f(self, *arrs):
        for a in arrs:
            a = np.asarray(a)
            if a.size:
                self.min_f = min(self.min_f, float(a.min()))
                self.max_f = max(self.max_f, float(a.max()))

    def get_min_plain_q_val(self) -> int:
        return self.min_q

    def get_max_plain_q_val(self) -> int:
        return self.max_q

    # ---- semantics
    def plain_eval(self, x: np.ndarray, track: bool = True, ctx=None) -> np.ndarray:
        raise NotImplementedError

    def plain_q_eval(self, x: np.ndarray, track: bool = True, ctx=None, crt_modulus: Optional[int] = None) -> np.ndarray:
        raise NotImplementedError

    def quantize(self, q_const: float) -> None:  # SimpleQuant re-quantization
        pass

    def get_q_const(self) -> float:
        return 0.0

    def garble_spec(self) -> tuple[int, dict]:
        return self.kind, {}

    def __repr__(self) -> str:
        return f"{type(self).__name__}(in={self.in_dims}, out={self.out_dims})"


# ---------------------------------------------------------------------------
class Dense(Layer):
    """Fully connected layer, W [out][in]. Reference: circuit/layer/dense.h."""

    kind = Kind.DENSE
    name = "dense"

    def __init__(self, weights: np.ndarray, biases: np.ndarray, q_parameter: int = -1,
                 q_method: QuantizationMethod = QuantizationMethod.SimpleQuant, q_const: float = 10.0,
                 channel_tf: int = 0, in_scale_bits: int = 0):
        w = np.asarray(weights, dtype=np.float32)
        b = np.asarray(biases, dtype=np.float32).reshape(-1)
        assert w.ndim == 2 and w.shape[0] == b.shape[0], "weights/biases shape mismatch"
        super().__init__((w.shape[1],), (w.shape[0],))
        self.weights, self.biases = w, b
        self.q_method, self.q_parameter, self.q_const = QuantizationMethod(q_method), q_parameter, q_const
        self.channel_tf = int(channel_tf)
        self.in_scale_bits = int(in_scale_bits)
        self.q_weights, self.q_biases = quantize_params(w, b, self.q_method, q_parameter, q_const, self.in_scale_bits)
        self._track_q(self.q_weights, self.q_biases)

    @classmethod
    def from_quantized(cls, q_weights: np.ndarray, q_biases: np.ndarray, channel_tf: int = 0) -> "Dense":
        d = cls(np.asarray(q_weights, dtype=np.float32), np.asarray(q_biases, dtype=np.float32), q_const=1.0,
                channel_tf=channel_tf)
        d.q_weights = np.asarray(q_weights, dtype=np.int64)
        d.q_biases = np.asarray(q_biases, dtype=np.int64).reshape(-1)
        d.reset_ranges()
        d._track_q(d.q_weights, d.q_biases)
        return d

    def _src(self, x):
        if self.channel_tf == 0:
            return x
        K, ch = x.shape[0], self.channel_tf
        i = np.arange(K)
        return x[i // ch + (i % ch) * (K // ch)]

    def quantize(self, q_const):
        self.q_const = q_const
        self.q_weights, self.q_biases = quantize_params(self.weights, self.biases, QuantizationMethod.SimpleQuant,
                                                        -1, q_const)
        self.reset_ranges()

    def get_q_const(self):
        return self.q_const

    def plain_eval(self, x, track=True, ctx=None):
        x = self._src(np.asarray(x, dtype=np.float32).reshape(-1))
        y = self.weights @ x + self.biases
        if track:
            self._track_f(x, y, self.weights, self.biases)
        return y

    def plain_q_eval(self, x, track=True, ctx=None, crt_modulus=None):
        x = self._src(np.asarray(x, dtype=np.int64).reshape(-1))
        if track:
            self._track_q(x)
            # partial sums of every row, as the reference tracks them
            cs = np.cumsum(self.q_weights * x[None, :], axis=1)
            self._track_q(cs)
        y = self.q_weights @ x + self.q_biases
        if track:
            self._track_q(y)
        return y

    def get_min_plain_q_val(self):
        return min(self.min_q, int(self.q_weights.min()), int(self.q_biases.min()))

    def get_max_plain_q_val(self):
        return max(self.max_q, int(self.q_weights.max()), int(self.q_biases.max()))

    def garble_spec(self):
        return self.kind, {"in": self.in_size, "out": self.out_size, "w": self.q_weights.reshape(-1),
                           "b": self.q_biases.reshape(-1), "channel_tf": self.channel_tf}


def _im2col(x: np.ndarray, C, H, W, kh, kw, sh, sw, ph, pw, dh=1, dw=1):
    """Patch matrix [C*kh*kw][OH*OW]; tap (dy, dx) reads the padded image at (oy*sh + dy*dh, ox*sw + dx*dw)."""
    xp = np.pad(x.reshape(C, H, W), ((0, 0), (ph, ph), (pw, pw)))
    OH = (H + 2 * ph - (kh - 1) * dh - 1) // sh + 1
    OW = (W + 2 * pw - (kw - 1) * dw - 1) // sw + 1
    cols = np.empty((C, kh, kw, OH, OW), dtype=x.dtype)
    for dy in range(kh):
        for dx in range(kw):
            y0, x0 = dy * dh, dx * dw
            cols[:, dy, dx] = xp[:, y0:y0 + sh * (OH - 1) + 1:sh, x0:x0 + sw * (OW - 1) + 1:sw]
    return cols.reshape(C * kh * kw, OH * OW), OH, OW


class Conv2d(Layer):
    """2-D convolution, weights [F][C/groups][kh][kw]; optional zero padding
    and channel groups (extensions over the reference's 'valid'-only dense
    conv, needed by VGG/ResNet and by depthwise-separable networks). Group q
    holds filters [q*F/g, (q+1)*F/g) and reads channels [q*C/g, (q+1)*C/g).
    Dilation (atrous convolution, docs/DILATED_CONV.md): with the effective
    kernel keh = (kh-1)*dh + 1, OH = (H + 2*ph - keh)//sh + 1 and tap (dy, dx)
    of output (oy, ox) reads x[c][oy*sh - ph + dy*dh][ox*sw - pw + dx*dw]; a
    kernel axis of size 1 makes its dilation moot and stores it as 1.
    Reference: circuit/layer/conv2d.h (index bug §2.7 #2 fixed)."""

    kind = Kind.CONV
    name = "conv2d"

    def __init__(self, weights: np.ndarray, biases: np.ndarray, input_width: int, input_height: int, channel: int,
                 filter: int, filter_width: int, filter_height: int, stride_width: int = 1, stride_height: int = 1,
                 q_parameter: int = -1, q_method: QuantizationMethod = QuantizationMethod.SimpleQuant,
                 q_const: float = 10.0, pad_width: int = 0, pad_height: int = 0, groups: int = 1,
                 dilation_width: int = 1, dilation_height: int = 1, in_scale_bits: int = 0):
        self.C, self.H, self.W, self.F = int(channel), int(input_height), int(input_width), int(filter)
        self.groups = int(groups)
        self.in_scale_bits = int(in_scale_bits)
        if self.groups < 1 or self.C % self.groups or self.F % self.groups:
            raise ValueError(f"groups={groups} must be positive and divide channel={channel} and filter={filter}")
        self.Cg, self.Fg = self.C // self.groups, self.F // self.groups
        self.kh, self.kw, self.sh, self.sw = int(filter_height), int(filter_width), int(stride_height), int(stride_width)
        self.ph, self.pw = int(pad_height), int(pad_width)
        self.dh, self.dw = int(dilation_height), int(dilation_width)
        if self.dh < 1 or self.dw < 1 or self.dh != dilation_height or self.dw != dilation_width:
            raise ValueError(f"conv2d: dilation must be an integer >= 1, got ({dilation_height}, {dilation_width})")
        # a kernel axis of size 1 has no second tap to dilate: the layer is the plain conv and is stored as one
        if self.kh == 1:
            self.dh = 1
        if self.kw == 1:
            self.dw = 1
        keh, kew = (self.kh - 1) * self.dh + 1, (self.kw - 1) * self.dw + 1
        if self.H + 2 * self.ph < keh or self.W + 2 * self.pw < kew:
            raise ValueError(f"conv2d: empty output: the effective kernel ({keh} x {kew}) exceeds the padded input "
                             f"({self.H + 2 * self.ph} x {self.W + 2 * self.pw})")
        self.OH = (self.H + 2 * self.ph - keh) // self.sh + 1
        self.OW = (self.W + 2 * self.pw - kew) // self.sw + 1
        super().__init__((self.C, self.H, self.W), (self.F, self.OH, self.OW))
        w = np.asarray(weights, dtype=np.float32).reshape(self.F, self.Cg, self.kh, self.kw)
        b = np.asarray(biases, dtype=np.float32).reshape(self.F)
        self.weights, self.biases = w, b
        self.q_method, self.q_parameter, self.q_const = QuantizationMethod(q_method), q_parameter, q_const
        self.q_weights, self.q_biases = quantize_params(w, b, self.q_method, q_parameter, q_const,
                                                        self.in_scale_bits)
        self._track_q(self.q_weights, self.q_biases)

    @classmethod
    def from_quantized(cls, q_weights, q_biases, input_width, input_height, channel, filter, filter_width,
                       filter_height, stride_width=1, stride_height=1, pad_width=0, pad_height=0, groups=1,
                       dilation_width=1, dilation_height=1):
        if groups < 1 or channel % groups or filter % groups:
            raise ValueError(f"groups={groups} must be positive and divide channel={channel} and filter={filter}")
        c = cls(np.zeros((filter, channel // groups, filter_height, filter_width), np.float32),
                np.zeros(filter, np.float32),
                input_width, input_height, channel, filter, filter_width, filter_height, stride_width, stride_height,
                q_const=1.0, pad_width=pad_width, pad_height=pad_height, groups=groups,
                dilation_width=dilation_width, dilation_height=dilation_height)
        c.q_weights = np.asarray(q_weights, dtype=np.int64).reshape(filter, channel // groups, filter_height,
                                                                    filter_width)
        c.q_biases = np.asarray(q_biases, dtype=np.int64).reshape(filter)
        c.weights = c.q_weights.astype(np.float32)
        c.biases = c.q_biases.astype(np.float32)
        c.reset_ranges()
        c._track_q(c.q_weights, c.q_biases)
        return c

    def quantize(self, q_const):
        self.q_const = q_const
        self.q_weights, self.q_biases = quantize_params(self.weights, self.biases, QuantizationMethod.SimpleQuant,
                                                        -1, q_const)
        self.reset_ranges()

    def get_q_const(self):
        return self.q_const

    def _conv(self, x, w, b):
        cols, OH, OW = _im2col(x, self.C, self.H, self.W, self.kh, self.kw, self.sh, self.sw, self.ph, self.pw,
                               self.dh, self.dw)
        if self.groups == 1:
            y = w.reshape(self.F, -1) @ cols + b[:, None]
            return y.reshape(-1), cols
        # per group: the group's filters against the group's own rows of cols
        wg = w.reshape(self.groups, self.Fg, -1)
        cg = cols.reshape(self.groups, self.Cg * self.kh * self.kw, -1)
        y = np.matmul(wg, cg).reshape(self.F, -1) + b[:, None]
        return y.reshape(-1), cols

    def plain_eval(self, x, track=True, ctx=None):
        y, _ = self._conv(np.asarray(x, dtype=np.float32).reshape(-1), self.weights, self.biases)
        if track:
            self._track_f(x, y, self.weights, self.biases)
        return y

    def plain_q_eval(self, x, track=True, ctx=None, crt_modulus=None):
        x = np.asarray(x, dtype=np.int64).reshape(-1)
        y, cols = self._conv(x, self.q_weights, self.q_biases)
        if track:
            wf = self.q_weights.reshape(self.F, -1)
            # products and running partial sums (conv2d.h:85-140), over the
            # filter's own group of C/g*kh*kw terms
            Kg = self.Cg * self.kh * self.kw
            for f in range(self.F):
                q = f // self.Fg
                prod = wf[f][:, None] * cols[q * Kg:(q + 1) * Kg]
                self._track_q(prod, np.cumsum(prod, axis=0))
            self._track_q(y)
        return y

    def get_min_plain_q_val(self):
        return min(self.min_q, int(self.q_weights.min()), int(self.q_biases.min()))

    def get_max_plain_q_val(self):
        return max(self.max_q, int(self.q_weights.max()), int(self.q_biases.max()))

    def garble_spec(self):
        spec = {"C": self.C, "H": self.H, "W": self.W, "F": self.F, "kh": self.kh, "kw": self.kw,
                "sh": self.sh, "sw": self.sw, "ph": self.ph, "pw": self.pw,
                "w": self.q_weights.reshape(-1), "b": self.q_biases.reshape(-1)}
        if self.groups > 1:  # groups == 1 keeps the dense wire bytes
            spec["g"] = self.groups
        # written only when > 1: an undilated layer keeps its wire bytes
        if self.dh > 1:
            spec["dh"] = self.dh
        if self.dw > 1:
            spec["dw"] = self.dw
        return self.kind, spec


def _convt_check(kh, kw, sh, sw, ph, pw, oph, opw, groups=1, dilation=1):
    """The one domain of ConvTranspose2d (every engine shares it): groups = 1, no dilation, and per axis
    0 <= p <= k - 1, 0 <= op < s and op <= s * ceil(k / s) - k + p (no output row that no tap reaches)."""
    if int(groups) != 1:
        raise ValueError(f"conv_transpose2d: groups={groups} is not supported (groups = 1 only)")
    if int(dilation) != 1:
        raise ValueError(f"conv_transpose2d: dilation={dilation} is not supported")
    for ax, k, s, p, op in (("height", kh, sh, ph, oph), ("width", kw, sw, pw, opw)):
        if k < 1 or s < 1:
            raise ValueError(f"conv_transpose2d: kernel and stride must be positive ({ax}: k={k}, s={s})")
        if not 0 <= p <= k - 1:
            raise ValueError(f"conv_transpose2d: {ax} padding {p} outside [0, k - 1] = [0, {k - 1}]")
        if not 0 <= op < s:
            raise ValueError(f"conv_transpose2d: {ax} output padding {op} outside [0, stride) = [0, {s})")
        if op > s * ceil_div(k, s) - k + p:
            raise ValueError(f"conv_transpose2d: {ax} output padding {op} leaves output positions that no tap "
                             f"reaches (k={k}, s={s}, p={p}: at most {s * ceil_div(k, s) - k + p})")


class ConvTranspose2d(Layer):
    """Transposed 2-D convolution with PyTorch / ONNX semantics: input (C, H, W), weights [C][F][kh][kw], strides
    (sh, sw), symmetric pads (ph, pw), output padding (oph, opw), OH = (H-1) sh - 2 ph + kh + oph and
      y[f][oy][ox] = b[f] + sum w[c][f][dy][dx] x[c][iy][ix]
    over the taps with oy + ph - dy = sh iy, 0 <= iy < H (likewise in x). groups = 1, no dilation; the domain is
    _convt_check's. Linear, so free of garbled tables; hardened encoding only (docs/CONV_TRANSPOSE.md)."""

    kind = Kind.CONVT
    name = "conv_transpose2d"

    def __init__(self, weights: np.ndarray, biases: np.ndarray, input_width: int, input_height: int, channel: int,
                 filter: int, filter_width: int, filter_height: int, stride_width: int = 1, stride_height: int = 1,
                 q_parameter: int = -1, q_method: QuantizationMethod = QuantizationMethod.SimpleQuant,
                 q_const: float = 10.0, pad_width: int = 0, pad_height: int = 0, out_pad_width: int = 0,
                 out_pad_height: int = 0, groups: int = 1, dilation: int = 1, in_scale_bits: int = 0):
        self.C, self.H, self.W, self.F = int(channel), int(input_height), int(input_width), int(filter)
        self.in_scale_bits = int(in_scale_bits)
        self.kh, self.kw, self.sh, self.sw = int(filter_height), int(filter_width), int(stride_height), int(stride_width)
        self.ph, self.pw, self.oph, self.opw = int(pad_height), int(pad_width), int(out_pad_height), int(out_pad_width)
        _convt_check(self.kh, self.kw, self.sh, self.sw, self.ph, self.pw, self.oph, self.opw, groups, dilation)
        self.OH = (self.H - 1) * self.sh - 2 * self.ph + self.kh + self.oph
        self.OW = (self.W - 1) * self.sw - 2 * self.pw + self.kw + self.opw
        if self.OH < 1 or self.OW < 1:
            raise ValueError(f"conv_transpose2d: empty output ({self.OH} x {self.OW})")
        super().__init__((self.C, self.H, self.W), (self.F, self.OH, self.OW))
        w = np.asarray(weights, dtype=np.float32).reshape(self.C, self.F, self.kh, self.kw)
        b = np.asarray(biases, dtype=np.float32).reshape(self.F)
        self.weights, self.biases = w, b
        self.q_method, self.q_parameter, self.q_const = QuantizationMethod(q_method), q_parameter, q_const
        self.q_weights, self.q_biases = quantize_params(w, b, self.q_method, q_parameter, q_const,
                                                        self.in_scale_bits)
        self._track_q(self.q_weights, self.q_biases)

    @classmethod
    def from_quantized(cls, q_weights, q_biases, input_width, input_height, channel, filter, filter_width,
                       filter_height, stride_width=1, stride_height=1, pad_width=0, pad_height=0, out_pad_width=0,
                       out_pad_height=0, groups=1, dilation=1):
        c = cls(np.zeros((channel, filter, filter_height, filter_width), np.float32), np.zeros(filter, np.float32),
                input_width, input_height, channel, filter, filter_width, filter_height, stride_width, stride_height,
                q_const=1.0, pad_width=pad_width, pad_height=pad_height, out_pad_width=out_pad_width,
                out_pad_height=out_pad_height, groups=groups, dilation=dilation)
        c.q_weights = np.asarray(q_weights, dtype=np.int64).reshape(channel, filter, filter_height, filter_width)
        c.q_biases = np.asarray(q_biases, dtype=np.int64).reshape(filter)
        c.weights = c.q_weights.astype(np.float32)
        c.biases = c.q_biases.astype(np.float32)
        c.reset_ranges()
        c._track_q(c.q_weights, c.q_biases)
        return c

    def quantize(self, q_const):
        self.q_const = q_const
        self.q_weights, self.q_biases = quantize_params(self.weights, self.biases, QuantizationMethod.SimpleQuant,
                                                        -1, q_const)
        self.reset_ranges()

    def get_q_const(self):
        return self.q_const

    def _taps(self):
        """Per tap (dy, dx): the output rows / columns it reaches and the input rows / columns they read."""
        for dy in range(self.kh):
            oy = np.arange(self.H) * self.sh + dy - self.ph
            my = (oy >= 0) & (oy < self.OH)
            for dx in range(self.kw):
                ox = np.arange(self.W) * self.sw + dx - self.pw
                mx = (ox >= 0) & (ox < self.OW)
                if my.any() and mx.any():
                    yield dy, dx, oy[my], np.nonzero(my)[0], ox[mx], np.nonzero(mx)[0]

    def _convt(self, x, w, b):
        x = x.reshape(self.C, self.H, self.W)
        y = np.zeros((self.F, self.OH, self.OW), dtype=np.result_type(x.dtype, w.dtype))
        for dy, dx, oy, iy, ox, ix in self._taps():
            y[:, oy[:, None], ox[None, :]] += np.einsum("cf,cyx->fyx", w[:, :, dy, dx], x[:, iy[:, None], ix[None, :]])
        return (y + b[:, None, None]).reshape(-1)

    def plain_eval(self, x, track=True, ctx=None):
        y = self._convt(np.asarray(x, dtype=np.float32).reshape(-1), self.weights, self.biases)
        if track:
            self._track_f(x, y, self.weights, self.biases)
        return y

    def plain_q_eval(self, x, track=True, ctx=None, crt_modulus=None):
        x = np.asarray(x, dtype=np.int64).reshape(-1)
        y = self._convt(x, self.q_weights, self.q_biases)
        if track:
            # products and running partial sums over each output's valid taps, in (c, dy, dx) order (as Conv2d):
            # terms[c, dy, dx, f, oy, ox], zero where the tap does not reach the output
            xi = x.reshape(self.C, self.H, self.W)
            terms = np.zeros((self.C, self.kh, self.kw, self.F, self.OH, self.OW), dtype=np.int64)
            for dy, dx, oy, iy, ox, ix in self._taps():
                terms[:, dy, dx][:, :, oy[:, None], ox[None, :]] = (
                    self.q_weights[:, :, dy, dx][:, :, None, None] * xi[:, None][:, :, iy[:, None], ix[None, :]])
            terms = terms.reshape(self.C * self.kh * self.kw, -1)
            self._track_q(terms, np.cumsum(terms, axis=0), y)
        return y

    def get_min_plain_q_val(self):
        return min(self.min_q, int(self.q_weights.min()), int(self.q_biases.min()))

    def get_max_plain_q_val(self):
        return max(self.max_q, int(self.q_weights.max()), int(self.q_biases.max()))

    def garble_spec(self):
        return self.kind, {"C": self.C, "H": self.H, "W": self.W, "F": self.F, "kh": self.kh, "kw": self.kw,
                           "sh": self.sh, "sw": self.sw, "ph": self.ph, "pw": self.pw, "oph": self.oph,
                           "opw": self.opw, "w": self.q_weights.reshape(-1), "b": self.q_biases.reshape(-1)}


class Upsample(Layer):
    """Nearest-neighbour upsampling of a (C, H, W) tensor by integer factors (fh, fw) >= 1, not both 1:
    y[c][oy][ox] = x[c][oy // fh][ox // fw]. Free in the label domain, like Concat: no tables, no PRG draws, no
    constants, so it works under both encodings and every quantization scheme."""

    kind = Kind.UPSAMPLE
    name = "upsample"

    def __init__(self, dims, factor_height: int, factor_width: Optional[int] = None):
        dims = tuple(int(d) for d in dims)
        if len(dims) != 3:
            raise ValueError(f"upsample: the input is (C, H, W), got {dims}")
        self.C, self.H, self.W = dims
        self.fh = int(factor_height)
        self.fw = int(factor_height if factor_width is None else factor_width)
        if self.fh != factor_height or self.fw != (factor_height if factor_width is None else factor_width):
            raise ValueError("upsample: integer factors only")
        if self.fh < 1 or self.fw < 1 or self.fh * self.fw == 1:
            raise ValueError(f"upsample: factors must be >= 1 and not both 1, got ({self.fh}, {self.fw})")
        super().__init__(dims, (self.C, self.H * self.fh, self.W * self.fw))

    def _up(self, x):
        x = np.asarray(x).reshape(self.C, self.H, self.W)
        return np.repeat(np.repeat(x, self.fh, axis=1), self.fw, axis=2).reshape(-1)

    def plain_eval(self, x, track=True, ctx=None):
        return self._up(x)

    def plain_q_eval(self, x, track=True, ctx=None, crt_modulus=None):
        y = self._up(np.asarray(x, dtype=np.int64))
        if track:
            self._track_q(y)
        return y

    def garble_spec(self):
        return self.kind, {"C": self.C, "H": self.H, "W": self.W, "fh": self.fh, "fw": self.fw}

    def __repr__(self) -> str:
        return f"Upsample(in={self.in_dims}, factors=({self.fh}, {self.fw}))"


def _slice_bounds(d: int, start: int, stop: int) -> tuple:
    """ONNX Slice with a positive step on an axis of d elements: a negative start / stop counts from the end, then
    both are clamped to [0, d] (so INT64_MAX means "to the end")."""
    return tuple(min(max(int(v) + d if int(v) < 0 else int(v), 0), d) for v in (start, stop))


class Gather(Layer):
    """General reordering of a tensor by a public index map on the flat [C][H][W] order:
    out.flat[o] = x.flat[idx[o]]. Repeats are allowed (fan-out, as Upsample has) and elements may go unread. Free in
    the label domain: no tables, no PRG draws, no constants, so it works under both encodings and every
    quantization scheme. The constructors below build the maps of Transpose, Slice, channel shuffle,
    DepthToSpace and SpaceToDepth."""

    kind = Kind.GATHER
    name = "gather"

    def __init__(self, dims, idx, out_dims=None):
        dims = tuple(int(d) for d in dims)
        nin = _size(dims)
        a = np.asarray(idx)
        if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
            raise ValueError(f"gather: idx is a 1-D integer array, got shape {a.shape} of {a.dtype}")
        if a.size == 0:
            raise ValueError("gather: idx is empty")
        if not 0 < nin < 2 ** 31 or a.size >= 2 ** 31:
            raise ValueError(f"gather: sizes must lie in [1, 2^31), got Nin={nin}, Nout={a.size}")
        a = a.astype(np.int64)
        bad = np.nonzero((a < 0) | (a >= nin))[0]
        if bad.size:
            o = int(bad[0])
            what = "is negative (reserved)" if a[o] < 0 else f"is not below the input size {nin}"
            raise ValueError(f"gather: idx[{o}] = {int(a[o])} {what}")
        od = (int(a.size),) if out_dims is None else tuple(int(d) for d in out_dims)
        if _size(od) != a.size or any(d < 1 for d in od):
            raise ValueError(f"gather: out_dims {od} do not hold the {a.size} elements of idx")
        super().__init__(dims, od)
        a.setflags(write=False)  # garble_spec hands the array itself to the native specs (Circuit.garble_specs_native)
        self.idx = a

    # ---- the maps, written with numpy on np.arange(Nin).reshape(dims)
    @staticmethod
    def _ids(dims):
        dims = tuple(int(d) for d in dims)
        return np.arange(_size(dims), dtype=np.int64).reshape(dims)

    @classmethod
    def _of(cls, dims, ids):
        return cls(dims, ids.reshape(-1), ids.shape)

    @classmethod
    def transpose(cls, dims, perm):
        perm = tuple(int(p) for p in perm)
        if sorted(perm) != list(range(len(tuple(dims)))):
            raise ValueError(f"gather.transpose: perm {perm} is no permutation of the axes of {tuple(dims)}")
        return cls._of(dims, np.transpose(cls._ids(dims), perm))

    @classmethod
    def slice(cls, dims, axis, start, stop, step=1):
        """ONNX Slice along one axis: negative start / stop count from the end, both are clamped to [0, d]."""
        dims = tuple(int(d) for d in dims)
        axis, step = int(axis), int(step)
        if not -len(dims) <= axis < len(dims):
            raise ValueError(f"gather.slice: axis {axis} outside the {len(dims)} axes")
        if step < 1:
            raise ValueError(f"gather.slice: step must be >= 1, got {step}")
        axis %= len(dims)
        d = dims[axis]
        lo, hi = _slice_bounds(d, start, stop)
        if hi <= lo:
            raise ValueError(f"gather.slice: empty slice [{start}:{stop}:{step}] of an axis of {d}")
        sl = [np.s_[:]] * len(dims)
        sl[axis] = np.s_[lo:hi:step]
        return cls._of(dims, cls._ids(dims)[tuple(sl)])

    @classmethod
    def channel_shuffle(cls, dims, groups):
        dims = tuple(int(d) for d in dims)
        g = int(groups)
        if g < 1 or dims[0] % g:
            raise ValueError(f"gather.channel_shuffle: {g} groups do not divide {dims[0]} channels")
        ids = cls._ids(dims).reshape((g, dims[0] // g) + dims[1:])
        return cls(dims, np.swapaxes(ids, 0, 1).reshape(-1), dims)

    @classmethod
    def depth_to_space(cls, dims, r, mode="DCR"):
        dims = tuple(int(d) for d in dims)
        r = int(r)
        if len(dims) != 3 or r < 1 or dims[0] % (r * r):
            raise ValueError(f"gather.depth_to_space: (C, H, W) with C a multiple of r^2, got {dims}, r={r}")
        C, H, W = dims
        c = C // (r * r)
        if mode == "DCR":
            ids = cls._ids(dims).reshape(r, r, c, H, W).transpose(2, 3, 0, 4, 1)
        elif mode == "CRD":
            ids = cls._ids(dims).reshape(c, r, r, H, W).transpose(0, 3, 1, 4, 2)
        else:
            raise ValueError(f"gather.depth_to_space: mode is 'DCR' or 'CRD', got {mode!r}")
        return cls(dims, ids.reshape(-1), (c, H * r, W * r))

    @classmethod
    def space_to_depth(cls, dims, r):
        dims = tuple(int(d) for d in dims)
        r = int(r)
        if len(dims) != 3 or r < 1 or dims[1] % r or dims[2] % r:
            raise ValueError(f"gather.space_to_depth: (C, H, W) with H and W multiples of r, got {dims}, r={r}")
        C, H, W = dims
        ids = cls._ids(dims).reshape(C, H // r, r, W // r, r).transpose(2, 4, 0, 1, 3)
        return cls(dims, ids.reshape(-1), (C * r * r, H // r, W // r))

    def plain_eval(self, x, track=True, ctx=None):
        return np.asarray(x, dtype=np.float32).reshape(-1)[self.idx]

    def plain_q_eval(self, x, track=True, ctx=None, crt_modulus=None):
        y = np.asarray(x, dtype=np.int64).reshape(-1)[self.idx]
        if track:
            self._track_q(y)
        return y

    def garble_spec(self):
        return self.kind, {"idx": self.idx, "od": list(self.out_dims)}

    def __repr__(self) -> str:
        return f"Gather(in={self.in_dims}, out={self.out_dims})"


class Bilinear(Layer):
    """Bilinear resize of a (C, H, W) tensor to (C, OH, OW) (docs/BILINEAR.md): separable, one public two-tap table
    per axis. For output index o on an axis of n inputs and m outputs, in exact rational arithmetic,
      half_pixel:    src = (o + 1/2) n / m - 1/2, clamped to [0, n - 1]
      align_corners: src = o (n - 1) / (m - 1), 0 when m = 1
      asymmetric:    src = o n / m
    i0 = floor(src), i1 = min(i0 + 1, n - 1), lam = src - i0, n1 = floor(lam 2^b + 1/2), n0 = 2^b - n1. The axis'
    fraction bits b are the smallest value in 0..8 that makes every lam 2^b an integer (exact weights), else `bits`.
    With s = by + bx the quantized output is the exact integer
      y[c][oy][ox] = sum_{a, b in {0, 1}} ny_a[oy] nx_b[ox] x[c][iy_a[oy]][ix_b[ox]] = 2^s (interpolated value):
    it carries a scale 2^s larger than the input (pending scale bits, as a LeakyRelu's), which the next linear
    layer absorbs (in_scale_bits). Free in the label domain: public multiples and sums of labels, no tables, no PRG
    draws. Hardened encoding only, as ConvTranspose2d (the zero-mod-p weights differ per output position).

    factors: one number or (fh, fw), each with an integer n f (OH = H fh); or size = (OH, OW)."""

    kind = Kind.BILINEAR
    name = "bilinear"
    MODES = ("half_pixel", "align_corners", "asymmetric")
    MAX_BITS = 8

    def __init__(self, dims, factors=None, size=None, mode: str = "half_pixel", bits: int = 6):
        from fractions import Fraction

        dims = tuple(int(d) for d in dims)
        if len(dims) != 3 or min(dims) < 1:
            raise ValueError(f"bilinear: the input is (C, H, W), got {dims}")
        if mode not in self.MODES:
            raise ValueError(f"bilinear: mode is one of {self.MODES}, got {mode!r}")
        if int(bits) != bits or not 1 <= int(bits) <= self.MAX_BITS:
            raise ValueError(f"bilinear: bits must be an integer in [1, {self.MAX_BITS}], got {bits}")
        if (factors is None) == (size is None):
            raise ValueError("bilinear: give either factors or size")
        self.C, self.H, self.W = dims
        if size is not None:
            size = tuple(size)
            if len(size) != 2 or any(int(v) != v or int(v) < 1 for v in size):
                raise ValueError(f"bilinear: size is (OH, OW) with positive integers, got {size}")
            oh, ow = (int(v) for v in size)
        else:
            f = tuple(factors) if isinstance(factors, (tuple, list)) else (factors, factors)
            if len(f) != 2:
                raise ValueError(f"bilinear: factors is one number or (fh, fw), got {factors}")
            out = []
            for n, v in zip((self.H, self.W), f):
                m = Fraction(v) * n
                if m.denominator != 1 or m < 1:
                    raise ValueError(f"bilinear: factor {v} does not take an axis of {n} to a whole size; give size")
                out.append(int(m))
            oh, ow = out
        if (oh, ow) == (self.H, self.W):
            raise ValueError(f"bilinear: the output {(oh, ow)} equals the input")
        self.OH, self.OW, self.mode, self.bits = oh, ow, mode, int(bits)
        super().__init__(dims, (self.C, oh, ow))
        self.y0, self.y1, self.ny, self.by = self.axis_table(self.H, oh, mode, self.bits)
        self.x0, self.x1, self.nx, self.bx = self.axis_table(self.W, ow, mode, self.bits)
        for a in (self.y0, self.y1, self.ny, self.x0, self.x1, self.nx):
            a.setflags(write=False)  # garble_spec hands the arrays themselves to the native specs

    @staticmethod
    def axis_table(n: int, m: int, mode: str, bits: int):
        """(i0, i1, n1, b) of one axis: int64 arrays of length m and the axis' fraction bits."""
        from fractions import Fraction

        half = Fraction(1, 2)
        src = []
        for o in range(m):
            if mode == "half_pixel":
                s = min(max((o + half) * Fraction(n, m) - half, Fraction(0)), Fraction(n - 1))
            elif mode == "align_corners":
                s = Fraction(o * (n - 1), m - 1) if m > 1 else Fraction(0)
            else:
                s = Fraction(o * n, m)
            src.append(s)
        i0 = [s.numerator // s.denominator for s in src]
        lam = [s - i for s, i in zip(src, i0)]
        b = next((t for t in range(Bilinear.MAX_BITS + 1) if all((l * (1 << t)).denominator == 1 for l in lam)), bits)
        n1 = [int((l * (1 << b) + half).numerator // (l * (1 << b) + half).denominator) for l in lam]
        return (np.array(i0, dtype=np.int64), np.array([min(i + 1, n - 1) for i in i0], dtype=np.int64),
                np.array(n1, dtype=np.int64), b)

    @property
    def scale_bits(self) -> int:
        """s = by + bx: the output is 2^s times the interpolated value."""
        return self.by + self.bx

    def _taps(self, x, wy0, wy1, wx0, wx1):
        x = x.reshape(self.C, self.H, self.W)
        r = x[:, self.y0, :] * wy0[None, :, None] + x[:, self.y1, :] * wy1[None, :, None]
        return (r[:, :, self.x0] * wx0[None, None, :] + r[:, :, self.x1] * wx1[None, None, :]).reshape(-1)

    def plain_eval(self, x, track=True, ctx=None):
        sy, sx = float(1 << self.by), float(1 << self.bx)
        y = self._taps(np.asarray(x, dtype=np.float64), 1.0 - self.ny / sy, self.ny / sy, 1.0 - self.nx / sx,
                       self.nx / sx).astype(np.float32)
        if track:
            self._track_f(y)
        return y

    def plain_q_eval(self, x, track=True, ctx=None, crt_modulus=None):
        y = self._taps(np.asarray(x, dtype=np.int64), (1 << self.by) - self.ny, self.ny, (1 << self.bx) - self.nx,
                       self.nx)
        if track:
            self._track_q(y)  # 2^s times a convex combination: the output's own range bounds every partial sum
        return y

    def quantize(self, q_const):
        self.reset_ranges()

    def garble_spec(self):
        return self.kind, {"C": self.C, "H": self.H, "W": self.W, "OH": self.OH, "OW": self.OW, "by": self.by,
                           "bx": self.bx, "y0": self.y0, "y1": self.y1, "ny": self.ny, "x0": self.x0, "x1": self.x1,
                           "nx": self.nx}

    def __repr__(self) -> str:
        return (f"Bilinear(in={self.in_dims}, out={self.out_dims}, mode={self.mode}, "
                f"bits=({self.by}, {self.bx}))")


class Relu(Layer):
    """ReLU via approximate sign (type approx_relu). Reference: relu.h."""

    kind = Kind.RELU
    name = "approx_relu"

    def __init__(self, dims):
        super().__init__(dims, dims)

    def plain_eval(self, x, track=True, ctx=None):
        y = np.maximum(np.asarray(x), 0)
        if track:
            self._track_f(y)
        return y

    def plain_q_eval(self, x, track=True, ctx=None, crt_modulus=None):
        x = np.asarray(x, dtype=np.int64)
        y = np.maximum(x, 0)
        if track:
            self._track_q(x, y)
        return y

    def quantize(self, q_const):
        self.reset_ranges()


class LeakyRelu(Layer):
    """Leaky ReLU / PReLU with a dyadic slope (docs/LEAKY_RELU.md): slope_bits = s in [1, 8] and a numerator
    n_c = round(alpha_c 2^s) in [0, 2^s) per channel (a scalar slope is one channel group). The quantized
    function is y = 2^s x for x >= 0 and n_c x otherwise, exact: the output carries a scale 2^s larger than the
    input, which the next linear layer absorbs (in_scale_bits). y = n x + (2^s - n) relu(x), and a public
    multiple or a sum of labels is free, so the garbled tables are exactly a ReLU's."""

    kind = Kind.LEAKY
    name = "leaky_relu"
    MAX_SLOPE_BITS = 8

    def __init__(self, dims, alpha, slope_bits: int = 4):
        super().__init__(dims, dims)
        s = self._check_bits(slope_bits)
        a = np.asarray(alpha, dtype=np.float64).reshape(-1)
        if not np.all(np.isfinite(a)) or np.any(a < 0) or np.any(a >= 1):
            raise ValueError(f"leaky_relu: every slope must lie in [0, 1), got {a.tolist()}")
        n = np.floor(a * (1 << s) + 0.5).astype(np.int64)
        lost = (a > 0) & (n == 0)
        if lost.any():
            amin = float(a[lost].min())
            need = next(t for t in range(s + 1, 1100) if np.floor(amin * 2.0 ** t + 0.5) >= 1)
            raise ValueError(f"leaky_relu: slope {amin:g} rounds to 0 at slope_bits={s}; the smallest slope_bits "
                             f"that keeps it is {need}")
        if np.any(n >= (1 << s)):
            raise ValueError(f"leaky_relu: slope {float(a.max()):g} rounds to 1 at slope_bits={s}; slopes must "
                             f"stay below 1")
        self.alpha = a.astype(np.float32)
        self._set_n(n, s)

    @staticmethod
    def _check_bits(slope_bits) -> int:
        s = int(slope_bits)
        if s != slope_bits or not 1 <= s <= LeakyRelu.MAX_SLOPE_BITS:
            raise ValueError(f"leaky_relu: slope_bits must be an integer in [1, {LeakyRelu.MAX_SLOPE_BITS}], "
                             f"got {slope_bits}")
        return s

    def _set_n(self, n, s: int):
        n = np.asarray(n, dtype=np.int64).reshape(-1)
        if n.size not in (1, self.in_dims[0]):
            raise ValueError(f"leaky_relu: one slope or one per channel ({self.in_dims[0]}), got {n.size}")
        if np.any(n < 0) or np.any(n >= (1 << s)):
            raise ValueError(f"leaky_relu: slope numerators must lie in [0, 2^{s}), got {n.tolist()}")
        self.slope_bits, self.n = s, n
        # elements per channel group (channel of element e = e // bc)
        self.bc = self.out_size if n.size == 1 else self.out_size // n.size

    @classmethod
    def from_quantized(cls, dims, n, slope_bits: int) -> "LeakyRelu":
        s = cls._check_bits(slope_bits)
        l = cls(dims, 0.0, s)
        l._set_n(n, s)
        l.alpha = (l.n.astype(np.float64) / (1 << s)).astype(np.float32)
        return l

    def _per_elem(self, v):
        return np.repeat(np.asarray(v), self.bc) if len(v) > 1 else np.asarray(v)[0]

    def plain_eval(self, x, track=True, ctx=None):
        x = np.asarray(x, dtype=np.float32).reshape(-1)
        y = np.where(x >= 0, x, x * self._per_elem(self.alpha)).astype(np.float32)
        if track:
            self._track_f(y)
        return y

    def plain_q_eval(self, x, track=True, ctx=None, crt_modulus=None):
        x = np.asarray(x, dtype=np.int64).reshape(-1)
        y = np.where(x >= 0, x * (1 << self.slope_bits), x * self._per_elem(self.n))
        if track:
            self._track_q(x, y)
        return y

    def quantize(self, q_const):
        self.reset_ranges()

    def garble_spec(self):
        return self.kind, {"s": self.slope_bits, "n": [int(v) for v in self.n], "bc": int(self.bc)}

    def __repr__(self) -> str:
        return f"LeakyRelu(dims={self.in_dims}, n={self.n.tolist()}, slope_bits={self.slope_bits})"


class PiecewiseLinear(Layer):
    """Continuous piecewise-linear activation with m <= 8 breakpoints (docs/PWL.md): float breakpoints
    t_1 < ... < t_m, m + 1 segment slopes a_0 .. a_m (|a_j| <= 2), the value v at t_1 and slope_bits = s in [1, 8].
    Quantized under ScaleQuant (act_scale = 2^l) exactly and in integers:
      T_i = llround(t_i 2^l), A_j = round(a_j 2^s), D_i = A_i - A_(i-1), V = llround(v 2^(l+s)),
      y_q(x) = V + A_0 (x - T_1) + sum_i D_i relu(x - T_i).
    l = q_parameter (default 5, the zoo's). The output carries a scale 2^s larger than the input (pending scale bits, as a LeakyRelu's). Garbled as one sign
    and one set of mixed-modulus half gates per breakpoint with D_i != 0, all on the labels of x, and a free linear
    combination of the labels (csrc/gadgets.h PwlPlan). The named constructors tag the layer for the ONNX exporter."""

    kind = Kind.PWL
    name = "pwl"
    MAX_BREAKS = 8
    MAX_SLOPE_BITS = 8
    MAX_SLOPE = 2.0
    FN_CODES = {None: 0, "sigmoid": 1, "tanh": 2, "hard_sigmoid": 3}

    def __init__(self, dims, knots, slopes, value, slope_bits: int = 8, q_parameter: int = 5,
                 q_method: QuantizationMethod = QuantizationMethod.ScaleQuant):
        super().__init__(dims, dims)
        s = self._check_bits(slope_bits)
        self.q_method, self.q_parameter = QuantizationMethod(q_method), int(q_parameter)
        if self.q_method != QuantizationMethod.ScaleQuant:
            raise ValueError(f"pwl: a piecewise-linear activation exists under ScaleQuant only (its output carries a "
                             f"power-of-two scale 2^{s} that the next Rescale absorbs), not {self.q_method.name}")
        if self.q_parameter < 0:
            raise ValueError(f"pwl: q_parameter must be >= 0, got {q_parameter}")
        t = np.asarray(knots, dtype=np.float64).reshape(-1)
        a = np.asarray(slopes, dtype=np.float64).reshape(-1)
        if not 1 <= t.size <= self.MAX_BREAKS:
            raise ValueError(f"pwl: between 1 and {self.MAX_BREAKS} breakpoints, got {t.size}")
        if a.size != t.size + 1:
            raise ValueError(f"pwl: {t.size} breakpoints need {t.size + 1} slopes, got {a.size}")
        if not (np.all(np.isfinite(t)) and np.all(np.isfinite(a)) and np.isfinite(value)):
            raise ValueError("pwl: breakpoints, slopes and value must be finite")
        if np.any(np.abs(a) > self.MAX_SLOPE):
            raise ValueError(f"pwl: every slope must satisfy |a| <= {self.MAX_SLOPE:g}, got {a.tolist()}")
        self.t, self.a, self.v = t, a, float(value)
        self.fn, self.fn_params = None, {}
        scale = 1 << self.q_parameter
        T = quantize_scale(t, scale)
        A = np.floor(a * (1 << s) + 0.5).astype(np.int64)
        V = int(quantize_scale(np.asarray([self.v]), scale * (1 << s))[0])
        self._set_q(T, A, V, s)

    @staticmethod
    def _check_bits(slope_bits) -> int:
        s = int(slope_bits)
        if s != slope_bits or not 1 <= s <= PiecewiseLinear.MAX_SLOPE_BITS:
            raise ValueError(f"pwl: slope_bits must be an integer in [1, {PiecewiseLinear.MAX_SLOPE_BITS}], "
                             f"got {slope_bits}")
        return s

    def _set_q(self, T, A, V, s: int):
        T = np.asarray(T, dtype=np.int64).reshape(-1)
        A = np.asarray(A, dtype=np.int64).reshape(-1)
        if not 1 <= T.size <= self.MAX_BREAKS:
            raise ValueError(f"pwl: between 1 and {self.MAX_BREAKS} breakpoints, got {T.size}")
        if A.size != T.size + 1:
            raise ValueError(f"pwl: {T.size} breakpoints need {T.size + 1} slopes, got {A.size}")
        if np.any(np.diff(T) <= 0):
            raise ValueError(f"pwl: the quantized breakpoints must increase strictly, got {T.tolist()} (a larger "
                             f"q_parameter separates them)")
        if np.any(np.abs(A) > int(self.MAX_SLOPE * (1 << s))):
            raise ValueError(f"pwl: every slope numerator must satisfy |A| <= {int(self.MAX_SLOPE * (1 << s))}, "
                             f"got {A.tolist()}")
        D = np.diff(A)
        if not np.any(D != 0):
            raise ValueError(f"pwl: no breakpoint is left at slope_bits={s}: every slope change rounds to 0")
        self.slope_bits, self.T, self.A, self.D, self.V = s, T, A, D, int(V)

    @property
    def kept(self) -> list:
        """Indices of the breakpoints of the garbled form (D_i != 0)."""
        return [int(i) for i in np.flatnonzero(self.D)]

    @classmethod
    def from_quantized(cls, dims, T, A, V, slope_bits: int) -> "PiecewiseLinear":
        s = cls._check_bits(slope_bits)
        T = np.asarray(T, dtype=np.int64).reshape(-1)
        A = np.asarray(A, dtype=np.int64).reshape(-1)
        if not 1 <= T.size <= cls.MAX_BREAKS or A.size != T.size + 1:
            raise ValueError(f"pwl: between 1 and {cls.MAX_BREAKS} breakpoints and one more slope, got {T.size} and "
                             f"{A.size}")
        if np.any(np.abs(A) > int(cls.MAX_SLOPE * (1 << s))):
            raise ValueError(f"pwl: every slope numerator must satisfy |A| <= {int(cls.MAX_SLOPE * (1 << s))}, "
                             f"got {A.tolist()}")
        l = cls(dims, T.astype(np.float64), A.astype(np.float64) / (1 << s), float(V) / (1 << s), s, 0)
        l._set_q(T, A, V, s)
        return l

    @classmethod
    def interpolate(cls, dims, xs, ys, slope_bits: int = 8, q_parameter: int = 5,
                    q_method: QuantizationMethod = QuantizationMethod.ScaleQuant) -> "PiecewiseLinear":
        """The interpolant through (xs_i, ys_i), constant outside [xs_1, xs_m]."""
        xs = np.asarray(xs, dtype=np.float64).reshape(-1)
        ys = np.asarray(ys, dtype=np.float64).reshape(-1)
        if xs.size != ys.size or xs.size < 1:
            raise ValueError(f"pwl: interpolate needs as many values as knots, got {xs.size} and {ys.size}")
        if np.any(np.diff(xs) <= 0):
            raise ValueError(f"pwl: the knots must increase strictly, got {xs.tolist()}")
        inner = np.diff(ys) / np.diff(xs) if xs.size > 1 else np.zeros(0)
        return cls(dims, xs, np.concatenate([[0.0], inner, [0.0]]), ys[0], slope_bits, q_parameter, q_method)

    SIGMOID_KNOTS = (-5.0, -3.0, -2.0, -1.0, 1.0, 2.0, 3.0, 5.0)

    @classmethod
    def sigmoid(cls, dims, slope_bits: int = 8, q_parameter: int = 5,
                q_method: QuantizationMethod = QuantizationMethod.ScaleQuant) -> "PiecewiseLinear":
        xs = np.asarray(cls.SIGMOID_KNOTS)
        l = cls.interpolate(dims, xs, 1.0 / (1.0 + np.exp(-xs)), slope_bits, q_parameter, q_method)
        l.fn = "sigmoid"
        return l

    @classmethod
    def tanh(cls, dims, slope_bits: int = 8, q_parameter: int = 5,
             q_method: QuantizationMethod = QuantizationMethod.ScaleQuant) -> "PiecewiseLinear":
        xs = np.asarray(cls.SIGMOID_KNOTS) / 2.0
        l = cls.interpolate(dims, xs, np.tanh(xs), slope_bits, q_parameter, q_method)
        l.fn = "tanh"
        return l

    @classmethod
    def hard_sigmoid(cls, dims, alpha: float = 0.2, beta: float = 0.5, slope_bits: int = 8, q_parameter: int = 5,
                     q_method: QuantizationMethod = QuantizationMethod.ScaleQuant) -> "PiecewiseLinear":
        alpha, beta = float(alpha), float(beta)
        if not (np.isfinite(alpha) and np.isfinite(beta) and alpha > 0):
            raise ValueError(f"pwl: hard_sigmoid needs a finite alpha > 0 and a finite beta, got ({alpha}, {beta})")
        l = cls(dims, [-beta / alpha, (1.0 - beta) / alpha], [0.0, alpha, 0.0], 0.0, slope_bits, q_parameter, q_method)
        l.fn, l.fn_params = "hard_sigmoid", {"alpha": alpha, "beta": beta}
        return l

    def plain_eval(self, x, track=True, ctx=None):
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        y = self.v + self.a[0] * (x - self.t[0])
        for i, d in enumerate(np.diff(self.a)):
            y = y + d * np.maximum(x - self.t[i], 0.0)
        y = y.astype(np.float32)
        if track:
            self._track_f(y)
        return y

    def plain_q_eval(self, x, track=True, ctx=None, crt_modulus=None):
        x = np.asarray(x, dtype=np.int64).reshape(-1)
        y = self.V + int(self.A[0]) * (x - int(self.T[0]))
        for T, D in zip(self.T, self.D):
            y = y + int(D) * np.maximum(x - int(T), 0)
        if track:
            # every sign input x - T_i must lie in [-M/2, M/2)
            self._track_q(x, y, x - int(self.T[0]), x - int(self.T[-1]))
        return y

    def quantize(self, q_const):
        self.reset_ranges()

    def garble_spec(self):
        return self.kind, {"s": self.slope_bits, "T": [int(v) for v in self.T], "A": [int(v) for v in self.A],
                           "V": int(self.V), "fn": self.FN_CODES[self.fn]}

    def __repr__(self) -> str:
        return (f"PiecewiseLinear(dims={self.in_dims}, T={self.T.tolist()}, A={self.A.tolist()}, V={self.V}, "
                f"slope_bits={self.slope_bits}" + (f", fn={self.fn}" if self.fn else "") + ")")


class Clip(Layer):
    """Clamp to [lo, hi] (ONNX Clip; PyTorch ReLU6, Hardtanh, clamp). The quantized
    bounds are q_b = llround(b * act_scale) with the scheme's activation scale
    (ScaleQuant: 2^l, ScaleQuantPlus: s). SimpleQuant scales biases and products
    differently, so it has no activation scale and a Clip is refused under it.
    Garbled as two signs of the same input, one set of mixed-modulus half gates
    and a 2-row projection per residue (csrc/gadgets.h ClipPlan)."""

    kind = Kind.CLIP
    name = "clip"

    def __init__(self, dims, lo: float, hi: float, q_parameter: int = 0,
                 q_method: QuantizationMethod = QuantizationMethod.ScaleQuant):
        super().__init__(dims, dims)
        self.lo, self.hi = float(lo), float(hi)
        if not (np.isfinite(self.lo) and np.isfinite(self.hi) and self.lo < self.hi):
            raise ValueError(f"clip: bounds must be finite with lo < hi, got ({lo}, {hi})")
        self.q_method, self.q_parameter = QuantizationMethod(q_method), int(q_parameter)
        if self.q_method == QuantizationMethod.SimpleQuant:
            raise ValueError("clip: SimpleQuant has no single activation scale to quantize the bounds with; "
                             "use ScaleQuant or ScaleQuantPlus")
        scale = (1 << self.q_parameter) if self.q_method == QuantizationMethod.ScaleQuant else self.q_parameter
        q = quantize_scale(np.asarray([self.lo, self.hi]), scale)
        self._set_q(int(q[0]), int(q[1]))

    def _set_q(self, q_lo: int, q_hi: int):
        if not int(q_lo) < int(q_hi):
            raise ValueError(f"clip: quantized bounds must satisfy q_lo < q_hi, got ({q_lo}, {q_hi})")
        self.q_lo, self.q_hi = int(q_lo), int(q_hi)

    @classmethod
    def from_quantized(cls, dims, q_lo: int, q_hi: int) -> "Clip":
        if not int(q_lo) < int(q_hi):
            raise ValueError(f"clip: quantized bounds must satisfy q_lo < q_hi, got ({q_lo}, {q_hi})")
        c = cls(dims, float(q_lo), float(q_hi))
        c._set_q(q_lo, q_hi)
        return c

    def plain_eval(self, x, track=True, ctx=None):
        y = np.clip(np.asarray(x), np.float32(self.lo), np.float32(self.hi))
        if track:
            self._track_f(y)
        return y

    def plain_q_eval(self, x, track=True, ctx=None, crt_modulus=None):
        x = np.asarray(x, dtype=np.int64)
        y = np.clip(x, self.q_lo, self.q_hi)
        if track:
            # both sign inputs must lie in [-M/2, M/2)
            self._track_q(x, y, x - self.q_lo, x - self.q_hi)
        return y

    def quantize(self, q_const):
        self.reset_ranges()

    def garble_spec(self):
        return self.kind, {"lo": self.q_lo, "hi": self.q_hi}

    def __repr__(self) -> str:
        return f"Clip(dims={self.in_dims}, q_lo={self.q_lo}, q_hi={self.q_hi})"


class Sign(Layer):
    """Sign activation x >= 0 ? 1 : -1 (Tanh replacement). Reference: sign.h."""

    kind = Kind.SIGN
    name = "sign"

    def __init__(self, dims):
        super().__init__(dims, dims)

    def plain_eval(self, x, track=True, ctx=None):
        y = np.where(np.asarray(x) >= 0, 1.0, -1.0).astype(np.float32)
        if track:
            self._track_f(y)
        return y

    def plain_q_eval(self, x, track=True, ctx=None, crt_modulus=None):
        y = np.where(np.asarray(x) >= 0, 1, -1).astype(np.int64)
        if track:
            self._track_q(y)
        return y

    def quantize(self, q_const):
        self.reset_ranges()


class Rescale(Layer):
    """CRT scaling. Legacy DASH: `l` halvings (sign base extension); ReDash:
    division by CRT moduli `s` (base extension). Reference: rescale.h,
    rescale_gadget.h. With `crt_modulus` given, plain_q_eval reproduces the
    garbled semantics exactly: floor((x + (M/2 mod S)) / S) per step, which
    equals the reference's ceil(x/2) for the legacy mode."""

    kind = Kind.RESCALE
    name = "rescale"

    def __init__(self, l_or_s, dims):
        super().__init__(dims, dims)
        if isinstance(l_or_s, (list, tuple, np.ndarray)):
            self.l, self.s, self.use_sign_base_extension = -1, [int(v) for v in l_or_s], False
        else:
            self.l, self.s, self.use_sign_base_extension = int(l_or_s), [-1], True

    def _apply(self, x, crt_modulus):
        if self.use_sign_base_extension:
            if crt_modulus is None:
                return ceil_div(x, 1 << self.l)
            y = x
            for _ in range(self.l):
                y = (y + (crt_modulus // 2) % 2) // 2
            return y
        S = 1
        for f in self.s:
            S *= f
        if crt_modulus is None:
            y = x
            for f in self.s:
                y = ceil_div(y, f)
            return y
        return (x + (crt_modulus // 2) % S) // S

    def plain_eval(self, x, track=True, ctx=None):
        return np.asarray(x)

    def plain_q_eval(self, x, track=True, ctx=None, crt_modulus=None):
        x = np.asarray(x, dtype=np.int64)
        y = self._apply(x, crt_modulus)
        if track:
            self._track_q(x, y)
            if x.size:
                self.in_min_q = min(self.in_min_q, int(x.min()))
                self.in_max_q = max(self.in_max_q, int(x.max()))
        return y

    def reset_ranges(self):
        super().reset_ranges()
        self.in_min_q = Q_MAX  # tracked range of the rescale's input (mixed-radix headroom check)
        self.in_max_q = Q_MIN

    @property
    def input_tracked(self) -> bool:
        return self.in_max_q >= self.in_min_q

    def mrs_limit(self, crt_modulus: int) -> int:
        """Exclusive upper bound of the inputs on which the single-shot mixed-radix rescale
        (gadgets.h RescaleMrsPlan) equals the reference's l-fold halving: x + U < M with
        U = M/2 rounded up to S - 1 mod S, S = 2^l (the top U - M/2 < S values wrap)."""
        M, S = int(crt_modulus), 1 << self.l
        h = M // 2
        U = h + (S - 1 - h % S) % S
        return M - U

    def garble_spec(self):
        if self.use_sign_base_extension:
            return self.kind, {"mode": 0, "l": self.l}
        return self.kind, {"mode": 1, "s": list(self.s)}


class Flatten(Layer):
    kind = Kind.FLATTEN
    name = "flatten"

    def __init__(self, dims):
        super().__init__(dims, (_size(dims),))

    def plain_eval(self, x, track=True, ctx=None):
        return np.asarray(x).reshape(-1)

    def plain_q_eval(self, x, track=True, ctx=None, crt_modulus=None):
        if track:
            self.min_q, self.max_q = 0, 0
        return np.asarray(x).reshape(-1)


def _pool_out(n: int, k: int, s: int, p: int, ceil_mode: bool) -> int:
    """PyTorch/ONNX pooled size of one axis: floor_or_ceil((n + 2p - k)/s) + 1; with
    ceil_mode the last window must start inside the image or its left padding."""
    span = n + 2 * p - k
    if span < 0:
        raise ValueError(f"pool kernel {k} larger than the padded input {n} + 2*{p}")
    o = (-(-span // s) if ceil_mode else span // s) + 1
    if ceil_mode and (o - 1) * s >= n + p:
        o -= 1
    return o


class _Pool2d(Layer):
    """Shared pooling geometry: symmetric padding (at most half the kernel) and
    ceil_mode, with the PyTorch/ONNX output-size rule."""

    def __init__(self, input_width, input_height, channel, kernel_width, kernel_height, stride_width=None,
                 stride_height=None, pad_width=0, pad_height=0, ceil_mode=False):
        self.C, self.H, self.W = int(channel), int(input_height), int(input_width)
        self.kh, self.kw = int(kernel_height), int(kernel_width)
        self.sh = int(stride_height if stride_height is not None else kernel_height)
        self.sw = int(stride_width if stride_width is not None else kernel_width)
        self.ph, self.pw, self.ceil_mode = int(pad_height), int(pad_width), bool(ceil_mode)
        if self.ph < 0 or self.pw < 0 or 2 * self.ph > self.kh or 2 * self.pw > self.kw:
            raise ValueError(f"pool padding ({self.ph}, {self.pw}) must be at most half the kernel "
                             f"({self.kh}, {self.kw})")
        self.OH = _pool_out(self.H, self.kh, self.sh, self.ph, self.ceil_mode)
        self.OW = _pool_out(self.W, self.kw, self.sw, self.pw, self.ceil_mode)
        super().__init__((self.C, self.H, self.W), (self.C, self.OH, self.OW))

    @property
    def padded(self) -> bool:
        return bool(self.ph or self.pw or self.ceil_mode)

    def _coords(self, dy, dx):
        """Image coordinates (unclamped) of tap (dy, dx) for every output row / column."""
        return (np.arange(self.OH) * self.sh + dy - self.ph, np.arange(self.OW) * self.sw + dx - self.pw)

    def garble_spec(self):
        spec = {"C": self.C, "H": self.H, "W": self.W, "kh": self.kh, "kw": self.kw, "sh": self.sh, "sw": self.sw}
        # emitted only when set: pools without padding keep their wire bytes
        if self.ph:
            spec["ph"] = self.ph
        if self.pw:
            spec["pw"] = self.pw
        if self.ceil_mode:
            spec["ceil"] = 1
        return self.kind, spec


class MaxPool2d(_Pool2d):
    """Max pooling as a pairwise tree of max(a,b) = a + relu(b - a).
    Reference: max_pool2d.h, garbled_maxpool2d.h (output dims use the stride,
    fixing §2.7 #8).

    With padding or ceil_mode a tap outside the image is replaced by the tap at
    the clamped coordinate. Pads are at most half the kernel, so that tap lies in
    the same window and the max is unchanged; every window keeps kh*kw values
    and the max tree stays uniform. The duplicated taps of border windows cost
    real ReLU gadgets (tables and evaluation work); that is accepted in place of
    ragged trees."""

    kind = Kind.MAXPOOL
    name = "max_pool"

    def _windows(self, x):
        x = np.asarray(x).reshape(self.C, self.H, self.W)
        out = []
        for dy in range(self.kh):
            for dx in range(self.kw):
                ys, xs = self._coords(dy, dx)
                ys, xs = np.clip(ys, 0, self.H - 1), np.clip(xs, 0, self.W - 1)
                out.append(x[:, ys[:, None], xs[None, :]])
        return out

    def plain_eval(self, x, track=True, ctx=None):
        y = np.max(np.stack(self._windows(x)), axis=0).reshape(-1)
        if track:
            self._track_f(y)
        return y

    def plain_q_eval(self, x, track=True, ctx=None, crt_modulus=None):
        w = self._windows(np.asarray(x, dtype=np.int64))
        y = np.max(np.stack(w), axis=0).reshape(-1)
        if track:
            # differences b - a feed the ReLU gadgets (duplicated border taps included)
            self._track_q(y, *[a - b for a in w for b in w])
        return y


class SumPool2d(_Pool2d):
    """Window sum (free in the label domain). Average pooling = SumPool2d + a
    rescale or a weight fold into the next linear layer. With padding or
    ceil_mode the taps outside the image are skipped (zero padding)."""

    kind = Kind.SUMPOOL
    name = "sum_pool"

    def _sum(self, x):
        x = np.asarray(x).reshape(self.C, self.H, self.W)
        acc = np.zeros((self.C, self.OH, self.OW), dtype=x.dtype)
        for dy in range(self.kh):
            for dx in range(self.kw):
                ys, xs = self._coords(dy, dx)
                oy = np.nonzero((ys >= 0) & (ys < self.H))[0]
                ox = np.nonzero((xs >= 0) & (xs < self.W))[0]
                if oy.size and ox.size:
                    acc[:, oy[:, None], ox[None, :]] += x[:, ys[oy][:, None], xs[ox][None, :]]
        return acc.reshape(-1)

    def plain_eval(self, x, track=True, ctx=None):
        return self._sum(np.asarray(x, dtype=np.float32))

    def plain_q_eval(self, x, track=True, ctx=None, crt_modulus=None):
        y = self._sum(np.asarray(x, dtype=np.int64))
        if track:
            self._track_q(y)
        return y


class Add(Layer):
    """Residual addition of the current tensor and the output of layer `src`
    (-1 = circuit input). Free in the label domain."""

    kind = Kind.ADD
    name = "add"

    def __init__(self, dims, src: int):
        super().__init__(dims, dims)
        self.src = int(src)

    def plain_eval(self, x, track=True, ctx=None):
        return np.asarray(x) + ctx[self.src + 1]

    def plain_q_eval(self, x, track=True, ctx=None, crt_modulus=None):
        y = np.asarray(x, dtype=np.int64) + np.asarray(ctx[self.src + 1], dtype=np.int64)
        if track:
            self._track_q(y)
        return y

    def garble_spec(self):
        return self.kind, {"src": self.src}


class Concat(Layer):
    """Channel concatenation of the outputs of layers `srcs` (-1 = circuit
    input), in that order; the previous layer is named like any other operand.
    With the [C][H][W] layout this is the concatenation of the flat vectors, so
    1-D operands concatenate too. Free in the label domain: no tables, no PRG
    draws, no constants."""

    kind = Kind.CONCAT
    name = "concat"

    def __init__(self, dims_list, srcs):
        dims_list = [tuple(int(v) for v in d) for d in dims_list]
        self.srcs = [int(s) for s in srcs]
        if not dims_list or len(dims_list) != len(self.srcs):
            raise ValueError("Concat needs one dims entry per source")
        d0 = dims_list[0]
        for d in dims_list:
            if len(d) != len(d0) or d[1:] != d0[1:]:
                raise ValueError(f"Concat operands must agree on all but the channel axis: {dims_list}")
        self.dims_list = dims_list
        super().__init__(d0, (sum(d[0] for d in dims_list),) + d0[1:])

    def _cat(self, ctx, dtype):
        parts = [np.asarray(ctx[s + 1], dtype=dtype).reshape(-1) for s in self.srcs]
        for p, d in zip(parts, self.dims_list):
            assert p.size == _size(d), "concat operand size mismatch"
        return np.concatenate(parts)

    def plain_eval(self, x, track=True, ctx=None):
        return self._cat(ctx, np.float32)

    def plain_q_eval(self, x, track=True, ctx=None, crt_modulus=None):
        y = self._cat(ctx, np.int64)
        if track:
            self._track_q(y)
        return y

    def garble_spec(self):
        return self.kind, {"srcs": list(self.srcs)}


class Mul(Layer):
    """Product of two secret tensors: x, the layer's input, times y, the output
    of layer `src` (-1 = circuit input), as for Add. `src_dims` equal to `dims`
    (the default) multiplies elementwise; dims (C, H, W) with src_dims (C,) or
    (C, 1, 1) broadcasts y over the plane, out[c, h, w] = x[c, h, w] * y[c]. The
    full tensor is always x. Mul.square(dims), or a `src` that resolves to the
    layer's own input (its in_src, or the layer before it), is the square x * x. Scale-free: whoever builds the circuit
    puts the scheme's rescale behind it, as after a conv. Garbled as the
    generalized half gates, or one projection per residue for the square
    (csrc/gadgets.h MulPlan); hardened encoding only."""

    kind = Kind.MUL
    name = "mul"

    def __init__(self, dims, src: Optional[int], src_dims=None):
        dims = tuple(int(d) for d in dims)
        sd = dims if src_dims is None else tuple(int(d) for d in src_dims)
        # an explicit channel operand broadcasts even over a 1 x 1 plane (bc = 1)
        if src_dims is not None and len(dims) == 3 and sd in ((dims[0],), (dims[0], 1, 1)):
            self.bc = dims[1] * dims[2]
        elif sd == dims:
            self.bc = 0
        else:
            raise ValueError(f"mul: operand dims {sd} neither equal {dims} nor are its channels, "
                             "(C,) or (C, 1, 1) against (C, H, W); the full tensor is the layer's input")
        if src is None and self.bc:
            raise ValueError(f"mul: a square has no second operand, got src_dims {sd}")
        super().__init__(dims, dims)
        self.src_dims = sd
        self.src = None if src is None else int(src)

    @classmethod
    def square(cls, dims) -> "Mul":
        return cls(dims, None)

    @property
    def is_square(self) -> bool:
        """The layer alone can tell: no src, or a src that is its own in_src. A sequential layer whose src is the
        layer before it is a square too, which only its place in the circuit shows: squares_at."""
        return self.src is None or (self.in_src is not None and int(self.in_src) == self.src and not self.bc)

    def squares_at(self, index: int) -> bool:
        """As layer `index` of a circuit: does src resolve to the same tensor as the input? (Circuit.garble_specs
        garbles such a layer as the square.)"""
        x_src = int(self.in_src) if self.in_src is not None else index - 1
        return self.src is None or (not self.bc and self.src == x_src)

    def _y(self, x, ctx, dtype):
        if self.is_square:
            return x
        y = np.asarray(ctx[self.src + 1], dtype=dtype).reshape(-1)
        assert y.size == _size(self.src_dims), "mul operand size mismatch"
        return np.repeat(y, self.bc) if self.bc else y

    def plain_eval(self, x, track=True, ctx=None):
        x = np.asarray(x, dtype=np.float32).reshape(-1)
        out = x * self._y(x, ctx, np.float32)
        if track:
            self._track_f(out)
        return out

    def plain_q_eval(self, x, track=True, ctx=None, crt_modulus=None):
        x = np.asarray(x, dtype=np.int64).reshape(-1)
        y = self._y(x, ctx, np.int64)
        if x.size:
            ax = max(abs(int(x.min())), abs(int(x.max())))
            ay = max(abs(int(y.min())), abs(int(y.max())))
            if ax * ay >= 1 << 62:
                raise OverflowError(f"mul: the product of operands up to {ax} and {ay} does not fit 62 bits")
        out = x * y
        if track:
            self._track_q(x, y, out)
        return out

    def garble_spec(self):
        if self.is_square:
            return self.kind, {"sq": 1}
        p = {"src": self.src}
        if self.bc:
            p["bc"] = self.bc
        return self.kind, p

    def __repr__(self) -> str:
        return (f"Mul.square({self.in_dims})" if self.is_square else
                f"Mul({self.in_dims}, src={self.src}, src_dims={self.src_dims})")


def _as_matrix(d: Sequence[int]) -> tuple[int, int]:
    """Dims (d0, d1, ...) as the matrix d0 x prod(d1...) of the flat [C][H][W] order; (n,) is 1 x n."""
    d = tuple(int(v) for v in d)
    if not d:
        raise ValueError("matmul: an operand needs at least one axis")
    return (1, d[0]) if len(d) == 1 else (d[0], _size(d[1:]))


def _head_matrix(d: Sequence[int], heads: int) -> tuple[int, int]:
    """One head's matrix of a tensor of dims d split into `heads` contiguous slabs along its leading axis: slab
    dims (d[0] // heads, *d[1:]), read by _as_matrix."""
    d = tuple(int(v) for v in d)
    if heads == 1:
        return _as_matrix(d)
    if len(d) < 2:
        raise ValueError(f"matmul: a 1-D operand of dims {d} cannot be split into {heads} heads")
    if d[0] % heads:
        raise ValueError(f"matmul: the leading axis of dims {d} does not split into {heads} heads")
    return _as_matrix((d[0] // heads,) + d[1:])


class MatMul(Layer):
    """Contraction of two secret tensors: out[i, l] = sum_t x[i, t] * y[t, l].
    x is the layer's input, y the output of layer `src` (-1 = circuit input), as
    for Add and Mul. A tensor of dims (d0, d1, ...) is read as the matrix
    d0 x prod(d1...) in its flat order, a 1-D tensor (n,) as 1 x n; `trans_a` /
    `trans_b` transpose that view (strides only, no data moves). After the flags
    x is M x T and y is T x N. The output has dims (M, N), or `out_dims` of equal
    size. `src` may name the layer's own input (x x^T with trans_b): it is
    garbled as the general product. Scale-free: whoever builds the circuit puts
    the scheme's rescale behind it, as after a Mul. Garbled as T generalized half
    gates per output element and residue, summed (csrc/gadgets.h MatMulPlan);
    hardened encoding only.
    `heads` = G > 1 contracts G independent matrix pairs: both operands split
    along their leading axis (dims[0] % G == 0) into G contiguous slabs of dims
    (dims[0] // G, *dims[1:]), each read as a matrix and transposed as above, and
    out[g, i, l] = sum_t x_g[i, t] * y_g[t, l], flat head-major, default dims
    (G M, N). M, T, N are per head. G = 1 is the single contraction."""

    kind = Kind.MATMUL
    name = "matmul"

    def __init__(self, dims, src: int, src_dims, trans_a: bool = False, trans_b: bool = False, out_dims=None,
                 heads: int = 1):
        dims = tuple(int(d) for d in dims)
        sd = tuple(int(d) for d in src_dims)
        self.trans_a, self.trans_b = bool(trans_a), bool(trans_b)
        G = int(heads)
        if G < 1:
            raise ValueError(f"matmul: heads = {heads} of dims {dims} and {sd}: at least one head")
        xr, xc = _head_matrix(dims, G)
        yr, yc = _head_matrix(sd, G)
        M, T = (xc, xr) if self.trans_a else (xr, xc)
        T2, N = (yc, yr) if self.trans_b else (yr, yc)
        per = " per head" if G > 1 else ""
        if T != T2:
            raise ValueError(f"matmul: x of dims {dims} is {M} x {T}{' (transposed)' if self.trans_a else ''} and y of "
                             f"dims {sd} is {T2} x {N}{' (transposed)' if self.trans_b else ''}{per}: the inner sizes "
                             f"differ")
        od = (G * M, N) if out_dims is None else tuple(int(d) for d in out_dims)
        if _size(od) != G * M * N:
            raise ValueError(f"matmul: out_dims {od} do not hold the {M} x {N} product{per} of dims {dims} and {sd}"
                             f"{f' in {G} heads' if G > 1 else ''}")
        super().__init__(dims, od)
        self.src_dims = sd
        self.src = int(src)
        self.heads = G
        self.M, self.T, self.N = M, T, N

    def _views(self, x, ctx, dtype):
        """The operands as [G][M][T] and [G][T][N]."""
        G = self.heads
        x = np.asarray(x, dtype=dtype).reshape((G,) + _head_matrix(self.in_dims, G))
        y = np.asarray(ctx[self.src + 1], dtype=dtype).reshape(-1)
        assert y.size == _size(self.src_dims), "matmul operand size mismatch"
        y = y.reshape((G,) + _head_matrix(self.src_dims, G))
        return (x.transpose(0, 2, 1) if self.trans_a else x), (y.transpose(0, 2, 1) if self.trans_b else y)

    def plain_eval(self, x, track=True, ctx=None):
        a, b = self._views(x, ctx, np.float32)
        out = np.stack([a[g] @ b[g] for g in range(self.heads)]).astype(np.float32).reshape(-1)
        if track:
            self._track_f(out)
        return out

    def plain_q_eval(self, x, track=True, ctx=None, crt_modulus=None):
        a, b = self._views(x, ctx, np.int64)
        if a.size and b.size:
            ax = max(abs(int(a.min())), abs(int(a.max())))
            ay = max(abs(int(b.min())), abs(int(b.max())))
            if self.T * ax * ay >= 1 << 62:
                raise OverflowError(f"matmul: {self.T} products of operands up to {ax} and {ay} do not fit 62 bits")
        out = (a[:, :, :, None] * b[:, None, :, :]).sum(axis=2, dtype=np.int64).reshape(-1)
        if track:
            self._track_q(a, b, out)
        return out

    def garble_spec(self):
        p = {"src": self.src, "M": self.M, "T": self.T, "N": self.N}
        if self.trans_a:
            p["ta"] = 1
        if self.trans_b:
            p["tb"] = 1
        if self.heads > 1:
            p["G"] = self.heads
        return self.kind, p

    def __repr__(self) -> str:
        return (f"MatMul({self.in_dims}, src={self.src}, src_dims={self.src_dims}, trans_a={self.trans_a}, "
                f"trans_b={self.trans_b}, out_dims={self.out_dims}{f', heads={self.heads}' if self.heads > 1 else ''})")


# ---- test-only layers (reference: projection.h, mult_layer.h, mixed_mod_mult_layer.h, max.h, base_extension.h)
class Projection(Layer):
    kind = Kind.PROJ
    name = "projection"

    def __init__(self, dims, in_moduli: Sequence[int], out_moduli: Sequence[int], functionality: Callable[[int], int]):
        super().__init__(dims, dims)
        self.in_moduli, self.out_moduli, self.functionality = list(in_moduli), list(out_moduli), functionality

    def plain_eval(self, x, track=True, ctx=None):
        return np.asarray(x)

    def plain_q_eval(self, x, track=True, ctx=None, crt_modulus=None):
        return np.asarray(x)

    def garble_spec(self):
        p = {"in_mod": self.in_moduli, "out_mod": self.out_moduli}
        for j, m in enumerate(self.in_moduli):
            p[f"fn.{j}"] = [int(self.functionality(v)) for v in range(m)]
        return self.kind, p


class MultLayer(Layer):
    kind = Kind.MULT
    name = "mult_layer"

    def __init__(self, in_dims, out_dims=None):
        n = _size(in_dims)
        super().__init__(in_dims, out_dims or (n // 2,))

    def plain_eval(self, x, track=True, ctx=None):
        x = np.asarray(x).reshape(-1)
        return x[0::2] * x[1::2]

    def plain_q_eval(self, x, track=True, ctx=None, crt_modulus=None):
        x = np.asarray(x, dtype=np.int64).reshape(-1)
        y = x[0::2] * x[1::2]
        if track:
            self._track_q(x, y)
        return y


class MixedModMultLayer(MultLayer):
    kind = Kind.MMULT
    name = "mixed_mod_mult_layer"

    def __init__(self, in_dims, out_dims=None, smaller_modulus: int = 2):
        super().__init__(in_dims, out_dims)
        self.smaller_modulus = int(smaller_modulus)

    def garble_spec(self):
        return self.kind, {"q": self.smaller_modulus}


class Max(Layer):
    kind = Kind.MAX
    name = "max"

    def __init__(self, in_dims=(2,)):
        super().__init__(in_dims, (1,))

    def plain_eval(self, x, track=True, ctx=None):
        return np.asarray([np.max(x)])

    def plain_q_eval(self, x, track=True, ctx=None, crt_modulus=None):
        return np.asarray([np.max(np.asarray(x, dtype=np.int64))])


class ArgMax(Layer):
    """Index of the largest value along the first axis: (K,) -> (1,) or
    (C, H, W) -> (1, H, W). Ties go to the lowest index (np.argmax; ONNX ArgMax
    with select_last_index = 0). Scale-free, so it works under every
    quantization scheme. Garbled as the max tournament over (value, index)
    candidates with one exact sign per pair (csrc/gadgets.h ArgMaxPlan); the
    output is an ordinary CRT label tensor."""

    kind = Kind.ARGMAX
    name = "argmax"

    def __init__(self, dims):
        dims = tuple(int(d) for d in dims)
        if len(dims) not in (1, 3):
            raise ValueError(f"argmax: the input is (K,) or (C, H, W), got {dims}")
        self.K = dims[0]
        if self.K < 2:
            raise ValueError(f"argmax: needs at least 2 candidates along the first axis, got {self.K}")
        self.P = _size(dims[1:])  # output positions
        super().__init__(dims, (1,) + dims[1:])

    def plain_eval(self, x, track=True, ctx=None):
        y = np.argmax(np.asarray(x).reshape(self.K, self.P), axis=0).astype(np.float32)
        if track:
            self._track_f(y)
        return y

    def plain_q_eval(self, x, track=True, ctx=None, crt_modulus=None):
        v = np.asarray(x, dtype=np.int64).reshape(self.K, self.P)
        y = np.argmax(v, axis=0).astype(np.int64)
        if track:
            # every difference of two candidates of a position may feed a sign: the extreme ones bound them all
            span = v.max(axis=0) - v.min(axis=0)
            self._track_q(y, span, -span)
        return y

    def garble_spec(self):
        return self.kind, {"K": self.K, "P": self.P}


class BaseExtension(Layer):
    """Re-derives the residues of `extra_moduli` from the others (ReDash)."""

    kind = Kind.BASEEXT
    name = "base_extension"

    def __init__(self, dims, extra_moduli: Sequence[int]):
        super().__init__(dims, dims)
        self.extra_moduli = [int(v) for v in extra_moduli]

    def plain_eval(self, x, track=True, ctx=None):
        return np.asarray(x)

    def plain_q_eval(self, x, track=True, ctx=None, crt_modulus=None):
        return np.asarray(x)

    def garble_spec(self):
        return self.kind, {"extra": self.extra_moduli}
