"""ONNX model import/export.

`load_onnx_model(path, q_method, q_parameter)` mirrors the reference loader
(circuit/onnx_modelloader.h:156-406): Flatten / Reshape(flatten), Gemm, Conv,
MaxPool, Relu, Tanh|SignTanh -> Sign, with a Rescale inserted after every
Gemm/Conv for ScaleQuant (legacy `l` halvings) and ScaleQuantPlus (one ReDash
factor), q_const = 0.02 for SimpleQuant. Differences (deliberate):

* the protobuf is decoded by the native wire-format reader (csrc/onnx.cpp), no
  libprotobuf;
* attributes are looked up by name and initializers by the node's input
  names, not by position (the reference's positional access, :280-295, is
  exporter-specific);
* Conv `pads` (symmetric) and `dilations` are honoured, and Conv `auto_pad`
  is resolved from the effective kernel (`VALID`: no pads; `SAME_UPPER` /
  `SAME_LOWER`: accepted when the pads come out symmetric, refused with the
  node's name otherwise); Gemm `transB`/`alpha`/`beta`,
  MatMul+Add, BatchNormalization folding into the preceding Conv/Gemm,
  residual Add of two activations, Identity/Dropout are accepted;
* the import follows the graph: every node's data input is resolved through
  the tensor it names, dims are tracked per tensor, and a layer that does not
  read the previous layer's output gets `in_src` (projection shortcuts, the
  branches of a fire / inception module). `Concat` along the channel axis
  becomes a `Concat` layer; `MaxPool` takes symmetric `pads` and `ceil_mode`.

`Clip` (PyTorch ReLU6 / Hardtanh / clamp) becomes a `Clip` layer: at opset >= 11
its `min` / `max` are inputs 1 and 2, given as initializers or as scalar
`Constant` nodes that feed only Clips; at opset 6 they are attributes. `min = 0`
without a `max` is a `Relu`; any other Clip with a missing or infinite bound is
refused with the node's name, and so is a Clip under SimpleQuant (the bounds
are quantized with the activation scale, which SimpleQuant does not have). A
pending average factor f passes through with the bounds divided by f:
clip(f x, lo, hi) = f clip(x, lo / f, hi / f).

`ArgMax` along axis 1 (the classes of an [N, K] tensor, the channels of NCHW;
or the equivalent negative axis) becomes an `ArgMax` layer. Either `keepdims`
is accepted, since the batch-free dims (1,) / (1, H, W) are the same; any
other axis and `select_last_index = 1` are refused with the node's name. The
index drops a pending (positive) average factor, as a Sign does.

`ConvTranspose` (strides, symmetric pads, output_padding, group = 1) becomes a
`ConvTranspose2d` layer; a pending average factor goes into its weights and a
following BatchNormalization folds along the filter axis (axis 1 of its
[C][F][kh][kw] weights). Dilations, `auto_pad`, `output_shape`, groups and
asymmetric pads are refused with the node's name. `Resize` (opset >= 11) and
`Upsample` (opset <= 9) in mode `nearest` with integer scales [1, 1, fh, fw] (or
`sizes` that are integer multiples of the input), and for Resize
`coordinate_transformation_mode = asymmetric` with `nearest_mode = floor` (what
PyTorch exports for nn.Upsample(mode="nearest")), become an `Upsample` layer;
everything else is refused with the node's name. A pending factor passes through.

With the keyword `resize="bilinear"` a `Resize` (opset >= 11) in mode `linear`
becomes a `Bilinear` layer (docs/BILINEAR.md): `coordinate_transformation_mode`
`half_pixel` (the default), `pytorch_half_pixel` (output sizes above 1, where
both agree), `align_corners` or `asymmetric`; constant `scales` [1, 1, fh, fw]
whose products with the input sizes are whole numbers (the layer's coordinates
are the size ratios; non-integer factors such as 1.5 are fine) or constant
`sizes`. An `Upsample` (opset <= 9) in mode `linear` becomes a `Bilinear` in
mode asymmetric. ScaleQuant only: the output carries by + bx pending scale
bits more than the input. A pending average factor passes through (the map is
linear). Everything else (cubic, a `roi` crop via `tf_crop_and_resize`,
non-constant scales, a batch or channel scale) is refused with the node's name.
The default `resize="nearest"` keeps every `linear` node refused.

`Mul` of two produced tensors becomes a `Mul` layer: equal dims multiply
elementwise, `[N, C, 1, 1]` or `[N, C]` against `[N, C, H, W]` (either order;
the full tensor becomes the layer's input) broadcasts over the plane, and the
same tensor twice is a square, as is `Pow` with the constant scalar exponent 2.
Pending average factors multiply and pass through. The scheme's rescale
follows the layer exactly as after a conv. A `Mul` with an initializer
operand, any other broadcast and any other exponent are refused with the
node's name.

`MatMul` of two produced tensors, and `Gemm` of two produced tensors with
`alpha = 1` and no `C` (its `transA` / `transB` become the flags), becomes a
`MatMul` layer (docs/MATMUL.md) followed by the scheme's rescale, as after a
`Mul`. Operands are rank 2 behind the batch axis: a `Reshape` of a produced
`(C, H, W)` tensor to `(C, H W)` that feeds only such nodes is the same tensor
under new dims (the flat layout already is that matrix), and so is the only
`Reshape` of the node's result, e.g. back to `(C, H, W)`; every other `Reshape`
flattens as before. A `Transpose` that swaps the last two axes and feeds only
such nodes folds into `trans_a` / `trans_b`; any other `Transpose` is refused
with its name. An operand with a pending average factor or pending scale bits
is refused with the node's name. A `MatMul` / `Gemm` with an initializer
operand is a `Dense`, as before.

Heads. An operand of rank 3 behind the batch axis, `(h, a, b)`, is `h` head
slabs of the flat tensor and is accepted where it is such a `Reshape` alias
(e.g. a channel-major `(C, H, W)` tensor viewed as `(h, C / h, H W)`) or a
multi-head `MatMul` result as it stands (also behind a Relu, LeakyRelu, PRelu
or Clip), and the other operand has the same
`h`: the tensor is tracked as dims `(h a, b)` and the layer gets `heads = h`.
A `Transpose` with perm `[0, 1, 3, 2]` folds into the flags; the only `Reshape`
of the `(h, M, N)` result gives `out_dims`. This is what a channel-major
PyTorch attention exports (1x1 convs, `.view(N, h, dh, L)`,
`transpose(-1, -2)`, `matmul`), and it moves no data. Different head counts, a
rank-3 operand that is neither kind, rank above 3 and a `Transpose` that moves
the head axis (token-major exports) are refused with the node's name. The
export writes this form for `heads > 1`.

`ReduceSum` over (2, 3) is the plane `SumPool2d` itself (the exporter writes a
global sum pool that no linear layer follows this way).

Averages. `AveragePool`, `GlobalAveragePool` and `ReduceMean` over (2, 3)
import as a `SumPool2d` plus a *pending factor* 1/K on the tensor. The factor
passes through Relu, MaxPool, Flatten, Identity and Dropout (all commute with a
positive factor), a Sign drops it, and the next Conv / Gemm / MatMul multiplies
it into its **weights** (never its bias) before quantization. A factor that
reaches an Add, a Concat or a graph output has no linear layer to absorb it:
that raises NotImplementedError naming the node. Refused as well, because no
single factor exists: `AveragePool` with pads and `count_include_pad=0`, with
pads and `ceil_mode`, or with a `ceil_mode` that cuts the last window.

`LeakyRelu` (attribute `alpha`, default 0.01) and `PRelu` (a slope initializer:
a scalar, `(C,)`, `(C, 1, 1)` or `(1, C, 1, 1)` against a `(C, H, W)` tensor,
`(C,)` against a dense `(C,)` tensor) become a `LeakyRelu` layer with the dyadic
slope round(alpha 2^s) / 2^s, s = `leaky_bits` (docs/LEAKY_RELU.md). ScaleQuant
only: the layer's output carries a scale 2^s larger than its input, kept per
tensor as *pending scale bits* e next to the pending factor. Relu, MaxPool, sum
and average pooling, Flatten, Upsample, Identity and Dropout pass e through, a
Sign and an ArgMax drop it, and the next Conv / ConvTranspose / Gemm / MatMul
consumes it: its bias is quantized at 2^(2l + e) (`in_scale_bits=e`) and the
`Rescale` behind it is `Rescale(l + e)`. A `Mul` adds its operands' bits and
rescales by l + e. `Add` and `Concat` need equal bits on all operands; a `Clip`
or a graph output with pending bits is refused.

`Sigmoid`, `HardSigmoid` (attributes `alpha` / `beta`, ONNX defaults 0.2 / 0.5)
and, with the keyword `tanh="pwl"`, `Tanh` become a `PiecewiseLinear` layer
(docs/PWL.md) with `pwl_bits` slope bits; the default `tanh="sign"` keeps the
reference's BNN convention (Tanh -> Sign). ScaleQuant only. The layer's input
must carry no pending scale bits and no pending factor (refused with the node's
name); its output carries e = `pwl_bits`, consumed like a LeakyRelu's:

    operator                         pending scale bits e
    LeakyRelu / PRelu                e + leaky_bits
    Sigmoid / HardSigmoid / Tanh     0 required -> pwl_bits
    Relu, pools, Flatten, Upsample   passed through
    Resize linear (resize="bilinear") e + by + bx (the Bilinear layer's fraction bits)
    Slice, Split, Gather, ...        passed through (Gather layers)
    Conv / ConvTranspose / Gemm      consumed: in_scale_bits = e, Rescale(l + e)
    Mul                              e0 + e1 consumed: Rescale(l + e0 + e1)
    Add / Concat                     equal on all operands
    Sign / ArgMax                    dropped
    Clip, graph output               0 required

`Slice` (opset 1 attributes or opset >= 10 inputs, positive steps), `Split`
(equal parts, or `split` as attribute or input; every output its own layer
reading the Split's input), `DepthToSpace` (modes DCR and CRD), `SpaceToDepth`
and `Gather` with initializer indices along one axis (a scalar index drops the
axis) become `Gather` layers (docs/GATHER.md). All act on axes behind the
batch axis and take their parameters from attributes or initializers; anything
else is refused with the node's name. A map that is the identity under
unchanged dims is an alias, not a layer. A Gather is value-preserving: the
pending factor and the pending scale bits pass through. The flat form the
export writes, `Flatten -> Gather(axis=1) -> Reshape`, is read back as one layer
on the Flatten's input with the Reshape's dims as `out_dims`. A `Slice`, `Split`
or `Gather` whose input comes (also through elementwise nodes) from a `Reshape`
that is imported as a Flatten although its target has more than one axis
behind the batch axis is refused by name: its axes are not the tracked ones.

With the keyword `transpose="gather"` a `Transpose` that does not fold into a
MatMul and permutes a produced tensor's own tracked axes with `perm[0] == 0`
becomes a Gather too, and the chain `Reshape -> Transpose -> Reshape` whose
shapes are initializers and whose intermediates have no other consumer
(PyTorch's channel shuffle) becomes one Gather with the composed map. A
Transpose of a Reshape view next to a MatMul is still refused. The default
`transpose="matmul"` keeps every Transpose outside the MatMul fold refused.

`save_onnx_model(path, circuit)` writes a pytorch-style ONNX graph of a float
circuit with a small protobuf encoder (the python `onnx` package is not
available on the target image), so that models built or trained here can be
exchanged with other tools and re-imported.
"""
from __future__ import annotations

import struct
from pathlib import Path
from typing import Optional

import numpy as np

from ..native import native
from .circuit import Circuit
from .layers import (Add, ArgMax, Bilinear, Clip, Concat, Conv2d, ConvTranspose2d, Dense, Flatten, Gather, LeakyRelu, MatMul, MaxPool2d,
                     Mul, PiecewiseLinear, Relu, Rescale, Sign, SumPool2d, Upsample, _as_matrix, _convt_check, _head_matrix,
                     _pool_out, _slice_bounds)
from .quant import QuantizationMethod

DEFAULT_Q_CONST = 0.02  # onnx_modelloader.h:377


def parse_onnx(path_or_bytes) -> dict:
    """Decoded ModelProto as plain python (nodes, initializers, inputs, outputs)."""
    if isinstance(path_or_bytes, (bytes, bytearray)):
        blob = bytes(path_or_bytes)
    else:
        blob = Path(path_or_bytes).read_bytes()
    return native().onnx_parse(blob)


def _input_dims(model: dict, init_names: set) -> tuple:
    inputs = [i for i in model["inputs"] if i["name"] not in init_names]
    assert inputs, "onnx: graph has no data input"
    d = [int(v) for v in inputs[0]["dims"]]
    tf = model["producer_name"] == "tf2onnx"
    if tf and len(d) == 4:  # NHWC
        return (d[3], d[1], d[2])
    if tf and len(d) == 3:
        return (d[0], d[1], d[2])
    if len(d) == 4:  # NCHW
        return (d[1], d[2], d[3])
    if len(d) == 3:
        return (d[0], d[1], d[2])
    if len(d) == 2:
        return (d[1],)
    return (d[0],)


class _Spec:
    """A float layer awaiting quantization (BatchNorm may still fold into it)."""

    def __init__(self, kind: str, **kw):
        self.kind = kind
        self.kw = kw


def _sattr(a: dict, key: str, default: str) -> str:
    """A string attribute (the native reader hands strings over as bytes)."""
    v = a.get(key, default)
    return v.decode() if isinstance(v, (bytes, bytearray)) else str(v)


def _pool_attrs(node) -> tuple:
    """(kernel, strides, symmetric pads, ceil_mode) of a MaxPool / AveragePool node."""
    a, name = node["attrs"], node.get("name") or node["op_type"]
    k = [int(v) for v in a["kernel_shape"]]
    st = [int(v) for v in a.get("strides", [1, 1])]
    pads = [int(v) for v in a.get("pads", [0, 0, 0, 0])]
    if len(k) != 2 or any(int(v) != 1 for v in a.get("dilations", [1, 1])):
        raise NotImplementedError(f"onnx: {name}: only undilated 2-D pooling is supported")
    if pads[0] != pads[2] or pads[1] != pads[3]:
        raise NotImplementedError(f"onnx: {name}: asymmetric pads {pads} are not supported")
    if a.get("auto_pad", "NOTSET") not in ("NOTSET", b"NOTSET"):
        raise NotImplementedError(f"onnx: {name}: auto_pad is not supported")
    return k, st, (pads[0], pads[1]), bool(int(a.get("ceil_mode", 0)))


def create_circuit_from_onnx(model: dict, q_method: QuantizationMethod = QuantizationMethod.SimpleQuant,
                             q_const: float = DEFAULT_Q_CONST, q_parameter: int = -1, leaky_bits: int = 4,
                             tanh: str = "sign", pwl_bits: int = 8, transpose: str = "matmul",
                             resize: str = "nearest") -> Circuit:
    q_method = QuantizationMethod(q_method)
    if resize not in ("nearest", "bilinear"):
        raise ValueError(f"onnx: resize must be 'nearest' or 'bilinear', got {resize!r}")
    if tanh not in ("sign", "pwl"):
        raise ValueError(f"onnx: tanh must be 'sign' or 'pwl', got {tanh!r}")
    if transpose not in ("matmul", "gather"):
        raise ValueError(f"onnx: transpose must be 'matmul' or 'gather', got {transpose!r}")
    inits = {t["name"]: t for t in model["initializers"]}
    tf = model["producer_name"] == "tf2onnx"

    def arr(name: str) -> np.ndarray:
        t = inits[name]
        return np.asarray(t["values"], dtype=np.float32).reshape([int(v) for v in t["dims"]] or [-1])

    specs: list[_Spec] = []
    # per tensor: the spec producing it (-1 = graph input), its dims and the pending average factor (see the
    # module docstring)
    producer: dict[str, int] = {}
    tdims: dict[str, tuple] = {}
    tfac: dict[str, float] = {}
    tbits: dict[str, int] = {}  # pending scale bits e (a LeakyRelu's 2^s, see the module docstring)
    data_inputs = [i["name"] for i in model["inputs"] if i["name"] not in inits]
    producer[data_inputs[0]] = -1
    tdims[data_inputs[0]] = _input_dims(model, set(inits))
    tfac[data_inputs[0]] = 1.0
    tbits[data_inputs[0]] = 0
    alias: dict[str, str] = {}
    first_dense = True
    last_conv_filters = 0
    nodes = model["nodes"]
    skip = set()

    # scalar Constant nodes that feed only the min / max inputs of Clip nodes
    clip_consts: dict[str, float] = {}
    for node in nodes:
        if node["op_type"] != "Constant" or "value" not in node["attrs"]:
            continue
        out, t = node["outputs"][0], node["attrs"]["value"]
        uses = [(n["op_type"], pos) for n in nodes for pos, x in enumerate(n["inputs"]) if x == out]
        vals = np.asarray(t["values"], dtype=np.float64).reshape(-1) if isinstance(t, dict) else np.zeros(0)
        if uses and all(o == "Clip" and pos in (1, 2) for o, pos in uses) and vals.size == 1:
            clip_consts[out] = float(vals[0])

    # scalar Constant nodes that feed only the exponent of Pow nodes
    pow_consts: dict[str, float] = {}
    for node in nodes:
        if node["op_type"] != "Constant" or "value" not in node["attrs"]:
            continue
        out, t = node["outputs"][0], node["attrs"]["value"]
        uses = [(n["op_type"], pos) for n in nodes for pos, x in enumerate(n["inputs"]) if x == out]
        vals = np.asarray(t["values"], dtype=np.float64).reshape(-1) if isinstance(t, dict) else np.zeros(0)
        if uses and all(o == "Pow" and pos == 1 for o, pos in uses) and vals.size == 1:
            pow_consts[out] = float(vals[0])

    # MatMul / Gemm of two produced tensors (no initializer operand): a MatMul layer. Around such a node a Transpose
    # of the last two axes that feeds only such nodes folds into trans_a / trans_b, a Reshape that feeds only such
    # nodes (or such a Transpose) is the same tensor under matrix dims, and so is the only Reshape of its result.
    def uses_of(name: str) -> list:
        return [k for k, n in enumerate(nodes) if name in n["inputs"]]

    secret_mm = {k for k, n in enumerate(nodes) if n["op_type"] in ("MatMul", "Gemm") and len(n["inputs"]) >= 2
                 and n["inputs"][0] not in inits and n["inputs"][1] not in inits}
    fold_tr = set()
    for k, n in enumerate(nodes):
        perm = [int(v) for v in n["attrs"].get("perm", [])] if n["op_type"] == "Transpose" else []
        r = len(perm)
        if r >= 2 and perm == list(range(r - 2)) + [r - 1, r - 2] and uses_of(n["outputs"][0]) and \
                all(u in secret_mm for u in uses_of(n["outputs"][0])):
            fold_tr.add(k)
    mm_feed = {k for k, n in enumerate(nodes) if n["op_type"] == "Reshape" and uses_of(n["outputs"][0])
               and all(u in secret_mm or u in fold_tr for u in uses_of(n["outputs"][0]))}
    mm_back = {k for k, n in enumerate(nodes) if n["op_type"] == "Reshape" and any(
        nodes[m]["outputs"][0] == n["inputs"][0] and uses_of(n["inputs"][0]) == [k] for m in secret_mm)}
    tr_of: dict[str, str] = {}    # a folded Transpose's output -> its input
    vdims: dict[str, tuple] = {}  # a matrix-view Reshape's output -> its dims (the tensor itself is an alias)
    mheads: dict[str, int] = {}   # a multi-head MatMul's result (tracked as dims (h M, N)) -> h

    # Gather layers (docs/GATHER.md). The flat form the export writes, Flatten -> Gather(axis=1) -> Reshape: a
    # Flatten that feeds only such a Gather is the same tensor seen flat, and the only Reshape of the Gather's result
    # gives the layer's out_dims. With transpose="gather", the chain Reshape -> Transpose -> Reshape whose
    # intermediates have no other consumer (PyTorch's channel shuffle) becomes one Gather with the composed map.
    def init_shape(n) -> bool:
        return n["op_type"] == "Reshape" and len(n["inputs"]) > 1 and n["inputs"][1] in inits

    made_by = {n["outputs"][0]: k for k, n in enumerate(nodes) if n["outputs"]}
    gouts = {o["name"] for o in model.get("outputs", [])}  # an intermediate that is a graph output stays a tensor
    flat_feed: set = set()         # Flatten nodes that only feed a flat Gather
    flat_back: dict[int, int] = {}  # flat Gather -> the Reshape behind it
    for k, n in enumerate(nodes):
        m = made_by.get(n["inputs"][0]) if n["op_type"] == "Gather" and len(n["inputs"]) > 1 else None
        if m is not None and int(n["attrs"].get("axis", 0)) == 1 and n["inputs"][1] in inits and \
                nodes[m]["op_type"] == "Flatten" and int(nodes[m]["attrs"].get("axis", 1)) == 1 and \
                uses_of(nodes[m]["outputs"][0]) == [k] and nodes[m]["outputs"][0] not in gouts:
            flat_feed.add(m)
            u = uses_of(n["outputs"][0])
            if len(u) == 1 and init_shape(nodes[u[0]]) and nodes[u[0]]["inputs"][0] == n["outputs"][0] and \
                    n["outputs"][0] not in gouts:
                flat_back[k] = u[0]
    shuffle_chain: dict[int, tuple] = {}  # first Reshape -> (Transpose, second Reshape)
    if transpose == "gather":
        for k, n in enumerate(nodes):
            if not init_shape(n) or k in mm_feed or k in mm_back:
                continue
            u = uses_of(n["outputs"][0])
            if len(u) != 1 or nodes[u[0]]["op_type"] != "Transpose" or u[0] in fold_tr or \
                    n["outputs"][0] in gouts or nodes[u[0]]["outputs"][0] in gouts:
                continue
            u2 = uses_of(nodes[u[0]]["outputs"][0])
            if len(u2) == 1 and init_shape(nodes[u2[0]]) and u2[0] not in mm_feed and u2[0] not in mm_back and \
                    nodes[u2[0]]["inputs"][0] == nodes[u[0]]["outputs"][0]:
                shuffle_chain[k] = (u[0], u2[0])
    fviews: set = set()  # outputs of the flat_feed Flattens: aliases of their (C, H, W) input, read flat
    # A Reshape that is neither next to a MatMul nor part of a chain above is imported as a Flatten. Where its target
    # has more than one axis behind the batch axis (or is not an initializer), the graph's axes no longer are the
    # tracked ones: tensor name -> that Reshape's name, carried through elementwise nodes. An operator that names
    # an axis (Slice, Split, Gather) refuses such an input.
    unflat: dict[str, str] = {}
    elementwise = ("Identity", "Dropout", "Relu", "LeakyRelu", "PRelu", "Clip", "Sigmoid", "HardSigmoid", "Tanh",
                   "SignTanh", "Sign")

    def tracked_axes(node):
        nm = node["inputs"][0]
        if nm in unflat:
            raise NotImplementedError(
                f"onnx: {node.get('name') or node['op_type']}: the input {nm!r} comes from the Reshape "
                f"{unflat[nm]!r}, which is imported flat: a {node['op_type']} along an axis of the reshaped view is "
                "not supported")

    def view_shape(node, size: int, where: str = "next to a MatMul", batch_one: bool = False) -> tuple:
        """The target of a Reshape without its batch axis, 0 and -1 resolved against `size` elements. batch_one: the
        first entry must be the batch axis of one sample (1, 0 = copied, or the shape's only -1)."""
        name = node.get("name") or node["op_type"]
        if len(node["inputs"]) < 2 or node["inputs"][1] not in inits:
            raise NotImplementedError(f"onnx: {name}: the shape of a Reshape {where} must be an initializer")
        shp = [int(v) for v in np.asarray(inits[node["inputs"][1]]["values"]).reshape(-1)]
        if batch_one and (not shp or not (shp[0] in (0, 1) or (shp[0] == -1 and -1 not in shp[1:]))):
            raise NotImplementedError(f"onnx: {name}: a Reshape {where} must keep the batch axis (first entry 1), got "
                                      f"{shp}")
        shp = shp[1:]
        if any(v == 0 for v in shp):
            raise NotImplementedError(f"onnx: {name}: a Reshape {where} must state its dims (no 0 entries)")
        if shp.count(-1) == 1:
            known = int(np.prod([v for v in shp if v != -1], dtype=np.int64))
            shp[shp.index(-1)] = size // max(known, 1)
        if not shp or any(v < 1 for v in shp) or int(np.prod(shp, dtype=np.int64)) != size:
            raise NotImplementedError(f"onnx: {name}: Reshape of {size} elements to {shp}")
        return tuple(shp)

    def res(name: str) -> str:
        return alias.get(name, name)

    def src_of(name: str) -> Optional[int]:
        return producer.get(res(name))

    def data_in(node, name: str) -> tuple:
        """(producing spec, dims, pending factor) of a node's data input."""
        r = res(name)
        if r not in producer:
            raise NotImplementedError(f"onnx: {node.get('name') or node['op_type']}: input {name!r} is produced by "
                                      "an unsupported node")
        return producer[r], tdims[r], tfac[r]

    def bits(name: str) -> int:
        return tbits.get(res(name), 0)

    def emit(spec: _Spec, out_name: str, src: int, dims: tuple, fac: float = 1.0, e: int = 0):
        # a layer that does not read the previous layer's output names its source
        spec.kw["in_src"] = None if src == len(specs) - 1 else src
        specs.append(spec)
        producer[out_name] = len(specs) - 1
        tdims[out_name] = tuple(int(v) for v in dims)
        tfac[out_name] = fac
        tbits[out_name] = int(e)

    def no_factor(node, fac: float):
        if fac != 1.0:
            raise NotImplementedError(
                f"onnx: {node.get('name') or node['op_type']}: an average's 1/K factor reaches this "
                f"{node['op_type']} before a Conv/Gemm could absorb it")

    def same_bits(node, names):
        eb_ = [bits(x) for x in names]
        if len(set(eb_)) > 1:
            raise NotImplementedError(
                f"onnx: {node.get('name') or node['op_type']}: the operands of this {node['op_type']} carry "
                f"different LeakyRelu scales (2^e with e = {eb_}); no Conv/Gemm absorbed them")

    def ints_of(node, pos: int, what: str) -> list:
        """The integers of input `pos`, which must be an initializer."""
        nm = node["inputs"][pos] if len(node["inputs"]) > pos else ""
        if nm not in inits:
            raise NotImplementedError(f"onnx: {node.get('name') or node['op_type']}: {what} must be an initializer")
        t = inits[nm]
        return [int(v) for v in (list(t["ivalues"]) or np.asarray(t["values"]).reshape(-1))]

    def inner_axis(node, axis: int, dims) -> int:
        """An ONNX axis of the [N, ...dims] tensor as an axis of dims; the batch axis is refused."""
        nd = len(dims) + 1
        if tf or not -nd <= axis < nd or axis % nd == 0:
            raise NotImplementedError(f"onnx: {node.get('name') or node['op_type']}: {node['op_type']} along axis "
                                      f"{axis} of a rank-{nd} tensor: only the axes behind the batch axis of an NCHW or "
                                      "[N, K] tensor are supported")
        return axis % nd - 1

    def emit_gather(node, out_name: str, in_name: str, ids, out_dims=None):
        """out = the tensor `in_name` moved by the index map `ids` (shaped as the output, or flat with out_dims):
        a Gather layer, or an alias where the map is the identity under unchanged dims. Value-preserving: the
        pending factor and scale bits pass through."""
        j, dims, fac = data_in(node, in_name)
        ids = np.asarray(ids, dtype=np.int64)
        od = tuple(int(v) for v in (out_dims if out_dims is not None else (ids.shape or (1,))))
        if ids.size == 0:
            raise ValueError(f"onnx: {node.get('name') or node['op_type']}: the result is empty")
        if od == tuple(dims) and np.array_equal(ids.reshape(-1), np.arange(ids.size)):
            alias[out_name] = res(in_name)
            return
        emit(_Spec("gather", dims=tuple(dims), idx=ids.reshape(-1).copy(), out_dims=od), out_name, j, od, fac,
             bits(in_name))

    def ids_of(dims) -> np.ndarray:
        return np.arange(int(np.prod(dims)), dtype=np.int64).reshape(tuple(dims))

    for ni, node in enumerate(nodes):
        if ni in skip:
            continue
        op, a = node["op_type"], node["attrs"]
        ins, outs = node["inputs"], node["outputs"]
        if op in elementwise and ins and ins[0] in unflat:
            unflat[outs[0]] = unflat[ins[0]]
        if op in ("Identity", "Dropout"):
            alias[outs[0]] = res(ins[0])
            continue
        eb = bits(ins[0]) if ins else 0  # the data input's pending scale bits
        if op in ("Relu", "LeakyRelu", "PRelu", "Clip") and ins and res(ins[0]) in mheads:
            mheads[outs[0]] = mheads[res(ins[0])]  # an elementwise activation keeps the heads' slabs
        if ni in shuffle_chain:  # Reshape -> Transpose -> Reshape under transpose="gather": one composed map
            t_, r2 = shuffle_chain[ni]
            tn, name = nodes[t_], nodes[t_].get("name") or "Transpose"
            _, dims, _ = data_in(node, ins[0])
            size = int(np.prod(dims))
            s1 = view_shape(node, size, "in front of a Transpose", True)
            perm = [int(v) for v in tn["attrs"].get("perm", [])]
            if len(perm) != len(s1) + 1 or sorted(perm) != list(range(len(perm))) or perm[0] != 0:
                raise NotImplementedError(f"onnx: {name}: a Transpose with perm {perm} of a tensor of dims "
                                          f"{(1,) + s1}: only a permutation that keeps the batch axis is supported")
            s2 = view_shape(nodes[r2], size, "behind a Transpose", True)
            ids = np.transpose(np.arange(size, dtype=np.int64).reshape(s1), [p - 1 for p in perm[1:]])
            emit_gather(tn, nodes[r2]["outputs"][0], ins[0], ids.reshape(-1), s2)
            skip.update((t_, r2))
        elif op == "Flatten" and ni in flat_feed:
            data_in(node, ins[0])
            alias[outs[0]] = res(ins[0])
            fviews.add(outs[0])
        elif op == "Gather":
            name = node.get("name") or op
            tracked_axes(node)
            flat = ins[0] in fviews
            _, dims, _ = data_in(node, ins[0])
            if len(ins) < 2 or ins[1] not in inits:
                raise NotImplementedError(f"onnx: {name}: the indices of a Gather must be an initializer")
            ishape = [int(v) for v in inits[ins[1]]["dims"]]
            if len(ishape) > 1:
                raise NotImplementedError(f"onnx: {name}: Gather indices of shape {ishape}: only a scalar (the axis is "
                                          "dropped) or a 1-D list along one axis is supported")
            vdim = (int(np.prod(dims)),) if flat else tuple(dims)
            ax = inner_axis(node, int(a.get("axis", 0)), vdim)
            sel = np.asarray(ints_of(node, 1, "the indices of a Gather"), dtype=np.int64)
            if sel.size == 0 or (sel < -vdim[ax]).any() or (sel >= vdim[ax]).any():
                raise ValueError(f"onnx: {name}: Gather indices outside the axis of {vdim[ax]} elements (or none)")
            sel = np.where(sel < 0, sel + vdim[ax], sel)
            ids = np.take(ids_of(vdim), sel if ishape else int(sel[0]), axis=ax)
            if flat:  # the export's form: the map acts on the flat tensor, the Reshape behind it gives out_dims
                od = None
                if ni in flat_back:
                    od = view_shape(nodes[flat_back[ni]], ids.size, "behind a flat Gather", True)
                    skip.add(flat_back[ni])
                emit_gather(node, outs[0], ins[0], ids.reshape(-1), od or (ids.size,))
                if ni in flat_back:
                    alias[nodes[flat_back[ni]]["outputs"][0]] = res(outs[0])
            else:
                emit_gather(node, outs[0], ins[0], ids)
        elif op == "Slice":
            name = node.get("name") or op
            tracked_axes(node)
            _, dims, _ = data_in(node, ins[0])
            if "starts" in a:  # opset 1: attributes
                starts, ends = [int(v) for v in a["starts"]], [int(v) for v in a["ends"]]
                axes = [int(v) for v in a["axes"]] if "axes" in a else list(range(len(starts)))
                steps = [1] * len(starts)
            else:  # opset >= 10: inputs
                starts, ends = ints_of(node, 1, "the starts of a Slice"), ints_of(node, 2, "the ends of a Slice")
                axes = ints_of(node, 3, "the axes of a Slice") if len(ins) > 3 and ins[3] else list(range(len(starts)))
                steps = ints_of(node, 4, "the steps of a Slice") if len(ins) > 4 and ins[4] else [1] * len(starts)
            if not (len(starts) == len(ends) == len(axes) == len(steps)):
                raise ValueError(f"onnx: {name}: Slice starts, ends, axes and steps of different lengths")
            if any(s < 1 for s in steps):
                raise NotImplementedError(f"onnx: {name}: Slice steps {steps}: only positive steps are supported")
            ids = ids_of(dims)
            for s0, e0, ax0, st0 in zip(starts, ends, axes, steps):
                ax = inner_axis(node, ax0, dims)
                lo, hi = _slice_bounds(dims[ax], s0, e0)
                ids = ids[(np.s_[:],) * ax + (np.s_[lo:max(hi, lo):st0],)]
            emit_gather(node, outs[0], ins[0], ids)
        elif op == "Split":
            name = node.get("name") or op
            tracked_axes(node)
            _, dims, _ = data_in(node, ins[0])
            ax = inner_axis(node, int(a.get("axis", 0)), dims)
            if "split" in a:
                parts = [int(v) for v in a["split"]]
            elif len(ins) > 1 and ins[1]:
                parts = ints_of(node, 1, "the split of a Split")
            else:
                n_out = len(outs)
                if dims[ax] % n_out:
                    raise NotImplementedError(f"onnx: {name}: Split of an axis of {dims[ax]} into {n_out} parts: only "
                                              "equal parts (or a given split) are supported")
                parts = [dims[ax] // n_out] * n_out
            if len(parts) != len(outs) or sum(parts) != dims[ax] or any(p < 1 for p in parts):
                raise ValueError(f"onnx: {name}: split {parts} does not cut the axis of {dims[ax]} into {len(outs)} "
                                 "parts")
            ids, lo = ids_of(dims), 0
            for out_name, p in zip(outs, parts):  # every part its own layer, reading the Split's input
                emit_gather(node, out_name, ins[0], ids[(np.s_[:],) * ax + (np.s_[lo:lo + p],)])
                lo += p
        elif op in ("DepthToSpace", "SpaceToDepth"):
            name = node.get("name") or op
            _, dims, _ = data_in(node, ins[0])
            if tf or len(dims) != 3:
                raise NotImplementedError(f"onnx: {name}: {op} of an NCHW image only")
            try:
                if op == "DepthToSpace":
                    probe = Gather.depth_to_space(dims, int(a.get("blocksize", 0)), _sattr(a, "mode", "DCR"))
                else:
                    probe = Gather.space_to_depth(dims, int(a.get("blocksize", 0)))
            except ValueError as ex:
                raise NotImplementedError(f"onnx: {name}: {ex}") from None
            emit_gather(node, outs[0], ins[0], probe.idx, probe.out_dims)
        elif op == "Transpose" and transpose == "gather" and ni not in fold_tr:
            name = node.get("name") or op
            _, dims, _ = data_in(node, ins[0])
            perm = [int(v) for v in a.get("perm", [])] or list(range(len(dims), -1, -1))
            if ins[0] in vdims or ins[0] in fviews or len(perm) != len(dims) + 1 or \
                    sorted(perm) != list(range(len(perm))) or perm[0] != 0:
                raise NotImplementedError(f"onnx: {name}: a Transpose with perm {perm} of a tensor tracked under dims "
                                          f"{(1,) + tuple(dims)}: only a permutation of a produced tensor's own axes that "
                                          "keeps the batch axis becomes a Gather (a Reshape view is no such tensor)")
            emit_gather(node, outs[0], ins[0], np.transpose(ids_of(dims), [p - 1 for p in perm[1:]]))
        elif op == "Reshape" and (ni in mm_feed or ni in mm_back):
            j, dims, fac = data_in(node, ins[0])
            shp = view_shape(node, int(np.prod(dims)))
            alias[outs[0]] = res(ins[0])
            if ni in mm_back:  # the product continues under these dims, e.g. (C, H, W)
                specs[j].kw["out_dims"] = shp
                tdims[res(ins[0])] = shp
                mheads.pop(res(ins[0]), None)
            if ni in mm_feed:
                vdims[outs[0]] = shp
        elif op == "Transpose" and ni in fold_tr:
            data_in(node, ins[0])
            alias[outs[0]] = res(ins[0])
            tr_of[outs[0]] = ins[0]
        elif op == "Transpose":
            raise NotImplementedError(f"onnx: {node.get('name') or op}: a Transpose is supported only where it swaps "
                                      "the last two axes and feeds only a MatMul / Gemm of two produced tensors")
        elif ni in secret_mm:
            name = node.get("name") or op
            if op == "Gemm" and (float(a.get("alpha", 1.0)) != 1.0 or (len(ins) > 2 and ins[2])):
                raise NotImplementedError(f"onnx: {name}: a Gemm of two produced tensors is supported with alpha = 1 "
                                          "and no C only")
            flags, opnd, heads = [], [], []
            for pos, key in ((0, "transA"), (1, "transB")):
                nm, t = ins[pos], bool(int(a.get(key, 0))) if op == "Gemm" else False
                if nm in tr_of:
                    nm, t = tr_of[nm], not t
                j, dims, fac = data_in(node, nm)
                h = 1
                if nm in vdims:
                    # a Reshape alias: (r, c), or (h, a, b) = h head slabs, tracked as dims (h a, b) with heads = h
                    dims = vdims[nm]
                    if len(dims) > 3:
                        raise NotImplementedError(f"onnx: {name}: operand {pos} has dims {tuple(dims)} behind the batch "
                                                  "axis: rank above 3 (more than one axis of heads) is not supported")
                    if len(dims) == 3:
                        h, dims = int(dims[0]), (int(dims[0]) * int(dims[1]), int(dims[2]))
                elif res(nm) in mheads:  # a multi-head MatMul's result as it stands, (h, M, N)
                    h = mheads[res(nm)]
                elif len(dims) > 2:
                    raise NotImplementedError(f"onnx: {name}: operand {pos} has dims {tuple(dims)} behind the batch "
                                              "axis: a batch of more than one matrix per operand (heads) is accepted "
                                              "only as a Reshape alias (h, a, b) or a MatMul result; Reshape a "
                                              "(C, H, W) tensor to (C, H W), or to (h, C / h, H W) for h heads, first")
                heads.append(h)
                if fac != 1.0 or bits(nm):
                    raise NotImplementedError(f"onnx: {name}: operand {pos} carries a pending average factor or pending "
                                              f"scale bits ({fac:g}, 2^{bits(nm)}) that no Conv/Gemm absorbed")
                flags.append(t)
                opnd.append((j, tuple(dims)))
            (jx, dx), (jy, dy) = opnd
            if heads[0] != heads[1]:
                raise NotImplementedError(f"onnx: {name}: the operands have different head counts ({heads[0]} and "
                                          f"{heads[1]}); both must be (h, a, b) with the same h")
            try:
                probe = MatMul(dx, 0, dy, flags[0], flags[1], heads=heads[0])
            except ValueError as ex:
                raise ValueError(f"onnx: {name}: {ex}") from None
            emit(_Spec("matmul", dims=dx, src=jy, src_dims=dy, ta=flags[0], tb=flags[1], out_dims=None, heads=heads[0]),
                 outs[0], jx, probe.out_dims)
            if heads[0] > 1:
                mheads[outs[0]] = heads[0]
        elif op == "Flatten" or op == "Reshape":
            j, dims, fac = data_in(node, ins[0])
            if op == "Reshape" and not (init_shape(node) and int(np.asarray(inits[ins[1]]["values"]).size) == 2):
                unflat[outs[0]] = node.get("name") or op  # imported flat, but the graph goes on under other dims
            if op == "Reshape" and len(dims) == 1:
                alias[outs[0]] = res(ins[0])
                continue
            emit(_Spec("flatten", dims=dims), outs[0], j, (int(np.prod(dims)),), fac, eb)
        elif op in ("Gemm", "MatMul"):
            j, dims, fac = data_in(node, ins[0])
            w = arr(ins[1])
            trans_b = int(a.get("transB", 0)) if op == "Gemm" else 0
            if not trans_b:
                w = w.T  # [in][out] -> [out][in]
            w = w * float(a.get("alpha", 1.0))
            bias = np.zeros(w.shape[0], np.float32)
            if op == "Gemm" and len(ins) > 2 and ins[2]:
                bias = arr(ins[2]).reshape(-1) * float(a.get("beta", 1.0))
            out_name = outs[0]
            if op == "MatMul" and ni + 1 < len(nodes):
                nxt = nodes[ni + 1]
                other = [x for x in nxt["inputs"] if x != out_name]
                if nxt["op_type"] == "Add" and out_name in nxt["inputs"] and other and other[0] in inits:
                    bias = arr(other[0]).reshape(-1)
                    out_name = nxt["outputs"][0]
                    skip.add(ni + 1)
            channel_tf = 0
            if tf and first_dense and last_conv_filters > 0:
                channel_tf = last_conv_filters
            first_dense = False
            if fac != 1.0:  # pending average: into the weights, never the bias
                w = (w * np.float32(fac)).astype(np.float32)
            emit(_Spec("dense", w=w, b=bias, channel_tf=channel_tf, e=eb), out_name, j, (w.shape[0],))
        elif op == "Conv":
            j, dims, fac = data_in(node, ins[0])
            w = arr(ins[1])
            F, Cg, kh, kw = (int(v) for v in w.shape)
            group = int(a.get("group", 1))
            C = Cg * group  # weights are [F][C/group][kh][kw]
            if group < 1 or F % group or (len(dims) == 3 and dims[0] % group):
                raise ValueError(f"onnx: conv group {group} must divide the input channels and the {F} filters")
            name = node.get("name") or op
            dil = [int(v) for v in a.get("dilations", [1, 1])]
            if len(dil) != 2 or min(dil) < 1:
                raise ValueError(f"onnx: {name}: dilations {dil} must be two integers >= 1")
            st = [int(v) for v in a.get("strides", [1, 1])]
            assert len(dims) == 3 and dims[0] == C, f"onnx: conv expects {C} input channels, got dims {dims}"
            ke = [(kh - 1) * dil[0] + 1, (kw - 1) * dil[1] + 1]  # effective kernel
            auto = _sattr(a, "auto_pad", "NOTSET")
            if auto == "NOTSET":
                pads = [int(v) for v in a.get("pads", [0, 0, 0, 0])]
                assert pads[0] == pads[2] and pads[1] == pads[3], "onnx: only symmetric padding is supported"
            elif auto == "VALID":
                pads = [0, 0, 0, 0]
            elif auto in ("SAME_UPPER", "SAME_LOWER"):
                # output ceil(n / s); the total padding that needs is split in halves, the odd one at the end
                # (SAME_UPPER) or at the beginning (SAME_LOWER)
                tot = [max((-(-dims[1 + ax] // st[ax]) - 1) * st[ax] + ke[ax] - dims[1 + ax], 0) for ax in (0, 1)]
                if tot[0] % 2 or tot[1] % 2:
                    raise NotImplementedError(f"onnx: {name}: auto_pad {auto} gives asymmetric pads (total {tot} "
                                              f"over height, width); only symmetric padding is supported")
                pads = [tot[0] // 2, tot[1] // 2, tot[0] // 2, tot[1] // 2]
            else:
                raise NotImplementedError(f"onnx: {name}: auto_pad {auto} is not supported")
            bias = arr(ins[2]).reshape(-1) if len(ins) > 2 and ins[2] else np.zeros(F, np.float32)
            if fac != 1.0:
                w = (w * np.float32(fac)).astype(np.float32)
            H = (dims[1] + 2 * pads[0] - ke[0]) // st[0] + 1
            W = (dims[2] + 2 * pads[1] - ke[1]) // st[1] + 1
            emit(_Spec("conv", w=w, b=bias, dims=dims, stride=st, pads=(pads[0], pads[1]), group=group, dil=dil,
                       e=eb), outs[0], j, (F, H, W))
            last_conv_filters = F
        elif op == "ConvTranspose":
            j, dims, fac = data_in(node, ins[0])
            name = node.get("name") or op
            w = arr(ins[1])  # [C][F/group][kh][kw]
            if w.ndim != 4 or len(dims) != 3:
                raise NotImplementedError(f"onnx: {name}: only 2-D ConvTranspose of an image is supported")
            C, F, kh, kw = (int(v) for v in w.shape)
            if int(a.get("group", 1)) != 1:
                raise NotImplementedError(f"onnx: {name}: ConvTranspose with group != 1 is not supported")
            if any(int(v) != 1 for v in a.get("dilations", [1, 1])):
                raise NotImplementedError(f"onnx: {name}: dilated ConvTranspose is not supported")
            if _sattr(a, "auto_pad", "NOTSET") != "NOTSET":
                raise NotImplementedError(f"onnx: {name}: auto_pad is not supported")
            if "output_shape" in a:
                raise NotImplementedError(f"onnx: {name}: output_shape is not supported (give pads / output_padding)")
            st = [int(v) for v in a.get("strides", [1, 1])]
            pads = [int(v) for v in a.get("pads", [0, 0, 0, 0])]
            opad = [int(v) for v in a.get("output_padding", [0, 0])]
            if pads[0] != pads[2] or pads[1] != pads[3]:
                raise NotImplementedError(f"onnx: {name}: asymmetric pads {pads} are not supported")
            if dims[0] != C:
                raise ValueError(f"onnx: {name}: ConvTranspose expects {C} input channels, got dims {dims}")
            try:
                _convt_check(kh, kw, st[0], st[1], pads[0], pads[1], opad[0], opad[1])
            except ValueError as e:
                raise ValueError(f"onnx: {name}: {e}") from None
            bias = arr(ins[2]).reshape(-1) if len(ins) > 2 and ins[2] else np.zeros(F, np.float32)
            if fac != 1.0:
                w = (w * np.float32(fac)).astype(np.float32)
            OH = (dims[1] - 1) * st[0] - 2 * pads[0] + kh + opad[0]
            OW = (dims[2] - 1) * st[1] - 2 * pads[1] + kw + opad[1]
            emit(_Spec("convt", w=w, b=bias, dims=dims, stride=st, pads=(pads[0], pads[1]), opad=(opad[0], opad[1]),
                       e=eb), outs[0], j, (F, OH, OW))
            last_conv_filters = F
        elif op in ("Resize", "Upsample"):
            j, dims, fac = data_in(node, ins[0])
            name = node.get("name") or op
            if tf or len(dims) != 3:
                raise NotImplementedError(f"onnx: {name}: {op} of an NCHW image only")
            linear = resize == "bilinear" and _sattr(a, "mode", "nearest") == "linear"
            if _sattr(a, "mode", "nearest") != "nearest" and not linear:
                raise NotImplementedError(f"onnx: {name}: {op} mode {_sattr(a, 'mode', 'nearest')!r} is not supported "
                                          + ("(nearest and linear only)" if resize == "bilinear" else "(nearest only)"))
            if op == "Resize":
                if int(model.get("opset", 11)) < 11:
                    raise NotImplementedError(f"onnx: {name}: Resize needs opset >= 11")
                ctm, nm = _sattr(a, "coordinate_transformation_mode", "half_pixel"), \
                    _sattr(a, "nearest_mode", "round_prefer_floor")
                if linear:
                    if ctm not in ("half_pixel", "pytorch_half_pixel", "align_corners", "asymmetric"):
                        raise NotImplementedError(f"onnx: {name}: a linear Resize is supported with "
                                                  "coordinate_transformation_mode half_pixel, pytorch_half_pixel, "
                                                  f"align_corners or asymmetric, got {ctm!r}")
                elif ctm != "asymmetric" or nm != "floor":
                    raise NotImplementedError(f"onnx: {name}: Resize is supported with coordinate_transformation_mode="
                                              f"asymmetric and nearest_mode=floor only, got {ctm!r} / {nm!r}")
                s_in, z_in = (ins[2] if len(ins) > 2 else ""), (ins[3] if len(ins) > 3 else "")
            else:
                s_in, z_in = (ins[1] if len(ins) > 1 else ""), ""
            full = (1,) + tuple(dims)
            lin_size = None  # a linear Resize given by sizes: they need not be multiples of the input
            if s_in and s_in in inits and inits[s_in]["values"].size:
                sc = [float(v) for v in np.asarray(inits[s_in]["values"]).reshape(-1)]
            elif op == "Upsample" and "scales" in a:  # opset 7: an attribute
                sc = [float(v) for v in a["scales"]]
            elif z_in and z_in in inits:
                t = inits[z_in]
                sz = [int(v) for v in (list(t["ivalues"]) or np.asarray(t["values"]).reshape(-1))]
                if linear:
                    if len(sz) != 4 or sz[0] != 1 or sz[1] != dims[0] or min(sz[2:]) < 1:
                        raise NotImplementedError(f"onnx: {name}: sizes {sz} do not keep the batch and channel axes of "
                                                  f"the input {full}")
                    lin_size = (sz[2], sz[3])
                elif len(sz) != 4 or any(z % d for z, d in zip(sz, full)):
                    raise NotImplementedError(f"onnx: {name}: sizes {sz} are no integer multiples of the input {full}")
                sc = [1.0, 1.0, 0.0, 0.0] if lin_size else [z / d for z, d in zip(sz, full)]
            else:
                raise NotImplementedError(f"onnx: {name}: {op} needs constant scales or sizes")
            if linear:
                from fractions import Fraction

                if q_method != QuantizationMethod.ScaleQuant:
                    raise ValueError(f"onnx: {name}: a linear {op} is imported as a Bilinear layer under ScaleQuant only: "
                                     "its output carries a power-of-two scale that the next power-of-two Rescale absorbs")
                if len(sc) != 4 or sc[0] != 1 or sc[1] != 1:
                    raise NotImplementedError(f"onnx: {name}: {op} scales {sc} are not [1, 1, fh, fw]: the batch and "
                                              "channel axes cannot be resized")
                size = lin_size or [Fraction(v) * d for v, d in zip(sc[2:], dims[1:])]
                if any(Fraction(m).denominator != 1 or m < 1 for m in size):
                    raise NotImplementedError(f"onnx: {name}: {op} scales {sc} do not take the input {tuple(dims)} to whole "
                                              "sizes (the layer's coordinates are the size ratios); export with sizes")
                size = tuple(int(m) for m in size)
                mode = "asymmetric" if op == "Upsample" else {"pytorch_half_pixel": "half_pixel"}.get(ctm, ctm)
                if op == "Resize" and ctm == "pytorch_half_pixel" and min(size) <= 1:
                    raise NotImplementedError(f"onnx: {name}: pytorch_half_pixel with an output size of 1 is not supported")
                if size == tuple(dims[1:]):
                    raise NotImplementedError(f"onnx: {name}: {op} scales {sc} leave the size unchanged")
                spec = _Spec("bilinear", dims=dims, size=size, mode=mode)
                # the fraction bits are the tables': build them once here, the layer itself is built from the spec
                probe = Bilinear(dims, size=size, mode=mode)
                emit(spec, outs[0], j, (dims[0],) + size, fac, eb + probe.scale_bits)
                continue
            if len(sc) != 4 or sc[0] != 1 or sc[1] != 1 or any(v != int(v) or v < 1 for v in sc[2:]) or \
                    sc[2] * sc[3] == 1:
                raise NotImplementedError(f"onnx: {name}: {op} scales {sc} are not [1, 1, fh, fw] with integer "
                                          "factors >= 1 (not both 1)")
            fh, fw = int(sc[2]), int(sc[3])
            emit(_Spec("upsample", dims=dims, f=(fh, fw)), outs[0], j, (dims[0], dims[1] * fh, dims[2] * fw), fac, eb)
        elif op == "BatchNormalization":
            j = src_of(ins[0])
            assert j is not None and j >= 0 and specs[j].kind in ("conv", "dense", "convt"), \
                "onnx: BatchNormalization must follow a Conv, ConvTranspose or Gemm"
            scale, shift, mean, var = (arr(n).reshape(-1) for n in ins[1:5])
            eps = float(a.get("epsilon", 1e-5))
            g = scale / np.sqrt(var + eps)
            s = specs[j]
            if s.kind == "convt":  # the filters are axis 1 of [C][F][kh][kw]
                s.kw["w"] = s.kw["w"] * g.reshape(1, -1, 1, 1)
                s.kw["b"] = (s.kw["b"] - mean) * g + shift
                alias[outs[0]] = res(ins[0])
                continue
            s.kw["w"] = s.kw["w"] * g.reshape((-1,) + (1,) * (s.kw["w"].ndim - 1))
            s.kw["b"] = (s.kw["b"] - mean) * g + shift
            alias[outs[0]] = res(ins[0])
        elif op == "MaxPool":
            j, dims, fac = data_in(node, ins[0])
            k, st, pads, ceil = _pool_attrs(node)
            assert len(dims) == 3, f"onnx: MaxPool expects an image, got dims {dims}"
            out = (dims[0], _pool_out(dims[1], k[0], st[0], pads[0], ceil), _pool_out(dims[2], k[1], st[1], pads[1], ceil))
            emit(_Spec("maxpool", dims=dims, k=k, stride=st, pads=pads, ceil=ceil), outs[0], j, out, fac, eb)
        elif op in ("AveragePool", "GlobalAveragePool", "ReduceMean", "ReduceSum"):
            j, dims, fac = data_in(node, ins[0])
            name = node.get("name") or op
            assert len(dims) == 3, f"onnx: {op} expects an image, got dims {dims}"
            flat = False
            if op == "AveragePool":
                k, st, pads, ceil = _pool_attrs(node)
                if any(pads) and not int(a.get("count_include_pad", 0)):
                    raise NotImplementedError(f"onnx: {name}: pads with count_include_pad=0 divide every position "
                                              "by its own tap count")
                if ceil and any(pads):
                    raise NotImplementedError(f"onnx: {name}: ceil_mode with pads is not supported")
                if ceil:
                    # a window cut at the edge divides by its own (smaller) tap count: only a ceil_mode that
                    # cuts no window is a sum with one factor
                    for n_, k_, s_ in ((dims[1], k[0], st[0]), (dims[2], k[1], st[1])):
                        if (_pool_out(n_, k_, s_, 0, True) - 1) * s_ + k_ > n_:
                            raise NotImplementedError(f"onnx: {name}: ceil_mode cuts the last window, whose "
                                                      "divisor differs")
                    ceil = False
            else:
                if op in ("ReduceMean", "ReduceSum"):
                    axes = a.get("axes")
                    if axes is None and len(ins) > 1 and ins[1] in inits:
                        t = inits[ins[1]]  # opset 18: the axes are an int64 input
                        axes = list(t["ivalues"]) or [int(v) for v in np.asarray(t["values"]).reshape(-1)]
                    axes = [axes] if isinstance(axes, int) else (axes or [])
                    axes = sorted(int(v) % 4 for v in axes)
                    if tf or axes != [2, 3]:
                        raise NotImplementedError(f"onnx: {name}: {op} is supported over axes (2, 3) only")
                    flat = not int(a.get("keepdims", 1))
                k, st, pads, ceil = [dims[1], dims[2]], [1, 1], (0, 0), False
            out = (dims[0], _pool_out(dims[1], k[0], st[0], pads[0], ceil), _pool_out(dims[2], k[1], st[1], pads[1], ceil))
            if op != "ReduceSum":  # the plane sum is the SumPool2d itself
                fac = fac / float(k[0] * k[1])
            emit(_Spec("sumpool", dims=dims, k=k, stride=st, pads=pads, ceil=ceil), outs[0], j, out, fac, eb)
            if flat:  # keepdims=0: (C, 1, 1) -> (C,)
                emit(_Spec("flatten", dims=out), outs[0], len(specs) - 1, (out[0],), fac, eb)
        elif op == "Relu":
            j, dims, fac = data_in(node, ins[0])
            emit(_Spec("relu", dims=dims), outs[0], j, dims, fac, eb)
        elif op in ("LeakyRelu", "PRelu"):
            j, dims, fac = data_in(node, ins[0])
            name = node.get("name") or op
            if q_method != QuantizationMethod.ScaleQuant:
                raise ValueError(f"onnx: {name}: a {op} is imported under ScaleQuant only: its output carries a scale "
                                 f"2^{leaky_bits} that the next power-of-two Rescale absorbs (SimpleQuant has no "
                                 "rescale, a ScaleQuantPlus rescale divides by CRT moduli)")
            if op == "LeakyRelu":
                alpha = np.asarray([float(a.get("alpha", 0.01))], np.float32)
            else:
                if len(ins) < 2 or ins[1] not in inits:
                    raise NotImplementedError(f"onnx: {name}: the PRelu slope must be an initializer")
                sl = arr(ins[1])
                shape, C = tuple(int(v) for v in sl.shape), int(dims[0])
                ok = [(C,)] + ([(C, 1, 1), (1, C, 1, 1)] if len(dims) == 3 else [])
                if sl.size != 1 and shape not in ok:
                    raise NotImplementedError(f"onnx: {name}: PRelu slope of shape {shape} against a tensor of dims "
                                              f"{tuple(dims)}: only a scalar or one slope per channel is supported")
                alpha = sl.reshape(-1)
            # leaky(f x) = f leaky(x) for f > 0: the pending factor passes through
            emit(_Spec("leaky", dims=dims, alpha=alpha), outs[0], j, dims, fac, eb + int(leaky_bits))
        elif op == "Constant" and (outs[0] in clip_consts or outs[0] in pow_consts):
            continue
        elif op == "Clip":
            j, dims, fac = data_in(node, ins[0])
            name = node.get("name") or op

            def bound(pos: int, attr: str) -> Optional[float]:
                if attr in a:  # opset 6: attributes
                    return float(a[attr])
                if len(ins) <= pos or not ins[pos]:
                    return None
                if ins[pos] in inits:
                    v = arr(ins[pos]).reshape(-1)
                    if v.size != 1:
                        raise NotImplementedError(f"onnx: {name}: Clip bound {ins[pos]!r} is not a scalar")
                    return float(v[0])
                if ins[pos] in clip_consts:
                    return clip_consts[ins[pos]]
                raise NotImplementedError(f"onnx: {name}: Clip bound {ins[pos]!r} is neither an initializer nor a "
                                          "scalar Constant")

            lo, hi = bound(1, "min"), bound(2, "max")
            # the opset-6 attribute defaults are the float limits: as good as absent
            lo = None if lo is None or not np.isfinite(lo) or lo <= -3.4e38 else lo
            hi = None if hi is None or not np.isfinite(hi) or hi >= 3.4e38 else hi
            if lo == 0.0 and hi is None:
                emit(_Spec("relu", dims=dims), outs[0], j, dims, fac, eb)
            elif lo is None or hi is None:
                raise NotImplementedError(f"onnx: {name}: a Clip needs finite min and max (only min=0 without max "
                                          "is accepted, as a Relu)")
            else:
                if q_method == QuantizationMethod.SimpleQuant:
                    raise ValueError(f"onnx: {name}: a Clip layer cannot be quantized under SimpleQuant (no single "
                                     "activation scale for its bounds); use ScaleQuant or ScaleQuantPlus")
                if not lo < hi:
                    raise ValueError(f"onnx: {name}: Clip needs min < max, got ({lo}, {hi})")
                if eb:
                    raise NotImplementedError(f"onnx: {name}: a LeakyRelu's 2^{eb} scale reaches this Clip before a "
                                              "Conv/Gemm could absorb it")
                # clip(f x, lo, hi) = f clip(x, lo / f, hi / f): the pending factor passes through
                emit(_Spec("clip", dims=dims, lo=lo / fac, hi=hi / fac), outs[0], j, dims, fac)
        elif op == "ArgMax":
            j, dims, fac = data_in(node, ins[0])
            name = node.get("name") or op
            axis, nd = int(a.get("axis", 0)), len(dims) + 1  # dims leave the batch axis out
            if tf or len(dims) not in (1, 3) or axis not in (1, 1 - nd):
                raise NotImplementedError(f"onnx: {name}: ArgMax is supported along axis 1 (the classes of an [N, K] "
                                          f"tensor, the channels of NCHW) only, got axis {axis} of a rank-{nd} tensor")
            if int(a.get("select_last_index", 0)):
                raise NotImplementedError(f"onnx: {name}: ArgMax with select_last_index=1 is not supported (ties go "
                                          "to the lowest index)")
            # keepdims only shapes the output; the index drops a pending positive factor
            emit(_Spec("argmax", dims=dims, keepdims=int(a.get("keepdims", 1))), outs[0], j, (1,) + tuple(dims[1:]))
        elif op in ("Sigmoid", "HardSigmoid") or (op == "Tanh" and tanh == "pwl"):
            j, dims, fac = data_in(node, ins[0])
            name = node.get("name") or op
            if q_method != QuantizationMethod.ScaleQuant:
                raise ValueError(f"onnx: {name}: a {op} is imported as a piecewise-linear layer (pwl) under ScaleQuant "
                                 f"only: its output carries a scale 2^{pwl_bits} that the next power-of-two Rescale "
                                 "absorbs")
            if eb:
                raise NotImplementedError(f"onnx: {name}: a pending 2^{eb} scale reaches this {op} before a Conv/Gemm "
                                          "could absorb it (its breakpoints are quantized at the activation scale)")
            if fac != 1.0:
                raise NotImplementedError(f"onnx: {name}: an average's 1/K factor reaches this {op} before a "
                                          "Conv/Gemm could absorb it")
            fn = {"Sigmoid": "sigmoid", "Tanh": "tanh", "HardSigmoid": "hard_sigmoid"}[op]
            emit(_Spec("pwl", dims=dims, fn=fn, alpha=float(a.get("alpha", 0.2)), beta=float(a.get("beta", 0.5)),
                       name=name), outs[0], j, dims, 1.0, int(pwl_bits))
        elif op in ("Tanh", "SignTanh", "Sign"):
            j, dims, fac = data_in(node, ins[0])
            emit(_Spec("sign", dims=dims), outs[0], j, dims)  # the sign drops a positive factor
        elif op == "Add":
            if any(x in inits for x in ins):
                raise NotImplementedError("onnx: Add of a constant is only supported directly after MatMul")
            (j0, d0, f0), (j1, d1, f1) = data_in(node, ins[0]), data_in(node, ins[1])
            no_factor(node, f0)
            no_factor(node, f1)
            same_bits(node, ins)
            assert d0 == d1, f"onnx: Add operands of different dims {d0} and {d1}"
            if j1 == len(specs) - 1:  # the current tensor is the previous layer's where possible
                j0, j1 = j1, j0
            emit(_Spec("add", dims=d0, src=j1), outs[0], j0, d0, 1.0, eb)
        elif op == "Mul":
            name = node.get("name") or op
            const = [x for x in ins if x in inits]
            if const:
                raise NotImplementedError(f"onnx: {name}: Mul by the constant {const[0]!r} is not supported (only the "
                                          "product of two produced tensors)")
            (j0, d0, f0), (j1, d1, f1) = data_in(node, ins[0]), data_in(node, ins[1])
            if res(ins[0]) == res(ins[1]):
                emit(_Spec("mul", dims=d0, sq=True, e=2 * eb), outs[0], j0, d0, f0 * f0)
            else:
                def chan(full, d):
                    return len(full) == 3 and tuple(d) in ((full[0],), (full[0], 1, 1))

                if tuple(d0) == tuple(d1):
                    if j1 == len(specs) - 1:  # the current tensor is the previous layer's where possible
                        (j0, d0), (j1, d1) = (j1, d1), (j0, d0)
                    sd = None
                elif chan(d0, d1):
                    sd = tuple(d1)
                elif chan(d1, d0):  # the full tensor is the layer's input
                    (j0, d0), (j1, d1) = (j1, d1), (j0, d0)
                    sd = tuple(d1)
                else:
                    raise NotImplementedError(f"onnx: {name}: Mul of dims {tuple(d0)} and {tuple(d1)}: only equal dims "
                                              "and a per-channel operand ([N, C, 1, 1] or [N, C] against "
                                              "[N, C, H, W]) are supported")
                emit(_Spec("mul", dims=d0, sq=False, src=j1, src_dims=sd, e=bits(ins[0]) + bits(ins[1])), outs[0], j0,
                     d0, f0 * f1)
        elif op == "Pow":
            name = node.get("name") or op
            j, dims, fac = data_in(node, ins[0])
            ex = None
            if len(ins) > 1 and ins[1] in inits and arr(ins[1]).size == 1:
                ex = float(arr(ins[1]).reshape(-1)[0])
            elif len(ins) > 1 and ins[1] in pow_consts:
                ex = pow_consts[ins[1]]
            if ex != 2.0:
                raise NotImplementedError(f"onnx: {name}: Pow is supported with the constant scalar exponent 2 only"
                                          + ("" if ex is None else f", got {ex}"))
            emit(_Spec("mul", dims=dims, sq=True, e=2 * eb), outs[0], j, dims, fac * fac)
        elif op == "Concat":
            name = node.get("name") or op
            ops_ = [data_in(node, x) for x in ins]
            axis = int(a.get("axis", 1))
            nd = len(ops_[0][1])
            if tf or nd not in (1, 3) or axis % (nd + 1) != 1:
                raise NotImplementedError(f"onnx: {name}: Concat is supported along the channel axis (axis=1 of "
                                          "NCHW or 2-D tensors) only")
            same_bits(node, ins)
            for _, d_, f_ in ops_:
                no_factor(node, f_)
                if len(d_) != nd or d_[1:] != ops_[0][1][1:]:
                    raise ValueError(f"onnx: {name}: Concat operands of different H x W")
            dl = [d_ for _, d_, _ in ops_]
            out = (sum(d_[0] for d_ in dl),) + tuple(dl[0][1:])
            emit(_Spec("concat", dims_list=dl, srcs=[j_ for j_, _, _ in ops_]), outs[0], len(specs) - 1, out, 1.0, eb)
        else:
            raise NotImplementedError(f"onnx: unsupported operator {op}")

    for o in model.get("outputs", []):
        r = res(o["name"])
        if r in tfac and tfac[r] != 1.0:
            raise NotImplementedError(f"onnx: graph output {o['name']!r} carries an average's 1/K factor that no "
                                      "Conv/Gemm absorbs")
        if tbits.get(r, 0):
            raise NotImplementedError(f"onnx: graph output {o['name']!r} carries a LeakyRelu's 2^{tbits[r]} scale that "
                                      "no Conv/Gemm absorbs")

    # materialize: quantize weights, insert rescales, remap spec indices -> layer indices
    layers = []
    spec_to_layer: dict[int, int] = {-1: -1}
    for i, s in enumerate(specs):
        kw = s.kw
        if s.kind == "flatten":
            layers.append(Flatten(kw["dims"]))
        elif s.kind == "dense":
            layers.append(Dense(kw["w"], kw["b"], q_parameter, q_method, q_const, channel_tf=kw["channel_tf"],
                                in_scale_bits=kw["e"]))
        elif s.kind == "conv":
            C, H, W = kw["dims"]
            F, _, kh, kw_ = kw["w"].shape
            layers.append(Conv2d(kw["w"], kw["b"], W, H, C, F, kw_, kh, kw["stride"][1], kw["stride"][0],
                                 q_parameter, q_method, q_const, pad_width=kw["pads"][1], pad_height=kw["pads"][0],
                                 groups=kw["group"], dilation_width=kw["dil"][1], dilation_height=kw["dil"][0],
                                 in_scale_bits=kw["e"]))
        elif s.kind == "convt":
            C, H, W = kw["dims"]
            _, F, kh, kw_ = kw["w"].shape
            layers.append(ConvTranspose2d(kw["w"], kw["b"], W, H, C, F, kw_, kh, kw["stride"][1], kw["stride"][0],
                                          q_parameter, q_method, q_const, pad_width=kw["pads"][1],
                                          pad_height=kw["pads"][0], out_pad_width=kw["opad"][1],
                                          out_pad_height=kw["opad"][0], in_scale_bits=kw["e"]))
        elif s.kind == "upsample":
            layers.append(Upsample(kw["dims"], kw["f"][0], kw["f"][1]))
        elif s.kind == "bilinear":
            layers.append(Bilinear(kw["dims"], size=kw["size"], mode=kw["mode"]))
        elif s.kind == "gather":
            layers.append(Gather(kw["dims"], kw["idx"], kw["out_dims"]))
        elif s.kind in ("maxpool", "sumpool"):
            C, H, W = kw["dims"]
            cls = MaxPool2d if s.kind == "maxpool" else SumPool2d
            layers.append(cls(W, H, C, kw["k"][1], kw["k"][0], kw["stride"][1], kw["stride"][0],
                              pad_width=kw["pads"][1], pad_height=kw["pads"][0], ceil_mode=kw["ceil"]))
        elif s.kind == "relu":
            layers.append(Relu(kw["dims"]))
        elif s.kind == "leaky":
            al = kw["alpha"]
            try:
                layers.append(LeakyRelu(kw["dims"], al if al.size > 1 else float(al[0]), leaky_bits))
            except ValueError as ex:
                raise ValueError(f"onnx: {ex}") from None
        elif s.kind == "pwl":
            try:
                if kw["fn"] == "hard_sigmoid":
                    layers.append(PiecewiseLinear.hard_sigmoid(kw["dims"], kw["alpha"], kw["beta"], pwl_bits,
                                                               q_parameter, q_method))
                else:
                    layers.append(getattr(PiecewiseLinear, kw["fn"])(kw["dims"], pwl_bits, q_parameter, q_method))
            except ValueError as ex:
                raise ValueError(f"onnx: {kw['name']}: {ex}") from None
        elif s.kind == "sign":
            layers.append(Sign(kw["dims"]))
        elif s.kind == "clip":
            layers.append(Clip(kw["dims"], kw["lo"], kw["hi"], q_parameter, q_method))
        elif s.kind == "argmax":
            layers.append(ArgMax(kw["dims"]))
        elif s.kind == "add":
            layers.append(Add(kw["dims"], spec_to_layer[kw["src"]]))
        elif s.kind == "concat":
            layers.append(Concat(kw["dims_list"], [spec_to_layer[j] for j in kw["srcs"]]))
        elif s.kind == "mul":
            layers.append(Mul.square(kw["dims"]) if kw["sq"] else
                          Mul(kw["dims"], spec_to_layer[kw["src"]], kw["src_dims"]))
        elif s.kind == "matmul":
            layers.append(MatMul(kw["dims"], spec_to_layer[kw["src"]], kw["src_dims"], kw["ta"], kw["tb"],
                                 kw["out_dims"], heads=kw["heads"]))
        if kw.get("in_src") is not None:
            layers[-1].in_src = spec_to_layer[kw["in_src"]]
        spec_to_layer[i] = len(layers) - 1
        if s.kind in ("dense", "conv", "convt", "mul", "matmul"):  # a product carries both operands' scales, as a conv's does
            out = layers[-1].out_dims
            if q_method == QuantizationMethod.ScaleQuant:  # + the input's pending scale bits
                layers.append(Rescale(q_parameter + kw.get("e", 0), out))
                spec_to_layer[i] = len(layers) - 1
            elif q_method == QuantizationMethod.ScaleQuantPlus:
                layers.append(Rescale([q_parameter], out))
                spec_to_layer[i] = len(layers) - 1
    return Circuit(layers, q_parameter)


def load_onnx_model(path, q_method: QuantizationMethod = QuantizationMethod.SimpleQuant, q_parameter: int = -1,
                    q_const: float = DEFAULT_Q_CONST, leaky_bits: int = 4, tanh: str = "sign",
                    pwl_bits: int = 8, transpose: str = "matmul", resize: str = "nearest") -> Circuit:
    """Reference: load_onnx_model (onnx_modelloader.h:371-406). leaky_bits: the slope bits of imported LeakyRelu /
    PRelu nodes (docs/LEAKY_RELU.md). tanh: "sign" imports Tanh as Sign (the reference's convention), "pwl" as a
    PiecewiseLinear; pwl_bits: the slope bits of imported Sigmoid / HardSigmoid / Tanh nodes (docs/PWL.md).
    transpose: "matmul" accepts a Transpose only where it folds into a MatMul, "gather" also turns every other
    Transpose that keeps the batch axis into a Gather layer (docs/GATHER.md). resize: "nearest" accepts a Resize /
    Upsample in mode nearest only, "bilinear" also imports mode linear as a Bilinear layer (docs/BILINEAR.md)."""
    return create_circuit_from_onnx(parse_onnx(path), q_method, q_const, q_parameter, leaky_bits, tanh, pwl_bits,
                                    transpose, resize)


# ------------------------------------------------------------------ export
def _varint(v: int) -> bytes:
    v &= (1 << 64) - 1
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _key(field: int, wt: int) -> bytes:
    return _varint((field << 3) | wt)


def _ld(field: int, payload: bytes) -> bytes:
    return _key(field, 2) + _varint(len(payload)) + payload


def _s(field: int, s: str) -> bytes:
    return _ld(field, s.encode())


def _i(field: int, v: int) -> bytes:
    return _key(field, 0) + _varint(v)


def _tensor(name: str, a: np.ndarray) -> bytes:
    a = np.ascontiguousarray(a, dtype=np.float32)
    body = b"".join(_i(1, d) for d in a.shape) + _i(2, 1) + _s(8, name) + _ld(9, a.tobytes())
    return body


def _tensor_i64(name: str, vals) -> bytes:
    a = np.ascontiguousarray(vals, dtype=np.int64)
    return b"".join(_i(1, d) for d in a.shape) + _i(2, 7) + _s(8, name) + _ld(9, a.tobytes())


def _attr_ints(name: str, vals) -> bytes:
    return _ld(5, _s(1, name) + b"".join(_i(8, int(v)) for v in vals) + _i(20, 7))


def _attr_int(name: str, v: int) -> bytes:
    return _ld(5, _s(1, name) + _i(3, int(v)) + _i(20, 2))


def _attr_str(name: str, v: str) -> bytes:
    return _ld(5, _s(1, name) + _ld(4, v.encode()) + _i(20, 3))


def _attr_float(name: str, v: float) -> bytes:
    return _ld(5, _s(1, name) + _key(2, 5) + struct.pack("<f", v) + _i(20, 1))


def _node(op: str, ins, outs, name: str, attrs: bytes = b"") -> bytes:
    return _ld(1, b"".join(_s(1, x) for x in ins) + b"".join(_s(2, x) for x in outs) + _s(3, name) + _s(4, op) + attrs)


def _value_info(name: str, dims) -> bytes:
    shape = b"".join(_ld(1, _i(1, int(d))) for d in dims)
    # ValueInfoProto{name, type: TypeProto{tensor_type: {elem_type FLOAT, shape}}}
    return _s(1, name) + _ld(2, _ld(1, _i(1, 1) + _ld(2, shape)))


def save_onnx_model(path, circuit: Circuit, producer: str = "dash_amd") -> None:
    """Write the float weights of `circuit` as an ONNX (opset 13) graph in the
    layout pytorch's exporter uses (NCHW input, Gemm with transB=1). Tensors
    are named by layer index, so `in_src`, `Add.src` and `Concat.srcs` become
    real edges. Rescale layers are quantization artefacts and are dropped;
    loading the file back with the same q_method re-inserts them. A SumPool2d
    is written as an average (AveragePool / GlobalAveragePool) and the next
    linear layer's weights are multiplied by its window size K: the inverse of
    the import fold."""
    nodes, inits = [], []
    names = {-1: "input"}  # layer index -> name of the tensor holding its output
    scale = {"input": 1}  # pending sum/average ratio K of a tensor (SumPool2d written as an average)
    for i, l in enumerate(circuit.layers):
        out = f"t{i}"
        name = f"{l.name}_{i}"
        src = getattr(l, "in_src", None)
        cur = names[src if src is not None else i - 1]
        K = scale[cur]
        if isinstance(l, Rescale):
            names[i] = cur
            continue
        if isinstance(l, (Add, Concat)):
            operands = [cur, names[l.src]] if isinstance(l, Add) else [names[s] for s in l.srcs]
            if any(scale[o] != 1 for o in operands):
                raise NotImplementedError(f"onnx export: the average before layer {i} ({l.name}) has no linear layer "
                                          "to fold its window size into")
        scale[out] = 1
        if isinstance(l, Flatten):
            nodes.append(_node("Flatten", [cur], [out], name, _attr_int("axis", 1)))
            scale[out] = K
        elif isinstance(l, Dense):
            assert l.channel_tf == 0, "onnx export: TF channel order is not representable"
            inits += [_tensor(f"{name}.weight", l.weights * np.float32(K)), _tensor(f"{name}.bias", l.biases)]
            nodes.append(_node("Gemm", [cur, f"{name}.weight", f"{name}.bias"], [out], name,
                               _attr_float("alpha", 1.0) + _attr_float("beta", 1.0) + _attr_int("transB", 1)))
        elif isinstance(l, Conv2d):
            inits += [_tensor(f"{name}.weight", l.weights * np.float32(K)), _tensor(f"{name}.bias", l.biases)]
            attrs = (_attr_ints("dilations", [l.dh, l.dw]) + _attr_int("group", l.groups) + _attr_ints("kernel_shape", [l.kh, l.kw])
                     + _attr_ints("pads", [l.ph, l.pw, l.ph, l.pw]) + _attr_ints("strides", [l.sh, l.sw]))
            nodes.append(_node("Conv", [cur, f"{name}.weight", f"{name}.bias"], [out], name, attrs))
        elif isinstance(l, ConvTranspose2d):
            inits += [_tensor(f"{name}.weight", l.weights * np.float32(K)), _tensor(f"{name}.bias", l.biases)]
            attrs = (_attr_ints("dilations", [1, 1]) + _attr_int("group", 1) + _attr_ints("kernel_shape", [l.kh, l.kw])
                     + _attr_ints("output_padding", [l.oph, l.opw]) + _attr_ints("pads", [l.ph, l.pw, l.ph, l.pw])
                     + _attr_ints("strides", [l.sh, l.sw]))
            nodes.append(_node("ConvTranspose", [cur, f"{name}.weight", f"{name}.bias"], [out], name, attrs))
        elif isinstance(l, Upsample):
            # what PyTorch writes for nn.Upsample(mode="nearest"): Resize with an empty roi and constant scales
            inits.append(_tensor(f"{name}.scales", np.asarray([1, 1, l.fh, l.fw], np.float32)))
            attrs = (_attr_str("coordinate_transformation_mode", "asymmetric") + _attr_str("mode", "nearest")
                     + _attr_str("nearest_mode", "floor"))
            nodes.append(_node("Resize", [cur, "", f"{name}.scales"], [out], name, attrs))
            scale[out] = K
        elif isinstance(l, Bilinear):
            # what PyTorch writes for F.interpolate(size=..., mode="bilinear"): Resize with an empty roi, no scales
            # and constant sizes; linear, so a pending average ratio passes through
            inits.append(_tensor_i64(f"{name}.sizes", (1, l.C, l.OH, l.OW)))
            attrs = _attr_str("coordinate_transformation_mode", l.mode) + _attr_str("mode", "linear")
            nodes.append(_node("Resize", [cur, "", "", f"{name}.sizes"], [out], name, attrs))
            scale[out] = K
        elif isinstance(l, Gather):
            # the map on the flat tensor: Flatten -> Gather(axis=1) -> Reshape(out_dims); value-preserving, so a
            # pending average ratio passes through
            inits.append(_tensor_i64(f"{name}.indices", l.idx))
            nodes.append(_node("Flatten", [cur], [f"{name}.flat"], f"{name}.flatten", _attr_int("axis", 1)))
            if len(l.out_dims) == 1:
                nodes.append(_node("Gather", [f"{name}.flat", f"{name}.indices"], [out], name, _attr_int("axis", 1)))
            else:
                inits.append(_tensor_i64(f"{name}.shape", (1,) + l.out_dims))
                nodes.append(_node("Gather", [f"{name}.flat", f"{name}.indices"], [f"{name}.g"], name,
                                   _attr_int("axis", 1)))
                nodes.append(_node("Reshape", [f"{name}.g", f"{name}.shape"], [out], f"{name}.reshape"))
            scale[out] = K
        elif isinstance(l, MaxPool2d):
            attrs = _attr_ints("kernel_shape", [l.kh, l.kw]) + _attr_ints("pads", [l.ph, l.pw, l.ph, l.pw]) + \
                _attr_ints("strides", [l.sh, l.sw])
            if l.ceil_mode:
                attrs += _attr_int("ceil_mode", 1)
            nodes.append(_node("MaxPool", [cur], [out], name, attrs))
            scale[out] = K
        elif isinstance(l, SumPool2d):
            if l.ceil_mode and ((l.OH - 1) * l.sh + l.kh > l.H + l.ph or (l.OW - 1) * l.sw + l.kw > l.W + l.pw):
                raise NotImplementedError(f"onnx export: layer {i}: a ceil-mode sum pool whose last window is cut "
                                          "is no average with one divisor")
            plane = (l.kh, l.kw) == (l.H, l.W) and not l.padded
            if plane and not any(isinstance(m, (Conv2d, Dense)) for m in circuit.layers[i + 1:]):
                # no later linear layer could absorb an average's K (a classifier conv + global pool head):
                # the plane sum itself
                inits.append(_tensor_i64(f"{name}.axes", [2, 3]))
                nodes.append(_node("ReduceSum", [cur, f"{name}.axes"], [out], name, _attr_int("keepdims", 1)))
                names[i] = out
                scale[out] = K
                continue
            if plane:
                nodes.append(_node("GlobalAveragePool", [cur], [out], name))
            else:
                attrs = _attr_ints("kernel_shape", [l.kh, l.kw]) + _attr_ints("pads", [l.ph, l.pw, l.ph, l.pw]) + \
                    _attr_ints("strides", [l.sh, l.sw])
                if l.ph or l.pw:
                    attrs += _attr_int("count_include_pad", 1)
                nodes.append(_node("AveragePool", [cur], [out], name, attrs))
            scale[out] = K * l.kh * l.kw
        elif isinstance(l, Relu):
            nodes.append(_node("Relu", [cur], [out], name))
            scale[out] = K
        elif isinstance(l, LeakyRelu):  # positive-homogeneous: a pending average ratio passes through
            if l.alpha.size == 1:
                nodes.append(_node("LeakyRelu", [cur], [out], name, _attr_float("alpha", float(l.alpha[0]))))
            else:
                shape = (l.alpha.size, 1, 1) if len(l.in_dims) == 3 else (l.alpha.size,)
                inits.append(_tensor(f"{name}.slope", l.alpha.reshape(shape)))
                nodes.append(_node("PRelu", [cur, f"{name}.slope"], [out], name))
            scale[out] = K
        elif isinstance(l, Clip):
            # opset-11 form: min / max are scalar inputs; on an average the bounds of the sum shrink by K
            inits += [_tensor(f"{name}.min", np.float32(l.lo / K)), _tensor(f"{name}.max", np.float32(l.hi / K))]
            nodes.append(_node("Clip", [cur, f"{name}.min", f"{name}.max"], [out], name))
            scale[out] = K
        elif isinstance(l, PiecewiseLinear):
            if K != 1:
                raise NotImplementedError(f"onnx export: the average before layer {i} ({l.name}) has no linear layer "
                                          "to fold its window size into")
            if l.fn == "sigmoid":
                nodes.append(_node("Sigmoid", [cur], [out], name))
            elif l.fn == "tanh":
                nodes.append(_node("Tanh", [cur], [out], name))
            elif l.fn == "hard_sigmoid":
                nodes.append(_node("HardSigmoid", [cur], [out], name, _attr_float("alpha", l.fn_params["alpha"])
                                   + _attr_float("beta", l.fn_params["beta"])))
            else:
                raise NotImplementedError(f"onnx export: layer {i} ({l.name}) is an untagged piecewise-linear function "
                                          "with no ONNX operator; only the sigmoid, tanh and hard_sigmoid "
                                          "constructors are exported")
        elif isinstance(l, Sign):
            nodes.append(_node("Sign", [cur], [out], name))
        elif isinstance(l, ArgMax):  # scale-free: a pending average ratio ends here
            nodes.append(_node("ArgMax", [cur], [out], name, _attr_int("axis", 1) + _attr_int("keepdims", 1)))
        elif isinstance(l, Add):
            nodes.append(_node("Add", [cur, names[l.src]], [out], name))
        elif isinstance(l, Mul):  # the operands' pending average ratios multiply
            other = cur if l.is_square else names[l.src]
            nodes.append(_node("Mul", [cur, other], [out], name))
            scale[out] = K * scale[other]
        elif isinstance(l, MatMul):
            # Reshape (where the tensor is no matrix yet) / Transpose / MatMul, and a Reshape of the result where the
            # layer continues under other dims: what the importer folds back into one layer
            if K != 1 or scale[names[l.src]] != 1:
                raise NotImplementedError(f"onnx export: the average before layer {i} ({l.name}) has no linear layer "
                                          "to fold its window size into")
            # With heads the operands are reshaped to (1, h, a, b), the Transpose swaps the last two of four axes and
            # the rank-4 result is always reshaped to the layer's out_dims.
            opnds = []
            G = l.heads
            for tag, tname, d_, tr in (("a", cur, l.in_dims, l.trans_a), ("b", names[l.src], l.src_dims, l.trans_b)):
                if len(d_) != 2 or G > 1:
                    shp = (1, G) + _head_matrix(d_, G) if G > 1 else (1,) + _as_matrix(d_)
                    inits.append(_tensor_i64(f"{name}.{tag}.shape", shp))
                    nodes.append(_node("Reshape", [tname, f"{name}.{tag}.shape"], [f"{name}.{tag}.m"], f"{name}.{tag}.reshape"))
                    tname = f"{name}.{tag}.m"
                if tr:
                    nodes.append(_node("Transpose", [tname], [f"{name}.{tag}.t"], f"{name}.{tag}.transpose",
                                       _attr_ints("perm", [0, 1, 3, 2] if G > 1 else [0, 2, 1])))
                    tname = f"{name}.{tag}.t"
                opnds.append(tname)
            if G == 1 and l.out_dims == (l.M, l.N):
                nodes.append(_node("MatMul", opnds, [out], name))
            else:
                inits.append(_tensor_i64(f"{name}.shape", (1,) + l.out_dims))
                nodes.append(_node("MatMul", opnds, [f"{name}.mm"], name))
                nodes.append(_node("Reshape", [f"{name}.mm", f"{name}.shape"], [out], f"{name}.reshape"))
        elif isinstance(l, Concat):
            nodes.append(_node("Concat", [names[s] for s in l.srcs], [out], name, _attr_int("axis", 1)))
        else:
            raise NotImplementedError(f"onnx export: layer {l.name} has no ONNX equivalent")
        names[i] = out
    last = names[len(circuit.layers) - 1]
    if scale[last] != 1:
        raise NotImplementedError("onnx export: the circuit ends in an average with no linear layer to fold its "
                                  "window size into")
    dims = (1,) + tuple(circuit.input_dims)
    graph = b"".join(nodes) + _s(2, "dash_amd") + b"".join(_ld(5, t) for t in inits)
    graph += _ld(11, _value_info("input", dims))
    graph += _ld(12, _value_info(last, (1,) + tuple(circuit.output_dims)))
    model = _i(1, 7) + _s(2, producer) + _s(3, "1") + _ld(7, graph) + _ld(8, _s(1, "") + _i(2, 13))
    Path(path).write_bytes(model)
