"""The shape table of the dilated convolution suites (docs/DILATED_CONV.md), shared by tests/test_dilated_conv.py
(host, CPU) and tests/test_gpu_dilated_conv.py (GPU), with the layer / circuit builders and launch_conv's form pick
restated from the planner bindings.

A shape is (W, H, C, F, kh, kw, sw, sh, pw, ph, dw, dh, groups); each is the smallest that exercises one thing."""
import numpy as np

import dash_amd as d

SHAPES = {
    "d2_same": (7, 6, 4, 5, 3, 3, 1, 1, 2, 2, 2, 2, 1),             # "same"-size atrous 3x3, halo of 2
    "d2_valid_rgb": (7, 7, 3, 4, 3, 3, 1, 1, 0, 0, 2, 2, 1),        # no padding, few channels: the tap-unrolled view
    "unequal": (9, 8, 5, 3, 3, 2, 2, 1, 1, 0, 1, 3, 1),             # dh != dw, non-square kernel, unequal strides
    "d2_s2": (9, 9, 4, 4, 3, 3, 2, 2, 2, 2, 2, 2, 1),               # stride and dilation together
    "all_pad_but_centre": (3, 3, 2, 2, 3, 3, 1, 1, 3, 3, 3, 3, 1),  # every off-centre tap lies in the padding
    "k1_d2": (5, 4, 4, 4, 1, 1, 1, 1, 0, 0, 2, 2, 1),               # moot dilation: the plain conv
    # (column stride 2: at unit stride the planner unrolls the taps of a 70-channel 3x3, 10 k-steps instead of 18)
    "c70_f20": (5, 5, 70, 20, 3, 3, 2, 1, 2, 2, 2, 2, 1),           # two channel chunks, partial filter block, streamed A
    "c64_k3": (6, 6, 64, 2, 3, 3, 1, 1, 2, 2, 2, 2, 1),             # 9 k-steps, A in registers
    "c64_k2_d3": (6, 5, 64, 2, 2, 2, 1, 1, 0, 0, 3, 3, 1),          # 4 k-steps
    "two_bands_c64": (32, 20, 64, 2, 3, 3, 1, 1, 2, 2, 2, 2, 1),    # the dilated halo crosses a band edge
    "dw_d2": (7, 6, 6, 6, 3, 3, 1, 1, 2, 2, 2, 2, 6),               # depthwise, dilated
    "grp2_d2_s2": (9, 8, 4, 6, 3, 3, 2, 2, 2, 2, 2, 2, 2),          # two groups, stride 2
    "grp_k2x5_d3": (16, 5, 4, 4, 2, 5, 1, 1, 0, 0, 3, 1, 2),        # more than four taps per row, runtime-tap instance
    "dw_two_bands": (36, 40, 2, 2, 3, 3, 1, 1, 2, 2, 2, 2, 2),      # grouped kernel with several row bands
    # the remaining dilated instantiation of k_conv_img2
    "ur0_c20": (7, 6, 20, 3, 3, 3, 1, 1, 2, 2, 2, 2, 1),            # unrolled view of 180 patch bytes: three k-steps
}
DENSE = [n for n, s in SHAPES.items() if s[12] == 1]
GROUPED = [n for n, s in SHAPES.items() if s[12] > 1]
B3 = [5, 7, 131]


def undilated(shape):
    """The row with both dilations set to 1 (the pads stay: the output grows)."""
    return shape[:10] + (1, 1) + shape[12:]


def weights(rng, shape):
    """Weights with zeros and multiples of 2, 3, 5 and 7 (zero mod a CRT prime: the Z_p term of the reference
    encoding), as tests/test_grouped_conv.py builds them."""
    W, H, C, F, kh, kw, sw, sh, pw, ph, dw, dh, g = shape
    w = rng.integers(-6, 7, (F, C // g, kh, kw))
    flat = w.reshape(-1)
    flat[::5] = 0
    flat[1::7] = 2 * 3 * 5
    flat[2::11] = -6
    flat[3::13] = 10
    flat[4::17] = 7
    return w, rng.integers(-9, 10, F)


def conv_layer(rng, shape, w=None, b=None):
    W, H, C, F, kh, kw, sw, sh, pw, ph, dw, dh, g = shape
    if w is None:
        w, b = weights(rng, shape)
    return d.Conv2d.from_quantized(w, b, W, H, C, F, kw, kh, sw, sh, pad_width=pw, pad_height=ph, groups=g,
                                   dilation_width=dw, dilation_height=dh)


def conv_rescale_relu(rng, shape, l=2):
    cv = conv_layer(rng, shape)
    return d.Circuit([cv, d.Rescale(l, cv.out_dims), d.Relu(cv.out_dims)])


def torch_conv(x, l, dtype=None):
    import torch

    dtype = dtype or torch.float64
    y = torch.nn.functional.conv2d(
        torch.tensor(np.asarray(x).reshape(1, l.C, l.H, l.W), dtype=dtype), torch.tensor(np.asarray(l.q_weights), dtype=dtype),
        torch.tensor(np.asarray(l.q_biases), dtype=dtype), stride=(l.sh, l.sw), padding=(l.ph, l.pw),
        dilation=(l.dh, l.dw), groups=l.groups)
    return y.numpy().reshape(-1)


def plan_of(native, shape, crt, mfma=True):
    """The planner binding of the row: hip_conv_plan (dense) or hip_conv_grp_plan (grouped)."""
    W, H, C, F, kh, kw, sw, sh, pw, ph, dw, dh, g = shape
    if g > 1:
        return native.hip_conv_grp_plan(C, H, W, F, kh, kw, sh, sw, ph, pw, g, crt, dh=dh, dw=dw)
    return native.hip_conv_plan(C, H, W, F, kh, kw, sh, sw, ph, pw, crt, mfma, dh=dh, dw=dw)


def form_of(shape, plan, mfma=True):
    """launch_conv's pick, restated (kernels_gemm.hip): the dilated forms carry a `d` behind the kernel's name."""
    W, H, C, F, kh, kw, sw, sh, pw, ph, dw, dh, g = shape
    dd = "d" if plan["dil"] else ""
    if g > 1:
        if (kh, kw) == (3, 3) and sw in (1, 2):
            return "conv.grp%s<3,3,%d>" % (dd, sw)
        if (kh, kw, sw) == (1, 1, 1) and not plan["dil"]:
            return "conv.grp<1,1,1>"
        return "conv.grp%s<0,0,0>" % dd
    if not mfma:
        return "conv.valu" + dd
    if plan["nbands"] == 0:
        return "conv.im2col" + dd
    ks = plan["KS"]
    if plan["ur"]:
        return "conv.img2%s<%d,1>" % (dd, 1 if ks == 1 else 0)
    keep = (9, 4) if plan["dil"] else (9, 4, 1)
    return "conv.img2%s<%d,0>" % (dd, ks if ks in keep else 0)
