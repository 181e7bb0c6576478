"""The case table of the device range guard (dash_amd/csrc/hip/guard.hip DevRangeGuard) and its plain reference,
shared by test_guard_cases.py (validates the table on the CPU) and test_gpu_range_guard.py (runs every case on the
GPU). The guard vouches for the rescale and sign gadgets: its dangerous failure is a false negative, so the cases
sit one unit on either side of every limit and compare the kernels' activations element for element.

A case builder returns (circuit, M, inputs, expected_bad); expected_bad comes only from RangeGuard.violations_np.
CASES maps a name to a Case: the builder, the inputs the table says exceed a linear layer's operand range (the
kernels' "uncertain" bit 1, written by hand and checked against operand_uncertain), whether the case also runs
with DASH_GUARD_I24=0, and for a pass / refuse pair its partner and the one input that may differ.

simulate_spec is a numpy int64 interpreter of RangeGuard.native_spec with the kernels' semantics. Like k_g_pool it
range-checks the elements a max-pooling window reads; violations_np checks the layer's whole input, so it is the
stricter one only for an element that a strided pool skips and no gadget ever sees (no case relies on that).

Accumulator bound: the 64-bit forms accumulate int32 operands times int32 weights in int64, which holds
sum_k |w_k| * 2^31 + |bias| only while a row's sum_k |w_k| stays below 2^32. Quantized model-zoo rows are far
below that (test_guard_cases.py measures them), so no layer is refused for it.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import dash_amd as d
from dash_amd.garbling import RangeGuard
from dash_amd.ir import layers as L
from dash_amd.ir.bases import crt_modulus, first_primes
from dash_amd.ir.layers import _im2col

M_BIG = 1 << 40  # no limit interferes: activations are compared as values
M6 = crt_modulus(first_primes(6))  # 30030: half 15015 is odd (halving constant c = 1), Rescale(5) has a wrap band
M3 = crt_modulus(first_primes(3))  # 30: signed range [-15, 15)
LIM24 = (1 << 23) - 1
I32_MAX, I32_MIN = (1 << 31) - 1, -(1 << 31)


# ------------------------------------------------------------------------------------ the reference interpreter
def simulate_spec(spec, xs):
    """Numpy interpreter of RangeGuard.native_spec with the kernels' semantics (csrc/hip/guard.hip), buffers
    shared exactly as the spec assigns them: a CPU check of the description the GPU guard runs.
    Returns (indices flagged, final activations (B, out_size))."""
    X = np.asarray(xs, dtype=np.int64)
    B = X.shape[0]
    bufs = [np.full((B, e), 7777777, dtype=np.int64) for e in spec["buf_elems"]]
    flags = np.zeros(B, dtype=bool)

    def ctx(i):
        return X if i == 0 else bufs[spec["ctx_buf"][i]]

    def post(ops, y):
        nonlocal flags
        for o in ops:
            if o.get("check"):
                flags |= ((y < o["lo"]) | (y >= o["hi"])).any(axis=1)
            k = o["kind"]
            if k == 2:
                for _ in range(o["l"]):
                    y = (y + o["c"]) >> 1
            elif k == 3:
                y = (y + o["c"]) // o["S"]
            elif k == 4:
                y = np.maximum(y, 0)
            elif k == 5:
                y = np.where(y >= 0, 1, -1)
        return y

    for d_ in spec["layers"]:
        x = ctx(d_["src"])[:, :d_["in_size"]].copy()
        k = d_["kind"]
        if k == 0:
            C, H, W, F, g = d_["C"], d_["H"], d_["W"], d_["F"], d_.get("g", 1)
            Cg, Fg = C // g, F // g
            xp = np.pad(x.reshape(B, C, H, W), ((0, 0), (0, 0), (d_["ph"], d_["ph"]), (d_["pw"], d_["pw"])))
            w = d_["w"].astype(np.int64).reshape(g, Fg, Cg, d_["kh"], d_["kw"])
            y = np.zeros((B, g, Fg, d_["OH"], d_["OW"]), np.int64)
            for dy in range(d_["kh"]):
                for dx in range(d_["kw"]):
                    win = xp[:, :, dy:dy + d_["sh"] * (d_["OH"] - 1) + 1:d_["sh"],
                             dx:dx + d_["sw"] * (d_["OW"] - 1) + 1:d_["sw"]]
                    # group q: its filters against its own channels
                    y += np.einsum("bqchw,qfc->bqfhw", win.reshape(B, g, Cg, d_["OH"], d_["OW"]), w[:, :, :, dy, dx])
            y = (y.reshape(B, F, d_["OH"], d_["OW"]) + d_["b"][None, :, None, None]).reshape(B, -1)
        elif k == 1:
            xin = x if d_.get("perm") is None else x[:, d_["perm"]]
            y = xin @ d_["w"].astype(np.int64).T + d_["b"]
        elif k in (6, 7):
            v = x.reshape(B, d_["C"], d_["H"], d_["W"])
            ws = [v[:, :, dy:dy + d_["sh"] * (d_["OH"] - 1) + 1:d_["sh"], dx:dx + d_["sw"] * (d_["OW"] - 1) + 1:d_["sw"]]
                  for dy in range(d_["kh"]) for dx in range(d_["kw"])]
            st = np.stack(ws)
            if d_.get("check"):  # the kernel reads the windows' elements only
                flags |= ((st < d_["lo"]) | (st >= d_["hi"])).any(axis=0).reshape(B, -1).any(axis=1)
            if k == 6:
                y = st.max(axis=0)
                if d_.get("check"):
                    flags |= ((st.max(axis=0) - st.min(axis=0)).reshape(B, -1) > d_["span_max"]).any(axis=1)
            else:
                y = st.sum(axis=0)
            y = y.reshape(B, -1)
        elif k == 8:
            y = x + ctx(d_["add_src"])[:, :d_["in_size"]]
        else:
            y = x
        bufs[d_["buf"]][:, :d_["out_size"]] = post(d_.get("post", []), y)
    out = bufs[spec["layers"][-1]["buf"]][:, :spec["layers"][-1]["out_size"]]
    flags |= ((out < spec["out_lo"]) | (out >= spec["out_hi"])).any(axis=1)
    return [int(i) for i in np.nonzero(flags)[0]], out


def conv_asafe(conv) -> int:
    """The 24-bit form's operand bound of a conv layer (0: a weight beyond 24 bits, the 64-bit form), in Python
    integers: asafe = min(2^23 - 1, (2^31 - 1) // max_f sum|w_f|)."""
    w = [[abs(int(v)) for v in row] for row in np.asarray(conv.q_weights).reshape(conv.F, -1)]
    if max(max(r) for r in w) > LIM24:
        return 0
    return min(LIM24, I32_MAX // max(1, max(sum(r) for r in w)))


def operand_uncertain(circuit, M, x, i24=True) -> bool:
    """Whether an operand a linear layer reads leaves that layer's exact operand range (the kernels' bit 1): a conv
    in the 24-bit form beyond +-asafe, a 64-bit conv or a dense layer beyond int32. Plain numpy evaluation."""
    x = np.asarray(x, dtype=np.int64).reshape(-1)
    ctx, cur = [x], x
    for l in circuit.layers:
        src = getattr(l, "in_src", None)
        inp = ctx[src + 1] if src is not None else cur
        if isinstance(l, L.Conv2d):
            cols, _, _ = _im2col(inp, l.C, l.H, l.W, l.kh, l.kw, l.sh, l.sw, l.ph, l.pw)  # the taps that are read
            a = conv_asafe(l) if i24 else 0
            if (a and (np.abs(cols) > a).any()) or (not a and ((cols > I32_MAX) | (cols < I32_MIN)).any()):
                return True
        elif isinstance(l, L.Dense):
            if ((inp > I32_MAX) | (inp < I32_MIN)).any():
                return True
        cur = l.plain_q_eval(inp, False, ctx, M)
        ctx.append(cur)
    return False


def expected_bad(circuit, M, xs):
    g = RangeGuard(circuit, M, mrs=True)
    return [i for i, x in enumerate(xs) if g.violations_np(x)]


def _ret(circuit, M, xs):
    xs = [np.asarray(x, dtype=np.int64).reshape(-1) for x in xs]
    return circuit, M, xs, expected_bad(circuit, M, xs)


# ------------------------------------------------------------------------------------ conv forms
def _conv(rng, C, H, W, F, kh, kw, sh=1, sw=1, ph=0, pw=0, g=1, wmax=9, big=False):
    w = rng.integers(-wmax, wmax + 1, (F, C // g, kh, kw))
    if big:  # one weight of 2^23: the layer takes the 64-bit form by itself
        w[F - 1, 0, kh - 1, kw - 1] = 1 << 23
    return d.Conv2d.from_quantized(w, rng.integers(-50, 51, F), W, H, C, F, kw, kh, sw, sh, pad_width=pw,
                                   pad_height=ph, groups=g)


# name: (C, H, W, F, kh, kw, sh, sw, ph, pw, groups, B, weights, tail); the k_g_conv instance is
# <3x3 | 2x2 | 1x1 | generic> x <24-bit | 64-bit> x <padded | unpadded>; "big" reaches the 64-bit form by a weight of
# 2^23, "env" cases run in both forms (DASH_GUARD_I24 unset and 0) and must agree. Output pixels per image 1, 63, 64
# and 65 are the wave-padding boundaries; F = 1, 7, 8, 9, 17 the clamped last filter block.
CONV_FORMS = {
    "c33_i24_7x9px_f7":       (3, 9, 11, 7, 3, 3, 1, 1, 0, 0, 1, 3, "small", "relu"),      # 63 pixels
    "c33_i24_pad_8x8px_f9":   (1, 8, 8, 9, 3, 3, 1, 1, 1, 1, 1, 1, "small", "rescale"),    # 64 pixels, C = 1, B = 1
    "c33_big_1px_f1":         (3, 3, 3, 1, 3, 3, 1, 1, 0, 0, 1, 3, "big", "none"),         # 1 pixel, F = 1
    "c33_env_pad_s2_5x13px":  (3, 9, 25, 17, 3, 3, 2, 2, 1, 1, 1, 3, "env", "relu"),       # 65 pixels, stride 2 pad 1
    "c33_i24_pad_depthwise":  (3, 8, 8, 3, 3, 3, 1, 1, 1, 1, 3, 3, "small", "relu"),       # Fg = 1
    "c22_i24_sh2_sw1_f8":     (3, 8, 10, 8, 2, 2, 2, 1, 0, 0, 1, 3, "small", "rescale"),   # sh != sw
    "c22_i24_ph1_8x8px_f17":  (1, 7, 9, 17, 2, 2, 1, 1, 1, 0, 1, 1, "small", "none"),      # ph = 1, pw = 0
    "c22_env_groups_fg10":    (6, 4, 4, 20, 2, 2, 1, 1, 0, 0, 2, 3, "env", "relu"),        # Fg = 10, Cg = 3
    "c22_big_pw1":            (1, 6, 5, 7, 2, 2, 1, 1, 0, 1, 1, 3, "big", "relu"),         # ph = 0, pw = 1
    "c11_i24_5x13px_f9":      (3, 5, 13, 9, 1, 1, 1, 1, 0, 0, 1, 3, "small", "rescale"),   # 65 pixels
    "c11_i24_ph1_7x9px_f8":   (1, 5, 9, 8, 1, 1, 1, 1, 1, 0, 1, 3, "small", "none"),       # 63 pixels, border rows = bias
    "c11_big_s3_unread":      (3, 8, 8, 7, 1, 1, 3, 3, 0, 0, 1, 3, "big", "relu"),         # row / column 7 unread
    "c11_env_pad_depthwise":  (3, 4, 4, 3, 1, 1, 1, 1, 1, 1, 3, 1, "env", "none"),
    "c55_i24_s2_f7":          (3, 9, 9, 7, 5, 5, 2, 2, 0, 0, 1, 3, "small", "relu"),
    "c13_i24_pw1_7x9px_f9":   (1, 7, 9, 9, 1, 3, 1, 1, 0, 1, 1, 3, "small", "relu"),       # kh = 1, kw = 3; 63 pixels
    "c31_big_sh3_unread_f17": (3, 10, 8, 17, 3, 1, 3, 1, 0, 0, 1, 3, "big", "none"),       # kh = 3, kw = 1; row 9 unread
    "c53_env_pad_sh2_f8":     (3, 8, 6, 8, 5, 3, 2, 1, 1, 1, 1, 3, "env", "rescale"),
}


def conv_form_case(name):
    C, H, W, F, kh, kw, sh, sw, ph, pw, g, B, wts, tail = CONV_FORMS[name]
    rng = np.random.default_rng(sorted(CONV_FORMS).index(name) + 100)
    conv = _conv(rng, C, H, W, F, kh, kw, sh, sw, ph, pw, g, big=wts == "big")
    n = conv.out_dims
    layers = [conv] + {"none": [], "relu": [d.Relu(n)], "rescale": [d.Rescale(2, n), d.Relu(n)]}[tail]
    xs = [rng.integers(-20, 21, conv.in_size) for _ in range(B)]
    if "unread" in name:  # the stride leaves the last row (and column) unread: a value no operand could hold
        v = xs[-1].reshape(C, H, W)
        v[:, H - 1, :] = 1 << 35
        if sw > 1:
            v[:, :, W - 1] = -(1 << 35)
    return _ret(d.Circuit(layers), M_BIG, xs)


# ------------------------------------------------------------------------------------ the 24-bit operand bound
def _worst_input(conv, f, oy, ox, a):
    """Every in-image tap of output pixel (oy, ox) holds +-a with the sign of filter f's weight (groups = 1)."""
    x = np.zeros((conv.C, conv.H, conv.W), np.int64)
    for dy in range(conv.kh):
        for dx in range(conv.kw):
            iy, ix = oy * conv.sh - conv.ph + dy, ox * conv.sw - conv.pw + dx
            if 0 <= iy < conv.H and 0 <= ix < conv.W:
                x[:, iy, ix] = np.where(conv.q_weights[f, :, dy, dx] >= 0, a, -a)
    return x.reshape(-1)


def i24_bound_case(kind):
    """Inputs: 0 the worst case of the heaviest filter (exact, certain), 1 one operand at asafe + 1, 2 one at
    -(asafe + 1) (both uncertain, nothing else), 3 a small one. kind: "sum" (asafe set by the int32 partial
    sums), "cap" (small weights: asafe = 2^23 - 1, the multiplier's width), "border" (padded, the worst case on
    the corner pixel, whose in-image taps are the heaviest)."""
    rng = np.random.default_rng(7)
    if kind == "cap":
        conv = _conv(rng, 2, 3, 3, 3, 3, 3, wmax=9)
    elif kind == "sum":
        conv = _conv(rng, 2, 3, 3, 3, 3, 3, wmax=200)
    else:  # filter 1 is the heaviest and all its weight sits on the taps of pixel (0, 0) that lie in the image
        conv = _conv(rng, 2, 4, 4, 3, 3, 3, ph=1, pw=1, wmax=20)
        conv.q_weights[1] = 0
        conv.q_weights[1, :, 1:, 1:] = rng.integers(100, 201, (2, 2, 2)) * np.where(rng.integers(0, 2, (2, 2, 2)) > 0, 1, -1)
    a = conv_asafe(conv)
    f = int(np.abs(conv.q_weights).reshape(conv.F, -1).sum(axis=1).argmax())
    xs = [_worst_input(conv, f, 0, 0, a)]
    for v in (a + 1, -(a + 1)):
        x = rng.integers(-20, 21, conv.in_size)
        x[5] = v
        xs.append(x)
    xs.append(rng.integers(-20, 21, conv.in_size))
    return _ret(d.Circuit([conv]), M_BIG, xs)


def i24_wrapped_sum_case():
    """The worst case with every operand at +-(asafe + 1): the 24-bit form's int32 sum wraps, and with this bias and
    modulus the wrapped value (about -2^32) violates the ReLU's range while the true value (about 0) does not. The
    input is uncertain and the exact host model passes it: its device bit 0 must not refuse it."""
    rng = np.random.default_rng(8)
    conv = _conv(rng, 2, 3, 3, 3, 3, 3, wmax=200)
    a = conv_asafe(conv)
    f = int(np.abs(conv.q_weights).reshape(conv.F, -1).sum(axis=1).argmax())
    conv.q_biases[f] = -(1 << 31)
    xs = [_worst_input(conv, f, 0, 0, a + 1), rng.integers(-20, 21, conv.in_size), _worst_input(conv, f, 0, 0, a)]
    return _ret(d.Circuit([conv, d.Relu(conv.out_dims)]), 3 << 31, xs)  # signed range [-3 * 2^30, 3 * 2^30)


# ------------------------------------------------------------------------------------ dense
def dense_case(kind):
    rng = np.random.default_rng(11)
    if kind == "1x1":
        c = d.Circuit([d.Dense.from_quantized([[-3]], [5]), d.Relu((1,))])
        xs = [[4], [-6], [0]]
    elif kind == "out257":  # 771 lanes: the lanes of one block span two inputs
        c = d.Circuit([d.Dense.from_quantized(rng.integers(-9, 10, (257, 5)), rng.integers(-50, 51, 257))])
        xs = [rng.integers(-20, 21, 5) for _ in range(3)]
    elif kind == "channel_tf3":
        c = d.Circuit([d.Dense.from_quantized(rng.integers(-9, 10, (4, 12)), rng.integers(-50, 51, 4), channel_tf=3),
                       d.Relu((4,))])
        xs = [rng.integers(-20, 21, 12) for _ in range(3)]
    else:  # "int32": 0 both int32 ends (exact, certain), 1 and 2 one past either end (uncertain), 3 small
        c = d.Circuit([d.Dense.from_quantized(rng.integers(-3, 4, (3, 4)) | 1, rng.integers(-50, 51, 3))])
        xs = [[I32_MAX, I32_MIN, 5, -7], [1, I32_MAX + 1, 2, 3], [I32_MIN - 1, 1, 2, 3], [4, -3, 2, 1]]
    return _ret(c, M_BIG, xs)


# ------------------------------------------------------------------------------------ pools
def pool_case(kind):
    rng = np.random.default_rng(13)
    P = {"max": d.MaxPool2d, "sum": d.SumPool2d}[kind.split("_")[0]]
    if kind.endswith("overlap_gaps"):  # kh != kw, sw < kw (overlap), sh > kh (gaps); 18 outputs per input, B = 3
        p = P(7, 6, 3, 3, 2, 2, 3)
    else:  # "whole": one window over the whole image, C = 1
        p = P(4, 3, 1, 4, 3)
    return _ret(d.Circuit([p]), M_BIG, [rng.integers(-99, 100, p.in_size) for _ in range(3)])


# max pooling limits, modulus 30: inputs in [-15, 15), span_max = 14. name: (window of the variant input, refused?)
POOL_LIMITS = {
    "span_max": ([-7, 7], False), "span_max+1": ([-7, 8], True),
    "lo": ([-15, -3], False), "lo-1": ([-16, -3], True),
    "hi-1": ([2, 14], False), "hi": ([2, 15], True),
}


def pool_limit_case(name):
    """Two windows of two per input (C = 2, H = 1, W = 2); input 1's second window is the variant."""
    win, _ = POOL_LIMITS[name]
    c = d.Circuit([d.MaxPool2d(2, 1, 2, 2, 1)])
    return _ret(c, M3, [[1, -2, 3, 4], [0, 5] + win, [-4, 4, 6, 6]])


# ------------------------------------------------------------------------------------ elementwise, fused epilogues
NEG = [-9, -8, -1, -2, 0, 1, 7, -33, -64, -63, 32, 31]


def elem_case(kind):
    n = len(NEG)
    eye = d.Dense.from_quantized(np.eye(4, dtype=np.int64), np.zeros(4, np.int64))
    if kind.startswith("halve"):  # an elementwise head: legacy halvings of negative odd and even values, c = 1
        c = d.Circuit([d.Rescale(int(kind[-1]), (n,))])
        xs = [NEG, [v - 1 for v in NEG], [-v for v in NEG]]
    elif kind == "redash_div":  # S = 6, c = 15015 mod 6 = 3: negative values divisible by 6 after + c and not
        c = d.Circuit([d.Rescale([2, 3], (n,))])
        xs = [[-3, -9, -15, -4, -5, -6, -7, -8, -10, 3, 2, 0], NEG, [-v for v in NEG]]
    elif kind == "sign":
        c = d.Circuit([d.Sign((3,))])
        xs = [[-1, 0, 1], [0, 0, -1], [1, -1, 0]]
    elif kind == "relu0":
        c = d.Circuit([d.Relu((3,))])
        xs = [[0, -1, 1], [-1, -1, 0], [5, 0, -5]]
    elif kind in ("caught_by_second", "caught_by_third"):  # ReLU passes the wrap band [mrs_limit, M/2), the Rescale(5) after it not
        mid = [d.Relu((4,)) for _ in range(1 if kind == "caught_by_second" else 2)]
        c = d.Circuit([eye] + mid + [d.Rescale(5, (4,))])
        lim = c.layers[-1].mrs_limit(M6)
        assert lim < M6 // 2 - 8
        xs = [[1, lim - 1, -5, 0], [1, 2, lim, 0], [0, 0, 0, M6 // 2 - 1]]
    elif kind == "run_of_eight":  # the spec splits the run at six fused ops
        run = [l for _ in range(4) for l in (d.Relu((4,)), d.Rescale(1, (4,)))]
        c = d.Circuit([eye] + run)
        xs = [[1000, -1000, 15014, -15015], [17, 16, 15, -17], [0, 0, 15015, 0]]
    elif kind == "add_from_input":  # the residual is the circuit input (stride N), B = 3
        rng = np.random.default_rng(17)
        c = d.Circuit([d.Dense.from_quantized(rng.integers(-5, 6, (30, 6)), rng.integers(-9, 10, 30)),
                       d.Dense.from_quantized(rng.integers(-5, 6, (6, 30)), rng.integers(-9, 10, 6)),
                       d.Add((6,), -1), d.Relu((6,))])
        xs = [rng.integers(-20, 21, 6) for _ in range(3)]
    else:  # "add_strided": sizes 50, 5, 5: the add's input lives in the 50-wide buffer (stride 50, 5 stored), B = 3
        assert kind == "add_strided"
        rng = np.random.default_rng(19)
        dn = [d.Dense.from_quantized(rng.integers(-5, 6, s), rng.integers(-9, 10, s[0]))
              for s in ((50, 8), (5, 50), (5, 5), (50, 5))]
        c = d.Circuit(dn[:3] + [d.Add((5,), 1), d.Relu((5,)), dn[3]])
        xs = [rng.integers(-20, 21, 8) for _ in range(3)]
    big = kind in ("add_from_input", "add_strided", "sign", "relu0")
    return _ret(c, M_BIG if big else M6, xs)


# ------------------------------------------------------------------------------------ limit edges through each head
# (head, follow, side, filter or output index). The conv heads have F = 12: filter blocks [0, 8) and the clamped
# [8, 12); filters 0 (first), 9 (in the clamped block) and 11 (last). "edge" variants put the extreme pre-activation
# of that filter on the last passing value (hi - 1 or lo), "over" variants one unit further (hi or lo - 1).
EDGE_HEADS = {
    "conv33pad": lambda rng: _conv(rng, 3, 5, 6, 12, 3, 3, ph=1, pw=1),
    "conv22": lambda rng: _conv(rng, 3, 5, 6, 12, 2, 2),
    "conv11": lambda rng: _conv(rng, 3, 5, 6, 12, 1, 1),
    "conv53s": lambda rng: _conv(rng, 3, 9, 8, 12, 5, 3, 2, 1),
    "dense": lambda rng: d.Dense.from_quantized(rng.integers(-9, 10, (12, 7)), rng.integers(-50, 51, 12)),
    "sumpool": lambda rng: d.SumPool2d(6, 4, 2, 3, 2),
    "add": lambda rng: d.Dense.from_quantized(rng.integers(-9, 10, (6, 6)), rng.integers(-50, 51, 6)),
}
EDGES = [
    ("conv33pad", "relu", "hi", 0), ("conv22", "relu", "hi", 9), ("conv11", "relu", "hi", 11),
    ("conv53s", "relu", "lo", 0), ("conv33pad", "relu", "lo", 9), ("conv22", "relu", "lo", 11),
    ("conv11", "rescale", "hi", 0), ("conv53s", "rescale", "hi", 9), ("conv33pad", "rescale", "hi", 11),
    ("conv22", "rescale", "lo", 0), ("conv11", "rescale", "lo", 9), ("conv53s", "rescale", "lo", 11),
    ("dense", "relu", "hi", 0), ("dense", "relu", "lo", 11), ("dense", "rescale", "hi", 11), ("dense", "rescale", "lo", 0),
    ("sumpool", "relu", "hi", 0), ("sumpool", "relu", "lo", 5), ("sumpool", "rescale", "hi", 5),
    ("sumpool", "rescale", "lo", 0),
    ("add", "relu", "hi", 0), ("add", "relu", "lo", 5), ("add", "rescale", "hi", 5), ("add", "rescale", "lo", 0),
]


def edge_case(head, follow, side, idx, over):
    """Input 1 of 3 holds the extreme pre-activation of filter / output idx; the bias of that filter (conv, dense)
    or one element of input 1 (pools, adds) is shifted until the extreme equals the limit's last passing value
    (over = False) or the first refused one (over = True)."""
    rng = np.random.default_rng(23)
    h = EDGE_HEADS[head](rng)
    if head == "add":  # x -> Dense -> + x: column idx of the weights is zero, so x[idx] moves output idx alone
        h.q_weights[:, idx] = 0
        layers = [h, d.Add((6,), -1)]
    else:
        layers = [h]
    n = layers[-1].out_dims
    fol = d.Relu(n) if follow == "relu" else d.Rescale(5, n)
    c = d.Circuit(layers + [fol])
    lo, hi = RangeGuard(c, M6, mrs=True)._limits(fol)
    assert (lo, hi) == (-15015, 15015 if follow == "relu" else fol.mrs_limit(M6)) and hi <= 15015
    target = (hi - 1 + over) if side == "hi" else (lo - over)
    xs = [rng.integers(-20, 21, c.input_size) for _ in range(3)]
    pre = d.Circuit(layers)
    if head in ("sumpool", "add"):
        # output idx of input 1 moves one for one with an element it reads (the pool's first tap / x[idx])
        y = pre.plain_q_eval(xs[1], False, M6)
        el = idx if head == "add" else (idx // (h.OH * h.OW)) * h.H * h.W + (idx // h.OW % h.OH) * h.sh * h.W \
            + (idx % h.OW) * h.sw
        xs[1][el] += target - int(y[idx])
    else:
        per = 1 if head == "dense" else h.OH * h.OW
        ys = np.stack([pre.plain_q_eval(x, False, M6).reshape(-1, per)[idx] for x in xs])
        ext = ys.max(axis=1) if side == "hi" else ys.min(axis=1)
        order = np.argsort(ext)
        b = int(order[-1] if side == "hi" else order[0])
        xs[1], xs[b] = xs[b], xs[1]  # the input holding the extreme goes to index 1
        h.q_biases[idx] += target - int(ext[b])
    return _ret(c, M6, xs)


# ------------------------------------------------------------------------------------ the table
Case = namedtuple("Case", "build uncertain env pair_of variant")


def _case(build, uncertain=(), env=False, pair_of=None, variant=None):
    return Case(build, tuple(uncertain), env, pair_of, variant)


CASES = {}
for _n, _v in CONV_FORMS.items():
    CASES[_n] = _case(lambda n=_n: conv_form_case(n), env=_v[12] == "env")
for _k in ("sum", "cap", "border"):
    CASES["i24_bound_" + _k] = _case(lambda k=_k: i24_bound_case(k), uncertain=(1, 2))
CASES["i24_wrapped_sum"] = _case(i24_wrapped_sum_case, uncertain=(0,))
for _k in ("1x1", "out257", "channel_tf3"):
    CASES["dense_" + _k] = _case(lambda k=_k: dense_case(k))
CASES["dense_int32"] = _case(lambda: dense_case("int32"), uncertain=(1, 2))
for _k in ("max_overlap_gaps", "max_whole", "sum_overlap_gaps", "sum_whole"):
    CASES["pool_" + _k] = _case(lambda k=_k: pool_case(k))
_POOL_PAIRS = {"span_max+1": "span_max", "lo-1": "lo", "hi": "hi-1"}
for _k in POOL_LIMITS:
    _p = _POOL_PAIRS.get(_k)
    CASES["maxpool_" + _k] = _case(lambda k=_k: pool_limit_case(k), pair_of="maxpool_" + _p if _p else None,
                                   variant=1 if _p else None)
for _k in ["halve%d" % l for l in range(1, 6)] + ["redash_div", "sign", "relu0", "caught_by_second",
                                                  "caught_by_third", "run_of_eight", "add_from_input", "add_strided"]:
    CASES["elem_" + _k] = _case(lambda k=_k: elem_case(k))
for _e in EDGES:
    _name = "edge_%s_%s_%s_%d" % _e
    CASES[_name] = _case(lambda e=_e: edge_case(*e, over=False))
    CASES[_name + "_over"] = _case(lambda e=_e: edge_case(*e, over=True), pair_of=_name, variant=1)
NAMES = list(CASES)


# the small conv -> rescale -> ReLU circuit of the ticket / chunk / graph tests
def ticket_circuit():
    rng = np.random.default_rng(29)
    conv = _conv(rng, 2, 4, 4, 3, 3, 3, ph=1, pw=1)
    n = conv.out_dims
    return d.Circuit([conv, d.Rescale(5, n), d.Relu(n)])


def ticket_inputs(c, B, bad=(), seed=0):
    """B small inputs; the ones listed in bad hold one element large enough to push a rescale input past M/2."""
    rng = np.random.default_rng(seed)
    xs = [rng.integers(-20, 21, c.input_size) for _ in range(B)]
    for i in bad:
        xs[i][int(rng.integers(0, c.input_size))] = 14000
    return xs
