"""The coverage table of the conv kernel forms (kernels_gemm.hip launch_conv / k_conv_img2) and the in-kernel
predicates, restated in Python. Shared by test_conv_plan.py (asserts every row through the planner binding, on
the CPU) and test_gpu_gemm_forms.py (runs every row on the GPU).

A row names the smallest shape found that reaches its form with the default 40 KiB LDS budget. The expected
columns are written by hand (worked out from launch.h, not copied from the code under test):
  form    the kernel launch_conv picks, as the launch log prints it
  plan    ur, KS (k-steps of 64), band (output rows per block), nbands
  sh24    per residue: the 24-bit reduction's shift, -1 for the 32-bit reduction
  stage   "q8": branch-free 8-byte loads (staged input row at least 8 wide), "b1": byte-wise
  stores  per band the epilogue store forms its columns take: "b128" (16-byte chunk of 64 columns), "dword", "byte"
"""


def ceil_div(a, b):
    return -(-a // b)


def _case(name, C, H, W, F, k, crt, form, ur, KS, band, nbands, sh24, stage, stores, stride=1, pad=None):
    pad = (k // 2 if k == 3 else 0) if pad is None else pad
    return dict(name=name, C=C, H=H, W=W, F=F, kh=k, kw=k, sh=stride, sw=stride, ph=pad, pw=pad, crt=crt, form=form,
                ur=ur, KS=KS, band=band, nbands=nbands, sh24=sh24, stage=stage, stores=stores)


B7 = [7, 127, 131]    # Kpad = 576: raw 24-bit, raw 32-bit, centered 24-bit in one launch
B32 = [32, 97, 107]   # an even modulus; both primes raw and 32-bit at Kpad = 576
B5 = [5, 128, 251]    # p = 128 (centered, half = 64) and the largest prime, both 32-bit from Kpad = 576 on
B2 = [2, 3, 5]        # p = 2: half = 1, 128 components

CONV_CASES = [
    # k_conv_img2<9,false>: the headline's kernel
    _case("k9_c58_w13", 58, 6, 13, 20, 3, B7, "conv.img2<9,0>", 0, 9, 6, 1, [6, -1, 1], "q8", [("byte",)]),
    _case("k9_c60_f70", 60, 8, 16, 70, 3, B32, "conv.img2<9,0>", 0, 9, 8, 1, [4, -1, -1], "q8", [("b128",)]),
    _case("k9_w5", 64, 5, 5, 6, 3, B5, "conv.img2<9,0>", 0, 9, 5, 1, [6, -1, -1], "b1", [("byte",)]),
    _case("k9_tail_chunk", 64, 5, 16, 6, 3, B7, "conv.img2<9,0>", 0, 9, 5, 1, [6, -1, 1], "q8", [("b128", "dword")]),
    _case("k9_bands_short", 64, 34, 10, 6, 3, B7, "conv.img2<9,0>", 0, 9, 31, 2, [6, -1, 1], "q8",
          [("byte", "dword"), ("byte",)]),
    _case("k9_bands_b128", 64, 26, 16, 6, 3, B7, "conv.img2<9,0>", 0, 9, 18, 2, [6, -1, 1], "q8",
          [("b128", "dword"), ("b128",)]),  # 288 = 4 chunks + 32 columns, then 128
    # the other A-in-registers instances
    _case("k4_2x2", 64, 9, 9, 20, 2, B7, "conv.img2<4,0>", 0, 4, 8, 1, [6, 2, 1], "q8", [("b128",)]),
    _case("k1_1x1", 24, 9, 9, 20, 1, B7, "conv.img2<1,0>", 0, 1, 9, 1, [6, 2, 1], "q8", [("byte",)]),
    _case("k1_1x1_s2", 64, 9, 9, 20, 1, B7, "conv.img2<1,0>", 0, 1, 5, 1, [6, 2, 1], "q8", [("byte",)], stride=2),
    # streamed A: two channel chunks, and the unrolled view that does not fit falling back to the layer's own image
    _case("k0_c128", 128, 6, 8, 6, 3, B5, "conv.img2<0,0>", 0, 18, 6, 1, [6, -1, -1], "q8", [("dword",)]),
    _case("k0_c70_s2", 70, 9, 9, 6, 3, B7, "conv.img2<0,0>", 0, 18, 5, 1, [6, -1, 1], "q8", [("byte",)], stride=2),
    _case("k0_fallback", 16, 6, 92, 4, 5, B7, "conv.img2<0,0>", 0, 25, 1, 6, [6, -1, 1], "q8", [("dword",)] * 6,
          pad=2),
    # tap-unrolled
    _case("ur1_bands", 3, 34, 32, 8, 3, B7, "conv.img2<1,1>", 1, 1, 12, 3, [6, 2, 1], "q8", [("b128",)] * 3),
    _case("ur0_bands", 3, 30, 20, 6, 5, B7, "conv.img2<0,1>", 1, 2, 12, 3, [6, 2, 1], "q8", [("dword",)] * 3, pad=2),
    _case("ur1_w6", 3, 6, 6, 6, 3, B2, "conv.img2<1,1>", 1, 1, 6, 1, [8, 7, 6], "b1", [("dword",)]),
    _case("ur1_w7", 3, 7, 7, 6, 3, B5, "conv.img2<1,1>", 1, 1, 7, 1, [6, 2, 1], "b1", [("byte",)]),
    # no band fits: im2col
    _case("im2col_1x1", 64, 2, 516, 4, 1, B7, "conv.im2col", 0, 1, 0, 0, [6, 2, 1], None, []),
    _case("im2col_3x3", 3, 3, 600, 4, 3, B7, "conv.im2col", 0, 9, 0, 0, [6, 2, 1], None, [], pad=0),
]
CASE = {c["name"]: c for c in CONV_CASES}


def plan_of(native, c, mfma=True):
    return native.hip_conv_plan(c["C"], c["H"], c["W"], c["F"], c["kh"], c["kw"], c["sh"], c["sw"], c["ph"], c["pw"],
                                c["crt"], mfma)


# --------------------------------------------------------------------------- launch_conv and k_conv_img2, restated
def form_of(plan):
    """launch_conv's pick among the MFMA kernels."""
    if plan["nbands"] == 0:
        return "conv.im2col"
    ks = plan["KS"]
    if plan["ur"]:
        return "conv.img2<1,1>" if ks == 1 else "conv.img2<0,1>"
    return "conv.img2<%d,0>" % (ks if ks in (9, 4, 1) else 0)


def stage_of(c, plan):
    """The staging path: the unrolled view loads from the layer's input rows, the plain view from its own."""
    return "q8" if c["W"] >= 8 else "b1"  # (ur: uW = the layer's W; plain: W)


def store_forms(npos, OW, row0, rows):
    """The store forms the columns of one band (output rows row0 .. row0 + rows) take, per 64-column chunk and per
    group of 4 columns."""
    ncol, start = rows * OW, row0 * OW
    dw = npos % 4 == 0 and start % 4 == 0
    dw16 = npos % 16 == 0 and start % 16 == 0
    forms = set()
    for colw in range(0, ncol, 64):
        if dw16 and colw + 64 <= ncol:
            forms.add("b128")
            continue
        for cb in range(colw, min(colw + 64, ncol), 4):
            forms.add("dword" if dw and cb + 3 < ncol else "byte")
    return tuple(sorted(forms))


def stores_of(plan):
    out = []
    for b in range(plan["nbands"]):
        row0 = b * plan["band"]
        out.append(store_forms(plan["OH"] * plan["OW"], plan["OW"], row0, min(plan["band"], plan["OH"] - row0)))
    return out


def reduction_of(sh24):
    return "u24" if sh24 >= 0 else "u32"


def operand_of(p):
    return "raw" if p < 128 else "centered"


def acc_bound(p, Kpad):
    """The epilogue's worst case x = acc + off + zc * zv + bias stays below this (conv_img_geometry's X)."""
    half = p // 2
    xmax = p - 1 if p < 128 else half
    return 2 * Kpad * half * xmax + (Kpad + 3) * p


def sh24_of(p, Kpad):
    """The smallest shift with ceil(2^(32 - sh) / p) < 2^24; the 24-bit reduction is exact while x << sh < 2^24."""
    sh = 0
    while (1 << (8 - sh)) >= p:
        sh += 1
    return sh if acc_bound(p, Kpad) < 1 << (24 - sh) else -1
