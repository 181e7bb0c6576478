"""The conv coverage table (tests/gemm_cases.py) against the planner, on the CPU: every row reaches the kernel form,
reduction, operand, staging and store classes it is in the table for, and together the rows cover every form and
class of launch_conv / k_conv_img2. test_gpu_gemm_forms.py runs the same rows on the GPU."""
import pytest

from tests.gemm_cases import (CASE, CONV_CASES, acc_bound, form_of, operand_of, plan_of, reduction_of, sh24_of,
                              stage_of, stores_of)


@pytest.mark.parametrize("name", [c["name"] for c in CONV_CASES])
def test_row(native, name):
    c = CASE[name]
    plan = plan_of(native, c)
    print(plan)
    K = c["C"] * c["kh"] * c["kw"]
    assert plan["Kpad"] == -(-K // 64) * 64
    assert (plan["ur"], plan["KS"], plan["band"], plan["nbands"]) == (c["ur"], c["KS"], c["band"], c["nbands"])
    assert form_of(plan) == c["form"]
    assert plan["sh24"] == c["sh24"] == [sh24_of(p, plan["Kpad"]) for p in c["crt"]]
    if plan["nbands"]:
        assert plan["Cpad"] == -(-(K if c["ur"] else c["C"]) // 64) * 64
        assert plan["KS"] == (1 if c["ur"] else c["kh"] * c["kw"]) * plan["Cpad"] // 64
        in_rows = (plan["band"] - 1) * (1 if c["ur"] else c["sh"]) + (1 if c["ur"] else c["kh"])
        assert in_rows * plan["ldsR"] <= 40 << 10 and plan["ldsS"] >= plan["Cpad"] + 16
        assert plan["ldsR"] >= (plan["OW"] if c["ur"] else c["W"] + 2 * c["pw"]) * plan["ldsS"]
        assert stage_of(c, plan) == c["stage"]
        assert stores_of(plan) == c["stores"]


def test_unroll_fallback_row(native):
    """k0_fallback is planned through conv_plan's fallback: the unroll rule fires (fewer k-steps) but no band of the
    unrolled view fits the budget, so the plan is the layer's own."""
    c = CASE["k0_fallback"]
    K = c["C"] * c["kh"] * c["kw"]
    assert -(-K // 64) < c["kh"] * c["kw"] * -(-c["C"] // 64) and c["sw"] == 1 and max(c["crt"]) <= 255
    S = -(-K // 64) * 64 + 16  # the unrolled view's smallest position stride: one output row alone exceeds 40 KiB
    assert ((c["W"] + 2 * c["pw"] - c["kw"]) + 1) * S > 40 << 10
    assert plan_of(native, c)["ur"] == 0


def test_plan_without_image_kernels(native):
    """mfma=False (the evaluator's VALU switch): no band plan, launch_conv takes k_conv_valu."""
    plan = plan_of(native, CASE["k9_c58_w13"], mfma=False)
    assert plan["nbands"] == 0 and plan["band"] == 0 and plan["ur"] == 0


def test_table_covers_every_form_and_class(native):
    forms, red, stage, stores = set(), set(), set(), set()
    for c in CONV_CASES:
        plan = plan_of(native, c)
        forms.add(form_of(plan))
        if not plan["nbands"]:
            continue
        kind = "ur" if plan["ur"] else "plain"
        for p, s in zip(c["crt"], plan["sh24"]):
            red.add((operand_of(p), reduction_of(s)))
        stage.add((kind, stage_of(c, plan)))
        for band in stores_of(plan):
            stores.update((kind, f) for f in band)
    assert forms == {"conv.img2<9,0>", "conv.img2<4,0>", "conv.img2<1,0>", "conv.img2<0,0>", "conv.img2<1,1>",
                     "conv.img2<0,1>", "conv.im2col"}
    assert red == {(o, r) for o in ("raw", "centered") for r in ("u24", "u32")}
    assert stage == {(k, s) for k in ("plain", "ur") for s in ("q8", "b1")}
    assert stores == {(k, f) for k in ("plain", "ur") for f in ("b128", "dword", "byte")}
    # k_conv_img2<9,false> itself: every class, F > 64, several bands, a partial 4-channel group
    k9 = [c for c in CONV_CASES if c["form"] == "conv.img2<9,0>"]
    assert any(c["F"] > 64 and c["F"] % 16 for c in k9) and any(c["nbands"] > 1 for c in k9)
    assert any(c["C"] % 4 for c in k9) and any(c["W"] % 8 for c in k9) and any(c["W"] < 8 for c in k9)
    assert {f for c in k9 for band in c["stores"] for f in band} == {"b128", "dword", "byte"}
    # even moduli, p = 2, p = 128 and the largest prime are in the table
    assert {2, 32, 128, 251} <= {p for c in CONV_CASES for p in c["crt"]}


def test_tight_24bit_bound_in_table(native):
    """A 24-bit residue whose worst-case accumulator bound is within a factor of 2 of the reduction's exactness
    limit 2^(24 - sh), and the 32-bit reduction at Kpad = 1152 with p = 251 (the worst-case label tests' targets)."""
    c = CASE["k9_c58_w13"]
    plan = plan_of(native, c)
    p, sh = c["crt"][2], plan["sh24"][2]
    assert p == 131 and sh == 1 and 2 * acc_bound(p, plan["Kpad"]) >= 1 << (24 - sh) > acc_bound(p, plan["Kpad"])
    c = CASE["k0_c128"]
    plan = plan_of(native, c)
    assert plan["Kpad"] == 1152 and c["crt"][2] == 251 and plan["sh24"][2] == -1
    assert acc_bound(251, 1152) < 1 << 31  # acc + off stays a non-negative int32
