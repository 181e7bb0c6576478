"""The device range guard's case table (tests/guard_cases.py), validated on the CPU before test_gpu_range_guard.py
trusts it on the device: the three CPU implementations of the guard agree on every case, the native description's
interpreter computes the plaintext activations, every pass / refuse pair differs in exactly the intended input, and
the operand bounds the table claims hold in Python integers."""
import numpy as np
import pytest

from dash_amd.garbling import RangeGuard
from dash_amd.garbling.guard import PendingCheck
from tests import guard_cases as gc

I32_MAX = (1 << 31) - 1


@pytest.fixture(scope="module")
def built():
    """Every case built once: name -> (circuit, M, inputs, expected_bad)."""
    return {n: gc.CASES[n].build() for n in gc.NAMES}


@pytest.mark.parametrize("name", gc.NAMES)
def test_cpu_implementations_agree(built, name):
    c, M, xs, bad = built[name]
    g = RangeGuard(c, M, mrs=True)
    assert g.batched and g.native_forms
    assert bad == [i for i, x in enumerate(xs) if g.violations_np(x)]
    assert sorted(g.submit(xs).bad_indices()) == bad  # the batched torch path
    sbad, out = gc.simulate_spec(g.native_spec(), xs)
    assert sbad == bad
    for i, x in enumerate(xs):
        if i not in bad:
            np.testing.assert_array_equal(out[i], c.plain_q_eval(x, False, M))
    # the inputs the table says leave a linear layer's operand range
    for i24 in (True, False) if gc.CASES[name].env else (True,):
        assert tuple(i for i, x in enumerate(xs) if gc.operand_uncertain(c, M, x, i24)) == gc.CASES[name].uncertain


def test_pairs_differ_in_the_intended_input_only(built):
    pairs = [n for n in gc.NAMES if gc.CASES[n].pair_of]
    assert len(pairs) == len(gc.EDGES) + 3
    for n in pairs:
        case = gc.CASES[n]
        (_, M, xs, bad), (_, M0, xs0, bad0) = built[n], built[case.pair_of]
        assert M == M0 and len(xs) == len(xs0)
        assert bad0 == [] and bad == [case.variant], n  # one unit apart: passes, then exactly that input refused
        for i, (a, b) in enumerate(zip(xs, xs0)):
            if i != case.variant:
                np.testing.assert_array_equal(a, b)
        diff = np.abs(np.asarray(xs[case.variant]) - np.asarray(xs0[case.variant])).sum()
        if n.startswith("edge_conv") or n.startswith("edge_dense"):  # the bias moved by one, not the inputs
            h, h0 = built[n][0].layers[0], built[case.pair_of][0].layers[0]
            assert diff == 0 and np.abs(h.q_biases - h0.q_biases).sum() == 1
            np.testing.assert_array_equal(h.q_weights, h0.q_weights)
        else:
            assert diff == 1


def test_edge_values_sit_on_the_limits(built):
    """The extreme gadget input of the edge cases is the limit's last passing value, of the _over cases the first
    refused one, for the filter the case names (violations_np reports min, max, lo, hi of the violated layer)."""
    for head, follow, side, idx in gc.EDGES:
        name = "edge_%s_%s_%s_%d" % (head, follow, side, idx)
        for over in (False, True):
            c, M, xs, bad = built[name + ("_over" if over else "")]
            pre = type(c)(c.layers[:-1])
            lo, hi = RangeGuard(c, M, mrs=True)._limits(c.layers[-1])
            per = c.layers[0].OH * c.layers[0].OW if head.startswith("conv") else 1
            ys = np.stack([pre.plain_q_eval(x, False, M) for x in xs])
            row = ys[1].reshape(-1, per)[idx]
            if side == "hi":
                assert ys.max() == row.max() == hi - 1 + over and ys.min() >= lo
                assert (ys[[0, 2]] < hi - 1).all()
            else:
                assert ys.min() == row.min() == lo - over and ys.max() < hi
                assert (ys[[0, 2]] > lo).all()


@pytest.mark.parametrize("kind", ["sum", "cap", "border"])
def test_i24_worst_case_stays_inside_int32(built, kind):
    """In Python integers: input 0 holds +-asafe on every tap of the heaviest filter with the weight's sign, its
    sum is the largest a 24-bit-form partial sum can be, and every prefix of every filter's sum fits int32."""
    c, M, xs, bad = built["i24_bound_" + kind]
    conv = c.layers[0]
    a = gc.conv_asafe(conv)
    w = [[int(v) for v in row] for row in conv.q_weights.reshape(conv.F, -1)]
    heavy = max(sum(abs(v) for v in row) for row in w)
    assert 0 < a <= gc.LIM24 and a * heavy <= I32_MAX
    assert a == gc.LIM24 or (a + 1) * heavy > I32_MAX
    assert (a == gc.LIM24) == (kind == "cap")
    cols, _, _ = gc._im2col(xs[0], conv.C, conv.H, conv.W, conv.kh, conv.kw, conv.sh, conv.sw, conv.ph, conv.pw)
    col = [int(v) for v in cols[:, 0]]  # the taps of output pixel (0, 0)
    worst = 0
    for row in w:
        s = 0
        for wk, xk in zip(row, col):
            s += wk * xk
            assert -(1 << 31) <= s <= I32_MAX
            worst = max(worst, abs(s))
    assert worst == a * heavy  # the bound is reached, on the border pixel too
    assert max(abs(v) for v in col) == a and int(np.abs(xs[0]).max()) == a
    assert int(np.abs(xs[1]).max()) == a + 1 and int(xs[1].max()) == a + 1 and int(xs[2].min()) == -(a + 1)
    if kind == "sum":
        assert worst > I32_MAX - heavy  # within one operand unit of the int32 end


def test_i24_wrapped_sum_is_a_false_refusal_unless_the_host_decides(built):
    """The table's claim about i24_wrapped_sum: the exact value passes, the value an int32 accumulator holds does
    not. And PendingCheck lets the host model decide an uncertain input whatever its device bit 0 says."""
    c, M, xs, bad = built["i24_wrapped_sum"]
    assert bad == []
    y = c.layers[0].plain_q_eval(xs[0], False, None, M)
    conv = c.layers[0]
    f = int(np.abs(conv.q_weights).reshape(conv.F, -1).sum(axis=1).argmax())
    exact = int(y[f]) - int(conv.q_biases[f])
    assert exact > I32_MAX and -M // 2 <= int(y[f]) < M // 2
    wrapped = exact - (1 << 32) + int(conv.q_biases[f])
    assert wrapped < -(M // 2)

    class Dev:  # a device that reports: input 0 uncertain and (spuriously) violating, input 1 clean, input 2 clean
        def wait(self, ticket):
            return [3, 0, 0]

    g = RangeGuard(c, M, mrs=True)
    assert PendingCheck(g, np.stack(xs), None, None, native=(Dev(), 0)).bad_indices() == []


def test_dense_int32_ends(built):
    c, M, xs, bad = built["dense_int32"]
    assert bad == []
    assert list(xs[0][:2]) == [I32_MAX, -(1 << 31)] and int(xs[1][1]) == 1 << 31 and int(xs[2][0]) == -(1 << 31) - 1
    w = np.abs(c.layers[0].q_weights).sum(axis=1).max()
    assert int(w) * (1 << 31) < 1 << 53  # the float64 torch path is exact on this case


def test_run_of_eight_splits_at_six_fused_ops(built):
    c, M, xs, bad = built["elem_run_of_eight"]
    spec = RangeGuard(c, M, mrs=True).native_spec()
    assert [(l["kind"], len(l["post"])) for l in spec["layers"]] == [(1, 6), (9, 2)]
    # an elementwise head carries its own op first
    c1, M1, _, _ = built["elem_halve3"]
    s1 = RangeGuard(c1, M1, mrs=True).native_spec()
    assert [(l["kind"], [o["kind"] for o in l["post"]]) for l in s1["layers"]] == [(9, [2])]
    assert s1["layers"][0]["post"][0]["c"] == 1 and s1["layers"][0]["post"][0]["l"] == 3


def test_add_strided_reads_a_wider_buffer(built):
    """The add's input holds 5 values in a buffer 50 wide, its residual comes from another buffer; the circuit
    input residual has stride N."""
    c, M, xs, bad = built["elem_add_strided"]
    spec = RangeGuard(c, M, mrs=True).native_spec()
    add = next(l for l in spec["layers"] if l["kind"] == 8)
    src_buf, res_buf = spec["ctx_buf"][add["src"]], spec["ctx_buf"][add["add_src"]]
    assert src_buf != res_buf and add["in_size"] == 5
    assert sorted((spec["buf_elems"][src_buf], spec["buf_elems"][res_buf])) == [5, 50]
    c2, M2, _, _ = built["elem_add_from_input"]
    add2 = next(l for l in RangeGuard(c2, M2, mrs=True).native_spec()["layers"] if l["kind"] == 8)
    assert add2["add_src"] == 0


def test_conv_table_covers_every_kernel_instance():
    """{3x3, 2x2, 1x1, generic} x {24-bit, 64-bit} x {padded, unpadded}, restated from DevRangeGuard::conv_kernel,
    and the shapes the table promises."""
    seen, px, fs = set(), set(), set()
    for name, (C, H, W, F, kh, kw, sh, sw, ph, pw, g, B, wts, tail) in gc.CONV_FORMS.items():
        conv = gc.CASES[name].build()[0].layers[0]
        k = (kh, kw) if (kh, kw) in ((3, 3), (2, 2), (1, 1)) else (0, 0)
        i24 = gc.conv_asafe(conv) > 0
        assert i24 == (wts != "big")
        seen.add((k, i24, ph > 0 or pw > 0))
        if wts == "env":
            seen.add((k, False, ph > 0 or pw > 0))
        px.add(conv.OH * conv.OW)
        fs.add(F // g)
    assert len(seen) == 16
    assert {1, 63, 64, 65} <= px and {1, 7, 8, 9, 17, 10} <= fs


def test_simulate_spec_conv_groups_match_the_layer():
    """The interpreter's grouped conv against Conv2d.plain_q_eval (its einsum ignored the groups before)."""
    c, M, xs, _ = gc.CASES["c22_env_groups_fg10"].build()
    spec = RangeGuard(c, M, mrs=True).native_spec()
    assert spec["layers"][0]["g"] == 2
    _, out = gc.simulate_spec(spec, xs)
    np.testing.assert_array_equal(out, np.stack([c.plain_q_eval(x, False, M) for x in xs]))


def test_zoo_rows_fit_the_int64_accumulator():
    """The 64-bit forms hold sum_k |w_k| * 2^31 in int64 only while a row's sum_k |w_k| < 2^32 (guard.hip header):
    every linear layer of the model zoo is far below that, so the guard refuses no layer for it."""
    from dash_amd.ir import layers as L
    from dash_amd.ir.quant import QuantizationMethod
    from dash_amd.models import BENCH_CONFIGS, build_circuit

    for key, cfg in BENCH_CONFIGS.items():
        c = build_circuit(key.split("/")[0], QuantizationMethod(cfg["q_method"]), cfg["q_parameter"], seed=0)
        for l in c.layers:
            if isinstance(l, (L.Conv2d, L.Dense)):
                rows = np.abs(np.asarray(l.q_weights, dtype=np.int64)).reshape(l.q_weights.shape[0], -1).sum(axis=1)
                assert int(rows.max()) < 1 << 32 and int(np.abs(l.q_biases).max()) < 1 << 62, key
