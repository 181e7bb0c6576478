"""DevRangeGuard (dash_amd/csrc/hip/guard.hip) on the device against the exact model, at the edges of
tests/guard_cases.py (validated on the CPU by test_guard_cases.py): raw flag bits, the activations read back
through the peek_output test hook, the public bad_indices() and the torch path on the device, all by exact integer
equality. Then tickets, chunks and captured graphs on one small conv -> rescale -> ReLU circuit."""
import numpy as np
import pytest

from dash_amd.garbling import RangeGuard
from tests import guard_cases as gc

pytestmark = pytest.mark.gpu


def _device_run(c, M, xs):
    """(raw flags, read-back of all inputs, the guard): one submit / wait through the raw DevRangeGuard."""
    g = RangeGuard(c, M, mrs=True, device=0)
    assert g._native_ok()
    dev = g._native()
    X = np.stack(xs)
    assert len(xs) <= dev.chunk()
    f = np.asarray(dev.wait(dev.submit(X)))
    out = dev.peek_output(len(xs))
    assert out.dtype == np.int64 and out.shape == (len(xs), c.output_size)
    return f, out, g


def _check(name, c, M, xs, bad, uncertain):
    f, out, g = _device_run(c, M, xs)
    assert f.shape == (len(xs),) and not (f & ~3).any()
    # bit 1: exactly the inputs the table says exceed a linear layer's operand range
    assert [int(i) for i in np.nonzero(f & 2)[0]] == list(uncertain), (name, f)
    for i, x in enumerate(xs):
        if i in uncertain:
            continue
        # bit 0 equals the exact model's flag; the activations of a passing input are the plaintext ones
        assert bool(f[i] & 1) == (i in bad), (name, i, f)
        if i not in bad:
            np.testing.assert_array_equal(out[i], c.plain_q_eval(x, False, M), err_msg="%s input %d" % (name, i))
    assert g.submit(xs).bad_indices() == bad, name
    return f, out


@pytest.mark.parametrize("name", gc.NAMES)
def test_case_on_device(name, monkeypatch):
    monkeypatch.delenv("DASH_GUARD_I24", raising=False)
    case = gc.CASES[name]
    c, M, xs, bad = case.build()
    f, out = _check(name, c, M, xs, bad, case.uncertain)
    # the torch path on the device gives the same flags
    gt = RangeGuard(c, M, mrs=True, device=0)
    gt.native_forms = False
    assert not gt._native_ok()
    assert sorted(gt.submit(xs).bad_indices()) == bad
    if case.env:  # the 64-bit product form of the same small-weight layer: the same flags and activations
        monkeypatch.setenv("DASH_GUARD_I24", "0")
        f64, out64 = _check(name, c, M, xs, bad, case.uncertain)
        np.testing.assert_array_equal(f64, f)
        np.testing.assert_array_equal(out64, out)


# ------------------------------------------------------------------------------------ tickets, chunks, graphs
@pytest.fixture(scope="module")
def tk():
    c = gc.ticket_circuit()
    g = RangeGuard(c, gc.M6, mrs=True)
    return c, g, g.native_spec()


def _dev(native, spec, chunk=None):
    args = (0, spec["layers"], spec["input_size"], spec["ctx_buf"], spec["buf_elems"], spec["out_lo"], spec["out_hi"])
    return native.DevRangeGuard(*args) if chunk is None else native.DevRangeGuard(*args, chunk)


def _expect(tk, xs):
    c, g, _ = tk
    return np.array([1 if g.violations_np(x) else 0 for x in xs])


def _outs(tk, xs):
    return gc.simulate_spec(tk[2], xs)[1]  # exact for refused inputs too (int64, no wrap at these sizes)


def test_chunk_of_two_one_hot_and_partial_last_chunk(native, tk):
    dev = _dev(native, tk[2], chunk=2)
    assert dev.chunk() == 2
    for i in range(5):
        xs = gc.ticket_inputs(tk[0], 5, bad=(i,), seed=i)
        want = _expect(tk, xs)
        assert list(np.nonzero(want)[0]) == [i]
        f = np.asarray(dev.wait(dev.submit(np.stack(xs))))
        np.testing.assert_array_equal(f, want)
        np.testing.assert_array_equal(dev.peek_output(1), _outs(tk, xs)[4:])  # the last chunk holds input 4 alone
    with pytest.raises(RuntimeError, match="peek_output"):
        dev.peek_output(3)  # more rows than a chunk holds: refused before anything is read


def test_default_chunk_boundaries(native, tk):
    dev = _dev(native, tk[2])
    ch = dev.chunk()
    assert ch == 64
    for B in (ch, ch + 1, 2 * ch):
        xs = gc.ticket_inputs(tk[0], B, bad=sorted({0, ch - 1, B - 1}), seed=B)
        want = _expect(tk, xs)
        assert want.sum() == len({0, ch - 1, B - 1})
        f = np.asarray(dev.wait(dev.submit(np.stack(xs))))
        np.testing.assert_array_equal(f, want)
        last = B - (B - 1) // ch * ch
        np.testing.assert_array_equal(dev.peek_output(last), _outs(tk, xs)[B - last:])


def test_more_batch_sizes_than_graphs_on_one_ticket(native, tk):
    """Ten batch sizes on one ticket pass the eight-graph limit (the graphs are dropped and captured again); the
    first size again, with other inputs, reads the new inputs."""
    dev = _dev(native, tk[2])
    for rep, sizes in enumerate((range(1, 11), (1, 2))):
        for B in sizes:
            xs = gc.ticket_inputs(tk[0], B, bad=(B - 1 - rep,) if B > rep else (), seed=100 * rep + B)
            f = np.asarray(dev.wait(dev.submit(np.stack(xs))))
            np.testing.assert_array_equal(f, _expect(tk, xs))
            np.testing.assert_array_equal(dev.peek_output(B), _outs(tk, xs))


def test_batch_beyond_the_tickets_capacity(native, tk):
    dev = _dev(native, tk[2])
    for B, bad in ((3, (1,)), (7, (6,)), (70, (0, 64, 69)), (3, (2,))):  # capacity 64, then 70
        xs = gc.ticket_inputs(tk[0], B, bad=bad, seed=B + len(bad))
        want = _expect(tk, xs)
        assert list(np.nonzero(want)[0]) == list(bad)
        f = np.asarray(dev.wait(dev.submit(np.stack(xs))))
        np.testing.assert_array_equal(f, want)
        last = B - (B - 1) // 64 * 64
        np.testing.assert_array_equal(dev.peek_output(last), _outs(tk, xs)[B - last:])


def test_three_tickets_waited_in_reverse(native, tk):
    dev = _dev(native, tk[2])
    batches = [gc.ticket_inputs(tk[0], B, bad=(i,), seed=40 + i) for i, B in enumerate((4, 6, 5))]
    tickets = [dev.submit(np.stack(xs)) for xs in batches]
    assert len(set(tickets)) == 3
    for t, xs in reversed(list(zip(tickets, batches))):
        np.testing.assert_array_equal(np.asarray(dev.wait(t)), _expect(tk, xs))
    np.testing.assert_array_equal(dev.peek_output(5), _outs(tk, batches[2]))  # the last chunk that ran


def test_stream_launches_equal_the_graph(native, tk, monkeypatch):
    xs = gc.ticket_inputs(tk[0], 9, bad=(2, 8), seed=7)
    res = []
    for graph in ("1", "0"):
        monkeypatch.setenv("DASH_GUARD_GRAPH", graph)
        dev = _dev(native, tk[2], chunk=4)
        for _ in range(2):  # the second submit replays the captured graph (or launches again)
            f = np.asarray(dev.wait(dev.submit(np.stack(xs))))
        res.append((f, dev.peek_output(1)))
    np.testing.assert_array_equal(res[0][0], _expect(tk, xs))
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], _outs(tk, xs)[8:])
    np.testing.assert_array_equal(res[0][1], res[1][1])
