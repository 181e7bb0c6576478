"""Every launch-size-dependent form of the mixed-radix gadget kernels, forced with the planning CU count.

A gadget launch picks one of several hand-written kernels for the same operation by comparing the launch with
the chip's CU count (mrs_chain.h launch_mrs_chain_k, kernels_gadget.hip launch_rescale_mrs /
launch_rescale_relu_out / launch_relu_mult / launch_rescale_update_approx, gadget_common.h aes_bs / grid_aes).
The parity tests' shapes reach only the small-launch forms; here ``hip_set_planning_cus`` plans a small launch as
the 165-GC headline is planned (count 1: staged forms, 512-lane blocks, capped grids, strided loops) and as
batch-1 latency is planned (count 1 << 20: quad forms, 64-lane blocks), and count 0 pins the device's own picks.

Each case asserts three things:
  * form: the launch log of the eager run is exactly the list of forms, grids and blocks that the pickers' rules
    (restated below in Python) give for the case, and for counts 1 and 1 << 20 also the forms written out by hand;
  * host oracle: the labels are bit-identical to GarbledCircuit.cpu_evaluate;
  * plain reference: the decoded integers equal plain_q_eval and a NumPy int64 closed form.

Circuits (host garbler, one seed per GC): R = Rescale(l) with the mixed-radix rescale (chain mode 0), S = Relu with
the exact mixed-radix sign (mode 1), J = Rescale(l) + Relu joint (mode 2), A = Rescale(2) + Relu with the reference
constructions (the AES-family kernels; these exist only in the reference encoding, so A is not hardened).
"""
import numpy as np
import pytest

import dash_amd as d
from dash_amd.garbling import GarbledCircuit

pytestmark = pytest.mark.gpu

BIG = 1 << 20
SIZES = [512, 528, 1040, 2064, 1031]  # full tile; m * 512 + 16 (16 live lanes in the last tile); prime
EDGE_AT = [0, 15, 16, 63, 64, 255, 256, 511, 512, -17, -16, -1]  # tile / wave / 16-byte row boundaries


def _ceil(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------ circuits
def _mrs_arg(k):
    # the approximate sign's MRS base: none below k = 4 (the parity tests' convention) and none exists for
    # k = 12; the mixed-radix constructions do not use it
    return 100.0 if 4 <= k <= 11 else None


def _shift(kind, k):
    if kind.startswith("A"):
        return 2
    return 1 if k <= 3 else (2 if k <= 5 else 5)  # 2^l well below M = 6, 30, 210, 2310, then the headline's l


def _inputs(kind, k, N):
    """x for GC 0: random over the operation's domain, every edge value somewhere, and the cardinal edges on the
    element indices where a tile, a wave or a 16-byte row starts or ends."""
    M = GarbledCircuit(d.Circuit([d.Relu((1,))]), k, _mrs_arg(k), garble_me=False).crt_modulus
    S, h = 1 << _shift(kind, k), M // 2
    hi = h if kind == "S" else h - S  # the rescale's non-wrapping domain [-h, h - S)
    rng = np.random.default_rng(1000 * k + N)
    x = rng.integers(-h, hi, N).astype(np.int64)
    edges = [0, 1, -1, -h, h - S - 1] + list(range(-2 * S - 2, 2 * S + 3)) + ([h - 1] if kind == "S" else [])
    edges = [v for v in edges if -h <= v < hi]
    x[70:70 + len(edges)] = edges
    cardinal = [-h, hi - 1, 0, -1, 1, -S, S, -S - 1, S + 1, -2 * S - 2, 2 * S + 2, -S + 1]
    cardinal = [v for v in cardinal if -h <= v < hi]
    for n, i in enumerate(EDGE_AT):
        if -N <= i < N:
            x[i] = cardinal[n % len(cardinal)]
    return x, S


def _build(kind, k, N):
    l = _shift(kind, k)
    if kind == "R":
        layers, kw = [d.Rescale(l, (N,))], dict(rescale="mrs")
    elif kind == "S":
        layers, kw = [d.Relu((N,))], dict(relu="mrs")
    elif kind == "J":
        layers, kw = [d.Rescale(l, (N,)), d.Relu((N,))], dict(rescale="mrs", relu="joint")
    else:
        layers = [d.Rescale(l, (N,)), d.Relu((N,))]
        kw = dict(rescale="legacy", relu="approx", fused_sign=kind == "A-fused", hardened=False)
    x, S = _inputs(kind, k, N)
    xs = [x, x[::-1].copy(), np.roll(x, 7)]  # a permutation per GC: a wrong batch stride cannot cancel out
    c = d.Circuit(layers)
    gcs = [GarbledCircuit(c, k, _mrs_arg(k), seed=bytes([k, i + 1]) * 8, **kw) for i in range(3)]
    assert all(g.hardened == (not kind.startswith("A")) for g in gcs)
    enc = [g.garble_inputs(v) for g, v in zip(gcs, xs)]
    cpu = [g.cpu_evaluate(e) for g, e in zip(gcs, enc)]
    plain = [g.plain_q_eval(v) for g, v in zip(gcs, xs)]
    ceil = [-((-v) // S) for v in xs]
    closed = {"R": ceil, "S": [np.maximum(v, 0) for v in xs]}.get(kind, [np.maximum(v, 0) for v in ceil])
    for p, c0 in zip(plain, closed):
        np.testing.assert_array_equal(p, c0)
    return dict(gcs=gcs, enc=enc, cpu=cpu, closed=closed, crt=gcs[0].crt_base)


_BUILT = {}


def _circuit(kind, k, N):
    """Garbled once per (circuit, k, N) and module, shared by every planning count and batch size."""
    key = (kind, k, N)
    if key not in _BUILT:
        _BUILT[key] = _build(kind, k, N)
    return _BUILT[key]


# ------------------------------------------------------------------------------------- the pickers, restated
def _aes_bs(n, y, z, cus):
    bs = 512
    while bs > 64 and n * y * z < bs * cus:
        bs //= 2
    return bs


def _grid_aes(n, bs, y, z, cus):
    resident = max(1, min(6 * 256 // bs, 5))  # 6 waves per SIMD; five 32 KiB AES images in 160 KiB of LDS
    return min(_ceil(n, bs), max(1, 4 * resident * cus // (y * z)))


def _line(form, grid, block):
    return "%s grid=(%d,%d,%d) block=%d" % (form, grid[0], grid[1], grid[2], block)


def _aes(name, n, y, z, cus):
    bs = _aes_bs(n, y, z, cus)
    return _line("aes." + name, (_grid_aes(n, bs, y, z, cus), y, z), bs)


def _chain(native, crt, mode, N, B, cus):
    k = len(crt)
    head = "K=%d mode=%d" % (k, mode)
    staged = N % 16 == 0 and N >= 512 and _ceil(N, 512) * B >= 2 * cus
    lds = sum(native.nr_comps(p) for p in crt) * 256
    if not staged and not (N % 16 != 0 and N > 256) and _ceil(N, 256) * B <= cus and lds <= 160 << 10:
        return _line("chain.quad " + head, (_ceil(N, 64), 1, B), 256)
    if staged:
        return _line("chain.staged " + head, (_grid_aes(N, 512, 1, B, cus), 1, B), 512)
    bs = _aes_bs(N, 1, B, cus)
    return _line("chain.lane " + head, (_grid_aes(N, bs, 1, B, cus), 1, B), bs)


def _relu_mult(k, N, B, cus):
    if N % 16 == 0 and N >= 256:
        return _line("relu_mult.staged", (min(_ceil(N, 256), max(1, 16 * cus // (k * B))), k, B), 256)
    return _line("relu_mult.lane", (_ceil(N, 256), k, B), 256)


def _expected(native, kind, crt, N, B, cus):
    k = len(crt)
    quad_out = _ceil(N, 256) * k * B <= cus
    if kind == "R":
        out = _line("mrs_out.quad", (_ceil(N, 64), k, B), 256) if quad_out else _line("mrs_out.lane", (_ceil(N, 256), k, B), 256)
        return [_chain(native, crt, 0, N, B, cus), out]
    if kind == "S":
        return [_aes("k_label_hash", N, k, B, cus), _chain(native, crt, 1, N, B, cus), _relu_mult(k, N, B, cus)]
    if kind.startswith("A"):
        # legacy rescale by 4 = two sign-base-extension steps (hash of the factor residue, update + approximate
        # sign, carry chain), then the approximate-sign ReLU (k = 7: at most 5 sign digits)
        ua = _aes("update_approx.small" if N * k * B <= 512 * cus else "update_approx.large", N, k, B, cus)
        sc = _aes("k_sign_chain_fused" if kind == "A-fused" else "k_sign_chain", N, 1, B, cus)
        return [_aes("k_rescale_hash", N, 1, B, cus), ua, sc, _aes("k_rescale_hash_sign", N, 1, B, cus), ua, sc,
                _aes("k_sign_approx<5>", N, k, B, cus), sc, _relu_mult(k, N, B, cus)]
    assert kind == "J"
    if B <= 2:  # the fused output kernel
        if quad_out:
            out = _line("relu_out.quad", (_ceil(N, 64), k, B), 256)
        elif N % 16 == 0 and N >= 256:
            out = _line("relu_out.staged", (_ceil(N, 256), k, B), 256)
        else:
            out = _aes("relu_out.lane", N, k, B, cus)
        return [_chain(native, crt, 2, N, B, cus), out]
    if N % 16 == 0 and N >= 512:
        out = _line("out_hash.staged", (_grid_aes(N, 512, k, B, cus), k, B), 512)
    else:
        out = _aes("out_hash.lane", N, k, B, cus)
    return [_chain(native, crt, 2, N, B, cus), out, _relu_mult(k, N, B, cus)]


def _parse(line):
    form, g, b = line.rsplit(" ", 2)
    return form, tuple(int(v) for v in g[len("grid=("):-1].split(",")), int(b[len("block="):])


def _find(log, prefix):
    hits = [_parse(ln) for ln in log if ln.startswith(prefix)]
    assert hits, "no %r launch in %s" % (prefix, log)
    return hits


def _by_hand(kind, N, B, count, log):
    """The forms at k = 7 written out (not derived from the rules above): counts 1 and 1 << 20, and the device's
    own picks (count 0) on a 256-CU part."""
    full = N % 16 == 0
    aes = [_parse(ln) for ln in log if ln.startswith("aes.")]
    if count == 1:
        assert all(b == 512 for _, _, b in aes), log
        # k * B >= 14 blocks in y, z against a cap of 12: one block in x walks every tile
        assert all(g[0] == 1 for _, g, _ in aes if g[1] > 1), log
        if not kind.startswith("A"):
            (form, g, b), = _find(log, "chain.")
            assert form.startswith("chain.staged" if full else "chain.lane") and b == 512, log
            assert g[0] == min(_ceil(N, 512), 12 // B), log
            if N == 2064 and B == 3:
                assert g[0] == 4 < _ceil(N, 512), log  # a block walks more than one tile
        if kind == "R":
            assert _find(log, "mrs_out.")[0][0] == "mrs_out.lane", log
        if kind == "J" and B == 2:
            assert _find(log, "relu_out." if full else "aes.relu_out.")[0][0] == ("relu_out.staged" if full else "aes.relu_out.lane"), log
        if kind == "J" and B == 3:
            form, g, b = _find(log, "out_hash." if full else "aes.out_hash.")[0]
            assert form == ("out_hash.staged" if full else "aes.out_hash.lane") and g[0] == 1 and b == 512, log
        if kind == "S" or (kind == "J" and B == 3) or kind.startswith("A"):
            form, g, b = _find(log, "relu_mult.")[-1]
            assert form == ("relu_mult.staged" if full else "relu_mult.lane"), log
            if full:
                assert g[0] == 1 < _ceil(N, 256), log  # capped grid: a block walks every 256-element tile
        if kind.startswith("A"):
            assert any(f.startswith("aes.update_approx.large") for f, _, _ in aes), log
            if N == 2064 and B == 3:  # the (x, 1, B) kernels: 5 tiles on 4 blocks
                assert any(g == (4, 1, 3) for _, g, _ in aes), log
    elif count == BIG:
        assert all(b == 64 and g[0] == _ceil(N, 64) for _, g, b in aes), log
        if not kind.startswith("A"):
            (form, g, b), = _find(log, "chain.")
            if full:
                assert form.startswith("chain.quad") and g[0] == _ceil(N, 64) > 1 and b == 256, log
            else:
                assert form.startswith("chain.lane") and b == 64, log
        if kind == "R":
            assert _find(log, "mrs_out.")[0][0] == "mrs_out.quad", log
        if kind == "J" and B == 2:
            assert _find(log, "relu_out.")[0][0] == "relu_out.quad", log
        if kind == "J" and B == 3 and full:
            form, g, b = _find(log, "out_hash.")[0]
            assert form == "out_hash.staged" and g[0] == _ceil(N, 512), log
            form, g, b = _find(log, "relu_mult.")[0]
            assert form == "relu_mult.staged" and g[0] == _ceil(N, 256), log
        if kind.startswith("A"):
            assert any(f.startswith("aes.update_approx.small") for f, _, _ in aes), log
    else:
        # the device's own picks on a 256-CU MI355X: every launch here is below one block per CU, so the latency
        # forms, with AES blocks of 64 lanes (128 once N * k * B reaches 128 * 256) and no second trip anywhere
        for _, g, b in aes:
            assert b == (128 if N * g[1] * g[2] >= 128 * 256 else 64) and g[0] == _ceil(N, b), log
        if not kind.startswith("A"):
            (form, g, b), = _find(log, "chain.")
            assert form.startswith("chain.quad" if full else "chain.lane") and g[0] == _ceil(N, 64), log
        if kind == "R":
            assert _find(log, "mrs_out.")[0][0] == "mrs_out.quad", log
        if kind == "J" and B == 2:
            assert _find(log, "relu_out.")[0][0] == "relu_out.quad", log
        if kind == "J" and B == 3:
            assert _find(log, "out_hash." if full else "aes.out_hash.")[0][1][0] == _ceil(N, 512 if full else 64), log
        if kind != "R" and not (kind == "J" and B == 2):
            form, g, b = _find(log, "relu_mult.")[0]
            assert form == ("relu_mult.staged" if full else "relu_mult.lane") and g[0] == _ceil(N, 256), log
        if kind.startswith("A"):
            assert any(f.startswith("aes.update_approx.small") for f, _, _ in aes), log


def _check_forms(native, kind, crt, N, B, count, log):
    cus = count if count else native.hip_planning_cus()  # count 0: the device's CU count (a regression pin)
    assert log == _expected(native, kind, crt, N, B, cus)
    if len(crt) == 7 and (count or cus == 256):
        _by_hand(kind, N, B, count, log)


# --------------------------------------------------------------------------------------------------- the check
def _run(native, kind, k, N, B, count):
    from dash_amd.runtime import HipEvaluator

    c = _circuit(kind, k, N)
    gcs = c["gcs"][:B]
    native.hip_launch_log_take()
    native.hip_set_planning_cus(count)
    try:
        ev = HipEvaluator([g.model for g in gcs])  # fresh: an evaluator's picks freeze at graph capture
        native.hip_launch_log(True)
        try:
            gpu = ev.evaluate(c["enc"][:B])  # the first run of an evaluator is eager
        finally:
            native.hip_launch_log(False)
        log = native.hip_launch_log_take()
    finally:
        native.hip_set_planning_cus(0)
    print("\n".join(log))
    _check_forms(native, kind, c["crt"], N, B, count, log)
    for want, got in zip(c["cpu"], gpu):
        assert len(want) == len(got)
        for (pw, aw), (pg, ag) in zip(want, got):
            assert pw == pg
            np.testing.assert_array_equal(aw, ag)
    for g, o, ref in zip(gcs, gpu, c["closed"]):
        np.testing.assert_array_equal(g.decode_outputs(o), ref)  # == plain_q_eval (checked in _build)


@pytest.mark.parametrize("count", [1, 0, BIG], ids=["cus1", "device", "cus1M"])
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("kind", ["R", "S", "J", "A-fused", "A-refcasts"])
def test_forms_k7(native, kind, N, B, count):
    _run(native, kind, 7, N, B, count)


@pytest.mark.parametrize("kind", ["R", "S", "J"])
@pytest.mark.parametrize("k", [2, 3, 4, 5, 6, 8, 9, 10, 11, 12])
def test_staged_forms_every_k(native, kind, k):
    """The per-K chain units instantiate every form separately: the staged form of each K (k = 7 is in the grid)."""
    _run(native, kind, k, 528, 2, 1)


_POW2_BASE, _POW2_MRS = [32, 97, 107], [22, 19, 15, 13]  # M = 332128: residue 32 of the ReDash optimized bases


def _pow2_circuit(N):
    """Relu over a base whose first residue is a power of two above 2 (the multiply walks' digit-stream branch,
    ModC bits = 5; the first-k-primes bases of the cases above have only p = 2 and odd residues): the hardened
    default with the approximate sign, 2 GCs, a permuted input per GC."""
    key = ("pow2", N)
    if key not in _BUILT:
        c = d.Circuit([d.Relu((N,))])
        gcs = [GarbledCircuit(c, _POW2_BASE, _POW2_MRS, seed=bytes([32, i + 1]) * 8) for i in range(2)]
        M = gcs[0].crt_modulus
        assert M == 332128 and all(g.hardened for g in gcs)
        # uniform over [-M/8, M/8): there the approximate sign is exact for every element (the host evaluator
        # equals max(x, 0) below, no element excluded)
        x = np.random.default_rng(32 + N).integers(-(M // 8), M // 8, N).astype(np.int64)
        small = [0, 1, -1, 2, -2]
        x[70:75] = small
        for n, i in enumerate(EDGE_AT):
            if -N <= i < N:
                x[i] = small[n % len(small)]
        xs = [x, x[::-1].copy()]
        enc = [g.garble_inputs(v) for g, v in zip(gcs, xs)]
        cpu = [g.cpu_evaluate(e) for g, e in zip(gcs, enc)]
        closed = [np.maximum(v, 0) for v in xs]
        for g, v, o, ref in zip(gcs, xs, cpu, closed):
            np.testing.assert_array_equal(g.plain_q_eval(v), ref)
            np.testing.assert_array_equal(g.decode_outputs(o), ref)
        _BUILT[key] = dict(gcs=gcs, enc=enc, cpu=cpu, closed=closed)
    return _BUILT[key]


@pytest.mark.parametrize("N,form", [(528, "relu_mult.staged"), (1031, "relu_mult.lane")])
def test_relu_mult_power_of_two_residue(native, N, form):
    from dash_amd.runtime import HipEvaluator

    c = _pow2_circuit(N)
    native.hip_launch_log_take()
    native.hip_set_planning_cus(1)
    try:
        ev = HipEvaluator([g.model for g in c["gcs"]])
        native.hip_launch_log(True)
        try:
            gpu = ev.evaluate(c["enc"])
        finally:
            native.hip_launch_log(False)
        log = native.hip_launch_log_take()
    finally:
        native.hip_set_planning_cus(0)
    print("\n".join(log))
    want_line = _relu_mult(len(_POW2_BASE), N, 2, 1)
    assert want_line.startswith(form) and want_line in log
    for want, got in zip(c["cpu"], gpu):
        assert len(want) == len(got)
        for (pw, aw), (pg, ag) in zip(want, got):
            assert pw == pg
            np.testing.assert_array_equal(aw, ag)
    for g, o, ref in zip(c["gcs"], gpu, c["closed"]):
        np.testing.assert_array_equal(g.decode_outputs(o), ref)  # == plain_q_eval == max(x, 0) (_pow2_circuit)


def test_planning_count_restores(native):
    dev = native.hip_planning_cus()
    assert native.hip_planning_override() == 0 and dev >= 1
    native.hip_set_planning_cus(1)
    try:
        assert native.hip_planning_cus() == 1 and native.hip_planning_override() == 1
    finally:
        native.hip_set_planning_cus(0)
    assert native.hip_planning_cus() == dev and native.hip_planning_override() == 0
    with pytest.raises(Exception, match=">= 0"):
        native.hip_set_planning_cus(-1)
    assert native.hip_planning_cus() == dev


def test_launch_log_off_by_default(native):
    from dash_amd.runtime import HipEvaluator

    c = _circuit("R", 7, 512)
    native.hip_launch_log_take()
    HipEvaluator([c["gcs"][0].model]).evaluate(c["enc"][:1])
    assert native.hip_launch_log_take() == []
