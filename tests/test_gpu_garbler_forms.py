"""The GPU garbler's kernel forms against the host garbler, at the edges (cases: tests/garbler_cases.py).

The device garbler (csrc/hip/garble_gpu.hip) must be byte-identical to the host garbler (csrc/garbler.cpp). Every
case here compares digests of the serialized offline message and decoder for one seed, and reads from the garbler's
launch record (native.hip_garbler_log / hip_garbler_log_take, csrc/hip/gpu_garbler.h) which path the case took.

Forms and what selects them (docs/GARBLER_FORMS.md has the full list):
  * element tails of the 64-lane tiles (k_draw, k_hash*, k_bank) and of k_emit's te = 1 << tsh tiles: N = 1, 63, 64,
    65, 257 for every gadget kind, in every encoding and sign construction the kind resolves under;
  * compress_xa classes by modulus: g8 (q <= 8), g4 (q <= 64), rt3 (65 <= q < 256, not a power of two): first-prime
    bases of 2, 3, 7, 8 and 9 residues and the three ReDash bases of BENCH_CONFIGS;
  * label blocks reused from the per-stream cache with another modulus' contents: test_order_dependence;
  * the process-wide A/B forms (DASH_GG_KEYS, DASH_GG_HASH, DASH_GG_FUSED, DASH_GG_AES_COPIES, DASH_GG_EMIT_LDS_KB,
    DASH_GG_DRAW_BLOCKS): one fresh child process each, test_process_wide_form.

Not covered, and why:
  * compress class pw2 (compress_xa_t<true>, compress_xa2_t<true>): of the moduli the GPU path takes (below 256,
    kargs.h) only q = 128 maps to it (powers of two up to 64 take g8 / g4), and no CRT or MRS base of BENCH_CONFIGS
    or of any case holds 128. The coverage assertion computes the required classes from the cases' own moduli, so
    it asks for pw2 as soon as a case brings such a base.
  * k_emit at tsh = 0 (one element per block): the cases reach tsh 1 to 5 at the default LDS budget and no scope
    of the short list drops to 0 under DASH_GG_EMIT_LDS_KB = 8 (minimum 1).
  * the approximate sign at k = 2 and k = 3: refused by the host garbler without an MRS base (garbler_cases.py).
  * the compile-time knobs DASH_GG_PB, DASH_GG_ALIGNED_GROUPS and DASH_GG_HASH_PAIRS need a rebuild.

Capped grids of the existing whole-model cases. `minionn_head` in test_gpu_parity.py::test_gpu_garbler_bit_identical*
garbles the first conv's 64 x 30 x 30 = 57600 elements per gadget at k = 7 (and 50176 behind the second conv). The
block counts follow from the launch formulas (blocks_for in garble_gpu.hip; lanes = N rounded up to 64 = 57600):
k_bank lanes x bank jobs / 256, k_hash_iu lanes x hash jobs / 512, k_draw lanes x draws / 512, k_emit the sum over
scopes of ceil(N / 2^tsh), k_rescale_post_g N x 128 / 256, k_bin_keys and k_rescale_pre N / 512, k_relu_finish
N / 256. A grid below its block count wraps and the kernel strides. Largest block count of any launch per case, as
the launch record gives them (test_minionn_head_wraps asserts the [fused] column's wraps and non-wraps):

  launch (cap)              [fused]  [refcasts]  mrs_rescale  mrs_relu  joint_relu   wraps
  k_bank (32768)             40500     63900       47025       47025     46800       in every case
  k_emit (65536)             36000     79200       36000       18000     21600       [refcasts] only
  k_rescale_post_g (4096)    28800     28800         -           -         -         the legacy rescale's cases
  k_hash_iu (16384)           5175      8775        5175        2138      2138       no
  k_draw (16384)              4500      8100        4500        3938      3938       no
  k_bin_keys (8192)            113       113         113         113       113       no
  k_rescale_pre (2048)         113       113         -           -         -         no
  k_relu_finish (4096)         225       225         225         225       225       no
  k_iR (1024)                    5         5           5           3         3       no

Uncovered: no whole-model case wraps k_hash_iu, k_bin_keys, k_rescale_pre, k_relu_finish or k_iR, and nothing in
the tree asserts a wrap of them (k_hash_iu would need about twice minionn_head's lanes x hash jobs, the N / 512 and
N / 256 grids millions of elements in one gadget; k_iR's grid is p x words / 256 blocks for the largest modulus p of
a projection set, words = 4 x chunks(p) <= 64, so its cap of 1024 needs p x words above 262144: no modulus below
32768, the largest that gets multiple rows, reaches it with fewer than 8 words, and those have at most 4). k_hash_jobs and
k_hash (16384) run only under DASH_GG_KEYS / DASH_GG_HASH, here at N = 65: never wrapped. k_lin, k_gsum (8192) and
k_clip_u, k_clip_finish (4096) are not launched by minionn_head; the pooling, Mul, PWL and Clip cases of the tree
are far below N x chunks / 256 = their caps. The draw grid wraps only under DASH_GG_DRAW_BLOCKS = 1
(test_process_wide_form[draw1], N = 65). The other caps have no knob, and adding one is out of scope.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import garbler_cases as gcs

pytestmark = pytest.mark.gpu

CASES = gcs.all_cases()
BY_NAME = {c.name: c for c in CASES}
_RUNS = {}  # case name -> (same, parsed record): each case garbles once per process


def _run(case, native):
    if case.name not in _RUNS:
        same, lines, _ = gcs.device_vs_host(case, native)
        _RUNS[case.name] = (same, gcs.parse_log(lines))
    return _RUNS[case.name]


def _projects(recs):
    return [r for r in recs if r["what"] == "project"]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_device_garbler_matches_host(case, native):
    """Byte identity, and the path: exactly the case's gadget entry points with its N and k, every projection set on
    the default key path (uniform-i hashes, hardened or not as the case's encoding says)."""
    same, recs = _run(case, native)
    print("\n".join(str(r) for r in recs))
    assert same, f"{case.name}: the device garbler's bytes differ from the host garbler's"
    entries = [r for r in recs if r["what"] == "entry"]
    assert {r["name"] for r in entries} == set(case.entries), entries
    if case.gadget_n:
        assert tuple(r["N"] for r in entries) == case.gadget_n, entries
        assert {r["k"] for r in entries} == {len(case.bases()[0])}, entries
    pro = _projects(recs)
    if case.kind not in ("dense", "dense_tf"):
        assert pro, "a gadget case without a projection set"
    for p in pro:
        assert p["keys"] == "iu" and p["by_i"] == 1 and p["hard"] == int(case.hardened), p
        assert p["hash"] == ("k_hash_iu<16,hard>" if case.hardened else "k_hash_iu<32>"), p
        assert len(p["tsh"]) == p["scopes"] and all(0 <= t <= 5 for t in p["tsh"]), p
        assert p["emit_blocks"] == sum(-(-p["N"] // (1 << t)) for t in p["tsh"]), p
    for r in recs:
        if r["what"] in ("launch", "draw"):
            assert 1 <= r["grid"] == min(r["blocks"], r["cap"]), r


EVAL = sorted({c.kind: c.name for c in reversed(CASES) if c.N == 65 or c.kind == "dense_tf"}.values())


@pytest.mark.parametrize("name", EVAL)
def test_device_garbled_model_evaluates(name, native):
    """One size per kind: the device-garbled model loads into a HipEvaluator and decodes to the plaintext result."""
    from dash_amd.runtime import HipEvaluator

    case = BY_NAME[name]
    same, _, g = gcs.device_vs_host(case, native, keep=True)
    assert same
    x = case.inputs(seed=9)
    ev = HipEvaluator(template=g.model, batch=1, device=0)
    ev.load(0, g.model)
    ev.encode_compressed_into(0, g, x)
    ev.upload_inputs_compressed()
    ev.run()
    ev.fetch_outputs()
    np.testing.assert_array_equal(ev.decode(0, g), g.plain_q_eval(x))


def test_order_dependence(native):
    """Label blocks come from a per-stream cache keyed by byte size (cache_get), and a block keeps what the earlier
    garbling left in it. A chunked label of modulus q takes N x chunks(q) x 16 bytes (chunks = ceil(nr_comps(q) / 8)),
    and the device conv writes only the nr_comps(q) real components of its output labels (k_chunk_res), so the
    padding components of a conv's output keep the block's earlier contents; the gadget behind the conv then reads
    that label as its input (compress_xa must count the padding as 0). The three circuits (garbler_cases.order_cases)
    are sized so that one block size is shared by labels of very different shapes:

      A  Rescale(1) + joint ReLU, base [2, 3], N = 48:
           q = 2, 16 chunks, no padding: 48 x 256 = 12288 B of random bits in every component
      B  conv 1x1 + Rescale([32]) + ReLU, base [32, 167, 173], N = 16 x 16 = 256:
           q = 167 / 173, 3 chunks, 7 padding components: 256 x 48 = 12288 B
      C  conv 1x1 + Rescale(3) + joint ReLU, first 7 primes, N = 8 x 16 = 128:
           q = 7, 6 chunks, 3 padding components: 128 x 96 = 12288 B
           (also q = 17 and B's q = 32, 4 chunks each: 128 x 64 = 8192 B against 256 x 64 = 16384 B: no collision)

    All run on one thread, hence on one garbling context and stream. A leaves its mod-2 labels in 12288-byte blocks;
    B's conv output for 167 and 173 and C's for 7 are allocated from them, and from each other's in the later
    rounds and in the reverse order. Each result must be the host garbler's, byte for byte."""
    A, B, C = gcs.order_cases()
    assert 48 * 16 * 16 == 256 * 3 * 16 == 128 * 6 * 16 == 12288
    assert native.nr_comps(2) == 128 and native.nr_comps(167) == native.nr_comps(173) == 17 and native.nr_comps(7) == 45
    seen = []
    for case in (A, B, C, A, C, B, A, B):
        if seen:  # the earlier garblings' label blocks wait in the cache
            assert native.gpu_table_cache_bytes() >= 12288
        same, lines, _ = gcs.device_vs_host(case, native)
        assert same, f"{case.name} after {seen}: the device garbler's bytes differ from the host garbler's"
        seen.append(case.name)
        xa = {}
        for p in _projects(gcs.parse_log(lines)):
            xa.update(p["xa"])
        if case is B:
            assert xa.get(167) == xa.get(173) == "rt3", xa
        else:
            assert xa.get(2) == "g8", xa
            assert case is A or xa.get(7) == "g8" and xa.get(11) == "g4", xa


def test_minionn_head_wraps(native):
    """The first column of the module docstring's table, from the launch record: garbling the `minionn_head[fused]`
    circuit of test_gpu_parity.py (conv, legacy Rescale(5), ReLU: 57600 elements per gadget) wraps the grids of k_bank
    and k_rescale_post_g and no other. (Byte identity of this circuit is that test's.)"""
    from dash_amd.garbling import GarbledCircuit
    from dash_amd.ir.circuit import Circuit
    from dash_amd.ir.quant import QuantizationMethod as Q
    from dash_amd.models import build_circuit

    full = build_circuit("MODEL_F_MINIONN_POOL_REPL", Q.ScaleQuant, 5, seed=0)
    native.hip_garbler_log(True)
    try:
        native.hip_garbler_log_take()
        GarbledCircuit(Circuit(full.layers[:3]), 7, 100.0, seed=gcs.SEED, device=0, fused_sign=True, hardened=False)
        recs = gcs.parse_log(native.hip_garbler_log_take())
    finally:
        native.hip_garbler_log(False)
    assert {r["N"] for r in recs if r["what"] == "entry"} == {57600}
    most = {}
    for r in recs:
        if r["what"] in ("launch", "draw"):
            name = r.get("name", "k_draw")
            most[name] = max(most.get(name, 0), r["blocks"])
            assert r["grid"] == min(r["blocks"], r["cap"]), r
    caps = {"k_bank": 32768, "k_emit": 65536, "k_rescale_post_g": 4096, "k_hash_iu": 16384, "k_draw": 16384,
            "k_bin_keys": 8192, "k_rescale_pre": 2048, "k_relu_finish": 4096, "k_iR": 1024}
    assert set(most) == set(caps), most
    assert {n for n in most if most[n] > caps[n]} == {"k_bank", "k_rescale_post_g"}, most
    assert most["k_bank"] == 40500 and most["k_rescale_post_g"] == 28800 and most["k_emit"] == 36000, most


def test_default_cases_cover_the_forms(native):
    """The union of the default-knob cases' records holds every compress class that a CRT or MRS modulus of any
    case maps to (from the predicate's restatement, garbler_cases.compress_class), at least two k_emit tile sizes,
    and the uniform-i key path both hardened and not: a later change to the case list cannot drop a form
    silently."""
    need = set()
    for c in CASES:
        crt, mrs = c.bases()
        need |= {gcs.compress_class(q) for q in crt + mrs}
    assert need >= {"g8", "g4", "rt3"}, need  # [2 ..], [.. 11 ..] / 32, and 97 / 107 / 167 / 173
    got, tsh, iu = set(), set(), set()
    for c in CASES:
        same, recs = _run(c, native)
        for p in _projects(recs):
            got |= set(p["xa"].values())
            tsh |= set(p["tsh"])
            if p["keys"] == "iu":
                iu.add(p["hard"])
    assert need <= got, (need, got)
    assert len(tsh) >= 2, tsh
    assert iu == {0, 1}, iu


# ------------------------------------------------------------------ process-wide forms, one child process each
SETTINGS = {
    "keys0": {"DASH_GG_KEYS": "0"},
    "keys1": {"DASH_GG_KEYS": "1"},
    "entry": {"DASH_GG_KEYS": "0", "DASH_GG_HASH": "entry"},
    "fused": {"DASH_GG_FUSED": "1"},
    "aes16": {"DASH_GG_AES_COPIES": "16"},
    "lds8": {"DASH_GG_EMIT_LDS_KB": "8"},
    "lds56": {"DASH_GG_EMIT_LDS_KB": "56"},
    "draw1": {"DASH_GG_DRAW_BLOCKS": "1"},
}
KNOBS = sorted({k for env in SETTINGS.values() for k in env})
CHILD_TIMEOUT_S = 120


@pytest.fixture(scope="module")
def children():
    """Runs the children lazily, one at a time. A child that ran to its end exits with status 0 and prints `same` or
    `differ` last, whatever it found. Every other end (a signal, an abort, its timeout, or a non-zero status, which
    is also how a HIP error raised as an exception in the child ends it) may mean a faulted card: that child is
    marked dead and no further child is started."""
    state = {"dead": None, "done": {}}

    def run(setting):
        if setting in state["done"]:
            return state["done"][setting]
        if state["dead"] is not None:
            pytest.fail(f"not run: child {state['dead']} died")
        root = str(Path(__file__).resolve().parents[1])
        env = {k: v for k, v in os.environ.items() if k not in KNOBS}
        env.update(SETTINGS[setting])
        try:
            r = subprocess.run([sys.executable, "-m", "tests.garbler_cases"], capture_output=True, text=True,
                               timeout=CHILD_TIMEOUT_S, env=env, cwd=root)
        except subprocess.TimeoutExpired as e:
            state["dead"] = setting
            pytest.fail(f"child {setting} hit its {CHILD_TIMEOUT_S} s timeout: {e.stdout!r} {e.stderr!r}")
        last = ([ln for ln in r.stdout.splitlines() if ln.strip()] or [""])[-1]
        if r.returncode != 0 or last not in ("same", "differ"):
            state["dead"] = setting
            pytest.fail(f"child {setting} died with status {r.returncode}: {r.stdout[-2000:]} {r.stderr[-2000:]}")
        state["done"][setting] = r
        return r

    return run


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_process_wide_form(setting, children, native):
    """Each A/B form of the garbler that is read once from the environment garbles the short list (sign, mixed-radix
    rescale, joint, ReDash rescale, 3x3 max pool at N = 65, both encodings where both exist) byte-identically to
    the host garbler, and the launch record shows that the setting took effect.

    DASH_GG_FUSED = 1: a hardened projection set without an R_INPUT payload offset (rin = 0) is fused, every other
    one keeps the uniform-i path. Fused: the sign's, the mixed-radix rescale's and the ReDash rescale's sets
    (sign-hard, rescale_mrs-hard, redash-hard, the rescale half of joint-hard, the sign half of every maxpool3-hard
    level). Not fused: the mixed-modulus half gates, which pay out multiples of the input label (the ReLU half of
    joint-hard and of every maxpool3-hard level), and every set of the reference-encoding cases."""
    r = children(setting)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = [ln for ln in r.stdout.splitlines() if ln.strip()]
    runs = {j["case"]: j for j in map(json.loads, out[:-1])}
    assert set(runs) == {c.name for c in gcs.child_cases()}
    assert all(j["same"] for j in runs.values()) and out[-1] == "same", {n: j["same"] for n, j in runs.items()}
    recs = {n: gcs.parse_log(j["log"]) for n, j in runs.items()}
    pro = [p for rs in recs.values() for p in _projects(rs)]
    draws = [x for rs in recs.values() for x in rs if x["what"] == "draw"]
    launches = {x["name"] for rs in recs.values() for x in rs if x["what"] == "launch"}
    base = [p for c in gcs.child_cases() for p in _projects(_run(c, native)[1])]  # this process: default knobs
    assert pro and draws and len(pro) == len(base)
    if setting == "keys0":
        assert {p["keys"] for p in pro} == {"jobs"} and "k_hash_jobs" in launches and "k_hash_iu" not in launches
        assert all(p["bank_paired"] == 0 and p["xa"] == {} for p in pro) and sum(p["bank_single"] for p in pro) > 0
    elif setting == "keys1":
        assert {p["keys"] for p in pro} == {"jobs"} and "k_hash_jobs" in launches
        assert all(p["bank_paired"] == 0 for p in pro) and any(p["xa"] for p in pro)  # multiple rows: bank only
    elif setting == "entry":
        assert {p["keys"] for p in pro} == {"entry"} and {p["hash"] for p in pro} == {"k_hash<32>"}
        assert "k_hash" in launches and "k_hash_jobs" not in launches and "k_hash_iu" not in launches
    elif setting == "fused":
        for p in pro:
            assert p["keys"] == ("fused" if p["hard"] and not p["rin"] else "iu"), p
        want = {"sign-hard-n65": ["fused"], "rescale_mrs-hard-n65": ["fused"], "joint-hard-n65": ["fused", "iu"],
                "redash-hard-n65": ["fused"] * 7, "maxpool3-hard-n65": ["fused", "iu"] * 4}
        for name, keys in want.items():
            assert [p["keys"] for p in _projects(recs[name])] == keys, name
        for name in ("sign-ref-n65", "redash-ref-n65", "maxpool3-ref-n65"):
            assert {p["keys"] for p in _projects(recs[name])} == {"iu"}, name
    elif setting == "aes16":
        assert {x["kernel"] for x in draws} == {"k_draw<16>"}
        assert {p["hash"] for p in pro} == {"k_hash_iu<16,hard>", "k_hash_iu<16>"}
    elif setting == "lds8":
        assert {p["budget"] for p in pro} == {8 << 10}
        assert min(t for p in pro for t in p["tsh"]) < min(t for p in base for t in p["tsh"])
        assert sum(p["scopes"] for p in pro) >= sum(p["scopes"] for p in base)
    elif setting == "lds56":
        # the default budget reaches tsh = 5 too: the budget itself, and fewer k_emit blocks than the default run
        assert {p["budget"] for p in pro} == {56 << 10} and {p["budget"] for p in base} == {24 << 10}
        assert any(t == 5 for p in pro for t in p["tsh"])
        assert sum(p["emit_blocks"] for p in pro) < sum(p["emit_blocks"] for p in base)
    elif setting == "draw1":
        assert all(x["grid"] == 1 and x["cap"] == 1 for x in draws) and any(x["blocks"] > 1 for x in draws)
    if setting not in ("keys0", "keys1", "entry", "fused"):
        assert {p["keys"] for p in pro} == {"iu"}
