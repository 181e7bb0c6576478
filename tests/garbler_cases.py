"""The GPU garbler's edge cases, as data (tests/test_garbler_cases.py on the host, tests/test_gpu_garbler_forms.py
and its child processes on the GPU).

A case garbles one gadget kind (one layer, or the shortest pair of layers that forms the gadget) at one size under
one encoding. `Case.build()` returns (circuit, crt, mrs, kwargs) for GarbledCircuit; `Case.entries` names the
gadget-level entry points of the device garbler the case is meant to reach (the `entry` lines of the garbler's
launch record, csrc/hip/gpu_garbler.h), `Case.inputs()` one input vector inside the gadgets' exact range.

Sizes. N in SIZES = (1, 63, 64, 65, 257) elements per gadget: one element, one below / at / one past a 64-lane tile
(65 is a multiple of no k_emit tile te > 1), and one past a 256-thread block.
  * elementwise kinds: the layer has N elements;
  * MaxPool2d 2x2 (stride 2): C x OH x OW outputs = 1, 63, 64, 65, 257 exactly (geometries in POOL2); the tree's
    two levels garble 2 N and N elements;
  * MaxPool2d 3x3 (stride 3): outputs = 1, 63, 64, 65, 257 exactly (POOL3); the four levels (4, 2, 1, 1 pairs, the
    first three with an odd carry) garble 4 N, 2 N, N and N elements;
  * Max((n,)): one window of n = 2, 126, 128, 130, 514 values, so the first level garbles N = n / 2 = 1, 63, 64, 65,
    257 pair differences and the later levels ceil-halve that;
  * SumPool2d 2x2 + Relu: the 2x2 geometries, the ReLU garbles N window sums;
  * Dense: (in, out) = (1, 1), (65, 63), (257, 64), (63, 65), (64, 257): the garbler's k_gdense tiles 64 outputs, so
    every size but 64 leaves a partial tile; the channel_tf case is (96, 33) with 3 channels.

Encodings. "hard": the hardened encoding (fused sign); "ref": the reference encoding with the fused sign
(hardened=False); "refcasts": the reference sign construction (fused_sign=False, reference encoding), for every kind
that holds an approximate sign. Every kind runs at every size in every encoding listed for it in _kinds. The
mixed-radix constructions exist hardened only, the legacy rescale in the reference encoding only; the ReDash rescale,
the base extension and the dense layer hold no sign gadget, so the sign construction does not change them.

Bases (BASE_CASES, N = 65). k = 2, 3 and 9 first-prime bases on the three core gadgets, and the three ReDash bases
of BENCH_CONFIGS on the ReDash rescale and the base extension. Below k = 4 no mrs argument is given (the convention
of tests/test_gpu_parity.py::test_rescale_relu_joint), and without an MRS base the approximate sign cannot be
garbled at all: Garbler refuses with "sign gadget needs a non-empty MRS base" (a DASH_CHECK of the sign plan; noted,
not widened). The sign gadget of the k = 2 and k = 3 cases is therefore the exact mixed-radix sign (relu="mrs").
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable

import numpy as np

import dash_amd as d
from dash_amd.ir.bases import crt_modulus, first_primes, get_mrs_base
from dash_amd.models import BENCH_CONFIGS

SIZES = (1, 63, 64, 65, 257)
# N -> (C, H, W) of a 2x2 / 3x3 max or sum pool with stride = kernel: C * (H / k) * (W / k) = N
POOL2 = {1: (1, 2, 2), 63: (7, 6, 6), 64: (1, 16, 16), 65: (5, 26, 2), 257: (1, 514, 2)}
POOL3 = {1: (1, 3, 3), 63: (7, 9, 9), 64: (1, 24, 24), 65: (5, 39, 3), 257: (1, 771, 3)}
MAXN = {1: 2, 63: 126, 64: 128, 65: 130, 257: 514}
DENSE = {1: (1, 1), 63: (65, 63), 64: (257, 64), 65: (63, 65), 257: (64, 257)}
REDASH_BASES = [(tuple(c["crt"]), tuple(c["mrs"])) for n, c in sorted(BENCH_CONFIGS.items()) if "/REDASH" in n]

ENC = {"hard": {}, "ref": {"hardened": False}, "refcasts": {"hardened": False, "fused_sign": False}}


@dataclass(frozen=True)
class Case:
    name: str
    kind: str
    N: int
    enc: str
    make: Callable[[], tuple] = field(repr=False, compare=False)  # -> (circuit, crt, mrs, kwargs)
    entries: tuple = ()      # entry points of the device garbler this case reaches (set of names)
    gadget_n: tuple = ()     # the N of those entry lines, in order (empty: not asserted)
    hardened: bool = True
    lo: int = -20            # input range [lo, hi]
    hi: int = 20
    child: bool = False      # on the child processes' short list

    def build(self):
        c, crt, mrs, kw = self.make()
        return c, crt, mrs, dict(kw)

    def bases(self):
        """(crt moduli, mrs moduli) of the case."""
        _, crt, mrs, _ = self.build()
        crt = first_primes(crt) if isinstance(crt, int) else [int(p) for p in crt]
        if mrs is None:
            mrs = []
        elif isinstance(mrs, float):
            mrs = get_mrs_base(len(crt), mrs)
        return crt, [int(m) for m in mrs]

    def inputs(self, seed: int = 3) -> np.ndarray:
        c = self.build()[0]
        M = crt_modulus(self.bases()[0])
        lo, hi = max(self.lo, -(M // 2) + 1), min(self.hi, M // 2 - 2)
        return np.random.default_rng(seed).integers(lo, hi + 1, c.input_size).astype(np.int64)


def _dense(fin, fout, channel_tf=0, seed=11):
    rng = np.random.default_rng(seed + fin + fout)
    return d.Dense(rng.integers(-4, 5, (fout, fin)), rng.integers(-6, 6, fout), q_const=1.0, channel_tf=channel_tf)


def _kinds(N: int):
    """kind -> (circuit builder, crt, mrs, kwargs, encodings, entries, gadget N per entry line)."""
    c2, h2, w2 = POOL2[N]
    c3, h3, w3 = POOL3[N]
    n = MAXN[N]
    halves = []
    v = n
    while v > 1:
        halves.append(v // 2)
        v = v // 2 + v % 2
    fin, fout = DENSE[N]
    return {
        "sign": (lambda: d.Circuit([d.Sign((N,))]), 7, 100.0, {}, ("hard", "ref", "refcasts"), ("sign",), (N,)),
        "relu": (lambda: d.Circuit([d.Relu((N,))]), 8, 100.0, {"relu": "approx"}, ("hard", "ref", "refcasts"),
                 ("sign_relu",), (N,)),
        "rescale_legacy": (lambda: d.Circuit([d.Rescale(2, (N,))]), 7, 100.0, {"rescale": "legacy"},
                           ("ref", "refcasts"), ("rescale_legacy_iter",), (N, N)),
        "rescale_mrs": (lambda: d.Circuit([d.Rescale(3, (N,))]), 7, 100.0, {"rescale": "mrs", "relu": "approx"},
                        ("hard",), ("rescale_mrs",), (N,)),
        "relu_mrs": (lambda: d.Circuit([d.Relu((N,))]), 7, 100.0, {"relu": "mrs"}, ("hard",), ("relu_mrs",), (N,)),
        "joint": (lambda: d.Circuit([d.Rescale(3, (N,)), d.Relu((N,))]), 7, 100.0,
                  {"rescale": "mrs", "relu": "joint"}, ("hard",), ("rescale_mrs", "relu_mult"), (N, N)),
        "redash": (lambda: d.Circuit([d.Rescale([32], (N,))]), [32, 3, 5, 7, 11, 13, 17], [10, 9, 9, 8, 7, 7, 6], {},
                   ("hard", "ref"), ("rescale_redash",), (N,)),
        "base_ext": (lambda: d.Circuit([d.BaseExtension((N,), [32])]), [32, 97, 107], [22, 19, 15, 13], {},
                     ("hard", "ref"), ("base_ext",), (N,)),
        "maxpool2": (lambda: d.Circuit([d.MaxPool2d(w2, h2, c2, 2, 2)]), 8, 100.0, {}, ("hard", "ref", "refcasts"),
                     ("maxpool_level",), (2 * N, N)),
        "maxpool3": (lambda: d.Circuit([d.MaxPool2d(w3, h3, c3, 3, 3)]), 8, 100.0, {}, ("hard", "ref", "refcasts"),
                     ("maxpool_level",), (4 * N, 2 * N, N, N)),
        "max": (lambda: d.Circuit([d.Max((n,))]), 8, 100.0, {}, ("hard", "ref", "refcasts"),
                ("maxpool_level",), tuple(halves)),
        "sumpool_relu": (lambda: d.Circuit([d.SumPool2d(w2, h2, c2, 2, 2), d.Relu((c2, h2 // 2, w2 // 2))]), 8, 100.0,
                         {"relu": "approx"}, ("hard", "ref", "refcasts"), ("sumpool", "sign_relu"), (N, N)),
        "dense": (lambda: d.Circuit([_dense(fin, fout)]), 8, 100.0, {}, ("hard", "ref"), ("dense",), (fin,)),
    }


CHILD_KINDS = ("sign", "rescale_mrs", "joint", "redash", "maxpool3")


def _gadget_cases():
    out = []
    for N in SIZES:
        for kind, (mk, crt, mrs, kw, encs, entries, gn) in _kinds(N).items():
            for enc in encs:
                kws = dict(kw, **ENC[enc])
                lo, hi = (0, 97 * 107 - 1) if kind == "base_ext" else (-20, 20)
                out.append(Case(f"{kind}-{enc}-n{N}", kind, N, enc, (lambda mk=mk, crt=crt, mrs=mrs, kws=kws:
                                                                    (mk(), crt, mrs, kws)),
                                entries, gn, enc == "hard", lo, hi,
                                N == 65 and kind in CHILD_KINDS and enc in ("hard", "ref")))
    out.append(Case("dense_tf-hard-n33", "dense_tf", 33, "hard",
                    lambda: (d.Circuit([_dense(96, 33, channel_tf=3)]), 8, 100.0, {}), ("dense",), (96,)))
    return out


def _base_cases():
    """N = 65: the small and large first-prime bases on the three core gadgets, the ReDash bases on the ReDash
    rescale and the base extension."""
    N, out = 65, []
    for k in (2, 3, 9):
        mrs = 100.0 if k >= 4 else None
        if k >= 4:
            out.append(Case(f"sign-hard-k{k}", "sign", N, "hard", lambda k=k, mrs=mrs: (
                d.Circuit([d.Sign((N,))]), k, mrs, {}), ("sign",), (N,)))
        else:  # no MRS base below k = 4: the exact sign (module docstring)
            out.append(Case(f"sign_mrs-hard-k{k}", "relu_mrs", N, "hard", lambda k=k, mrs=mrs: (
                d.Circuit([d.Relu((N,))]), k, mrs, {"relu": "mrs"}), ("relu_mrs",), (N,)))
        out.append(Case(f"rescale_mrs-hard-k{k}", "rescale_mrs", N, "hard", lambda k=k, mrs=mrs: (
            d.Circuit([d.Rescale(1, (N,))]), k, mrs, {"rescale": "mrs", "relu": "approx"}), ("rescale_mrs",), (N,)))
        out.append(Case(f"joint-hard-k{k}", "joint", N, "hard", lambda k=k, mrs=mrs: (
            d.Circuit([d.Rescale(1, (N,)), d.Relu((N,))]), k, mrs, {"rescale": "mrs", "relu": "joint"}),
            ("rescale_mrs", "relu_mult"), (N, N)))
    for crt, mrs in REDASH_BASES:
        tag = "_".join(map(str, crt[:3]))
        others = crt_modulus(list(crt[1:]))
        for enc in ("hard", "ref"):
            out.append(Case(f"redash-{enc}-b{tag}", "redash", N, enc, lambda crt=crt, mrs=mrs, enc=enc: (
                d.Circuit([d.Rescale([32], (N,))]), list(crt), list(mrs), dict(ENC[enc])), ("rescale_redash",), (N,),
                enc == "hard"))
            out.append(Case(f"base_ext-{enc}-b{tag}", "base_ext", N, enc, lambda crt=crt, mrs=mrs, enc=enc: (
                d.Circuit([d.BaseExtension((N,), [32])]), list(crt), list(mrs), dict(ENC[enc])), ("base_ext",), (N,),
                enc == "hard", 0, min(others, 1 << 20) - 1))
    return out


def _newer_cases():
    """Clip, ArgMax, Mul, MatMul, PiecewiseLinear and LeakyRelu have device cases at convenient sizes in their own
    files; here only N = 1 and N = 65. Their gadget-level entry points are their own (not in the ten recorded
    ones), except where they garble through a recorded one."""
    from tests import leaky_cases, matmul_cases, mul_cases, pwl_cases

    out = []
    for N in (1, 65):
        mm = (1, 1, 1) if N == 1 else (5, 2, 13)
        am = (3,) if N == 1 else (3, 5, 13)
        for kind, mk, kw, entries in (
                ("clip", lambda N=N: d.Circuit([d.Clip.from_quantized((N,), 0, 41)]), {"relu": "mrs"}, ()),
                ("argmax", lambda am=am: d.Circuit([d.ArgMax(am)]), {}, ()),
                ("mul_sq", lambda N=N: mul_cases.mul_circuit((N,), "sq"), {}, ()),
                ("mul_elem", lambda N=N: mul_cases.mul_circuit((N,), "elem"), {}, ("dense",)),
                ("matmul", lambda mm=mm: matmul_cases.matmul_circuit(*mm), {}, ("dense",)),
                ("pwl", lambda N=N: pwl_cases.pwl_circuit((N,), "m2"), {"relu": "mrs"}, ()),
                ("leaky", lambda N=N: leaky_cases.leaky_circuit((N,), 4), {"relu": "mrs"}, ("relu_mrs",))):
            out.append(Case(f"{kind}-hard-n{N}", kind, N, "hard", lambda mk=mk, kw=kw: (mk(), 7, 100.0, dict(kw)),
                            entries, ()))
    return out


def order_cases():
    """The three circuits of the order-dependence test (tests/test_gpu_garbler_forms.py::test_order_dependence has
    the sizes' reasoning). B and C start with a 1x1 convolution: the device conv writes only the n real components
    of its chunked output labels, so the padding components of that block keep what the block held before."""
    def conv(W, H):
        return d.Conv2d.from_quantized(np.array([3]).reshape(1, 1, 1, 1), np.array([1]), W, H, 1, 1, 1, 1)

    return [
        Case("order-A", "order", 48, "hard", lambda: (d.Circuit([d.Rescale(1, (48,)), d.Relu((48,))]), 2, None,
                                                      {"rescale": "mrs", "relu": "joint"}),
             ("rescale_mrs", "relu_mult"), (48, 48)),
        Case("order-B", "order", 256, "hard", lambda: (d.Circuit([conv(16, 16), d.Rescale([32], (1, 16, 16)),
                                                                  d.Relu((1, 16, 16))]),
                                                       [32, 167, 173], [26, 25, 21, 13], {}),
             ("rescale_redash", "sign_relu"), (256, 256)),
        Case("order-C", "order", 128, "hard", lambda: (d.Circuit([conv(16, 8), d.Rescale(3, (1, 8, 16)),
                                                                  d.Relu((1, 8, 16))]), 7, 100.0,
                                                       {"rescale": "mrs", "relu": "joint"}),
             ("rescale_mrs", "relu_mult"), (128, 128)),
    ]


def all_cases():
    return _gadget_cases() + _base_cases() + _newer_cases() + order_cases()


def child_cases():
    """The fixed short list a child process of the process-wide forms garbles: sign, mixed-radix rescale, joint,
    ReDash rescale and 3x3 max pool at N = 65, in both encodings where both exist."""
    return [c for c in all_cases() if c.child]


# ---------------------------------------------------------------- the garbler's launch record, parsed
def parse_log(lines):
    """The record's lines as dicts: {"what": entry|draw|launch|project, "name": ..., key: value ...}; integers
    where the value is one, `tsh` a list of ints, `xa` a {modulus: class} dict."""
    out = []
    for ln in lines:
        tok = ln.split()
        rec = {"what": tok[0]}
        rest = tok[1:]
        if tok[0] in ("entry", "launch"):
            rec["name"] = tok[1]
            rest = tok[2:]
        for t in rest:
            key, _, val = t.partition("=")
            if key == "tsh":
                rec[key] = [int(v) for v in val.split(",")]
            elif key == "xa":
                rec[key] = {} if val == "-" else {int(a.split(":")[0]): a.split(":")[1] for a in val.split(",")}
            else:
                rec[key] = int(val) if val.lstrip("-").isdigit() else val
        out.append(rec)
    return out


def compress_class(q: int) -> str:
    """The compress_xa form of modulus q, restated from garble_gpu.hip's xa_class / xa_group (held to the native
    predicate by tests/test_garbler_cases.py): chunk-aligned groups of 8 digits up to q = 8 and of 4 up to q = 64,
    else runtime groups of the most digits g with q^g <= 2^24, or the shift form for a power of two."""
    if q <= 8:
        return "g8"
    if q <= 64:
        return "g4"
    if q & (q - 1) == 0:
        return "pw2"
    g = 1
    while q ** (g + 1) <= 1 << 24:
        g += 1
    return f"rt{g}"


def digest(gc) -> tuple:
    """Digests of a garbled circuit's offline message and decoder (pytest's diff of two multi-MB byte strings on a
    failure takes minutes)."""
    import hashlib

    m, dec = gc.model.serialize(), gc.decoder.serialize()
    return (len(m), hashlib.sha256(m).hexdigest(), len(dec), hashlib.sha256(dec).hexdigest())


SEED = bytes(range(16))


def device_vs_host(case, native, keep: bool = False):
    """Garble `case` on the device (with the garbler's launch record on) and on the host with one seed:
    (digests equal, the device run's record lines, the device GarbledCircuit if keep)."""
    from dash_amd.garbling import GarbledCircuit

    c, crt, mrs, kw = case.build()
    native.hip_garbler_log(True)
    try:
        native.hip_garbler_log_take()
        dev = GarbledCircuit(c, crt, mrs, seed=SEED, device=0, **kw)
        lines = list(native.hip_garbler_log_take())
    finally:
        native.hip_garbler_log(False)
    host = GarbledCircuit(c, crt, mrs, seed=SEED, **kw)
    return digest(dev) == digest(host), lines, (dev if keep else None)


def _child_main() -> int:
    """A child process of tests/test_gpu_garbler_forms.py: the DASH_GG_* environment of this process selects the
    garbler's process-wide forms. One JSON line per case of the short list, then `same` or `differ`."""
    import json

    from dash_amd.native import native

    n = native()
    ok = True
    for case in child_cases():
        same, lines, _ = device_vs_host(case, n)
        ok &= same
        print(json.dumps({"case": case.name, "same": same, "log": lines}), flush=True)
    print("same" if ok else "differ", flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(_child_main())
