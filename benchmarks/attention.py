"""The multi-head MatMul of a ReLU-attention block against its two single-head yardsticks, per-op hipEvent timers.

    python benchmarks/attention.py --batch 24 --steps 7 --warmup 3 --out profiles/attention_b24.json

One-layer circuits at k = 7, one stream; every variant gets its own HipEvaluator with set_profile(True), the variants
alternate over the timed steps, all in one process. Shapes (G, M, T, N), G heads of an M x T by T x N contraction:
  zs  (4, 16, 8, 16)   the scores q^T k of RELU_ATTN_CIFAR (trans_a)      zm  (4, 8, 16, 16)   its mix v S^T (trans_b)
  ls  (4, 64, 8, 64)   the scores at L = 64 tokens                        lm  (4, 8, 64, 64)   their mix
Variants of a shape:
  heads.lane / heads.blocked   MatMul(..., heads=G) under either kernel form (DASH_MATMUL_FORM, which the evaluator
                               reads when it plans): the same garbled circuits
  heads  the same circuits again under the form the planner's rule picks
  sep    G single-head MatMul layers (M, T, N) on separate operands (2 G dense selections of the input), summed: what
         the heads cost without the head index, G key pre-passes and G launches; the planner's rule picks the form
  one    one single-head MatMul (G M, T, N): as many products in one contraction (it computes another function)
x is the circuit input, y a 0 / 1 dense selection of it. Reported per variant: the contraction and key pre-pass
times summed over the variant's MatMul layers, medians and spread over the timed steps, and for the heads variants
the ratio of contraction + pre-pass to each yardstick's of the same run.

The profiled steps run eagerly (set_profile turns graph replay off), so the times are those of the kernels alone.

Needs a GPU: there is no CPU fallback.
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

# (G, M, T, N), trans_a, trans_b
SHAPES = {"zs": ((4, 16, 8, 16), True, False), "zm": ((4, 8, 16, 16), False, True),
          "ls": ((4, 64, 8, 64), True, False), "lm": ((4, 8, 64, 64), False, True)}
VARIANTS = ("heads.lane", "heads.blocked", "heads", "sep", "one")


def select(rows, nin):
    """A 0 / 1 dense layer that reads the circuit input: output e is input element rows[e]."""
    import dash_amd as d

    w = np.zeros((len(rows), nin), dtype=np.int64)
    w[np.arange(len(rows)), rows] = 1
    sel = d.Dense.from_quantized(w, np.zeros(len(rows), dtype=np.int64))
    sel.in_src = -1
    return sel


def dims(G, M, T, N, ta, tb):
    return ((G * T, M) if ta else (G * M, T)), ((G * N, T) if tb else (G * T, N))


def circuit(shape, variant):
    """(circuit, indices of its MatMul layers)"""
    import dash_amd as d

    (G, M, T, N), ta, tb = SHAPES[shape]
    nx, ny = G * M * T, G * T * N
    idx = (nx - 1 - np.arange(ny)) % nx  # y's elements in x
    if variant == "sep":
        layers = []
        for g in range(G):
            layers += [select(idx[g * T * N:(g + 1) * T * N], nx), select(np.arange(g * M * T, (g + 1) * M * T), nx)]
        dx, dy = dims(1, M, T, N, ta, tb)
        for g in range(G):
            mm = d.MatMul(dx, 2 * g, dy, trans_a=ta, trans_b=tb)
            mm.in_src = 2 * g + 1
            layers.append(mm)
        return d.Circuit(layers), list(range(2 * G, 3 * G))
    if variant == "one":
        dx, dy = dims(1, G * M, T, N, ta, tb)
        mm = d.MatMul(dx, 0, dy, trans_a=ta, trans_b=tb)
        mm.in_src = -1
        return d.Circuit([select(idx[:T * N], nx), mm]), [1]
    dx, dy = dims(G, M, T, N, ta, tb)
    mm = d.MatMul(dx, 0, dy, trans_a=ta, trans_b=tb, heads=G)
    mm.in_src = -1
    return d.Circuit([select(idx, nx), mm]), [1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--crt", type=int, default=7)
    ap.add_argument("--shapes", default="zs,zm,ls,lm")
    ap.add_argument("--label", default="", help="free text kept in the record")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/attention.py: no GPU visible (the benchmark has no CPU fallback)")

    from dash_amd.garbling import GarbledCircuit
    from dash_amd.ir.bases import crt_modulus, first_primes
    from dash_amd.native import native
    from dash_amd.runtime import HipEvaluator

    n = native()
    B = args.batch
    half = crt_modulus(first_primes(args.crt)) // 2
    rng = np.random.default_rng(1)
    st = torch.cuda.current_stream()

    evs, info = {}, {}
    for shape in args.shapes.split(","):
        (G, M, T, N), ta, tb = SHAPES[shape]
        lim = math.isqrt((half - 1) // T)
        xs = [rng.integers(-lim, lim + 1, G * M * T) for _ in range(B)]
        gcs = None
        for variant in VARIANTS:
            kind, _, kform = variant.partition(".")
            if kind != "heads" or gcs is None:  # both kernel forms of the heads layer evaluate the same garbled circuits
                c, mms = circuit(shape, kind)
                gcs = [GarbledCircuit(c, args.crt, 100.0, seed=bytes([b + 1] * 16), device=0) for b in range(B)]
            if kform:
                os.environ["DASH_MATMUL_FORM"] = kform
            else:
                os.environ.pop("DASH_MATMUL_FORM", None)
            ev = HipEvaluator(template=gcs[0].model, batch=B, device=0)
            os.environ.pop("DASH_MATMUL_FORM", None)
            for b, gc in enumerate(gcs):
                ev.load(b, gc.model)
                ev.encode_compressed_into(b, gc, xs[b])
            n.hip_launch_log_take()
            n.hip_launch_log(True)
            for _ in range(args.warmup):
                ev.upload_inputs_compressed(st)
                ev.run(st)
            n.hip_launch_log(False)
            log = [l for l in n.hip_launch_log_take() if l.startswith("matmul.")]
            ev.fetch_outputs(st)
            for b, gc in enumerate(gcs):
                assert np.array_equal(ev.decode(b, gc), gc.plain_q_eval(xs[b])), (shape, variant)
            ev.set_profile(True)
            name = f"{shape}.{variant}"
            evs[name] = (ev, [f"matmul#{i}" for i in mms], [f"matmul#{i}.K" for i in mms])
            info[name] = {"shape": [G, M, T, N], "trans": [int(ta), int(tb)], "layers": len(mms),
                          "launch": sorted(set(log)), "products": G * M * T * N}
            if kform:
                assert {l.split()[0] for l in log} == {"matmul." + kform}, info[name]
    times = {name: [] for name in evs}
    pres = {name: [] for name in evs}
    for _ in range(args.steps):
        for name, (ev, ops, keys) in evs.items():  # the variants alternate
            ev.upload_inputs_compressed(st)
            ev.run(st)
            torch.cuda.synchronize()
            got = dict(ev.op_times())
            assert all(o in got for o in ops + keys), ev.op_times()
            times[name].append(sum(got[o] for o in ops))  # the layers alone: no save, restore or dense op
            pres[name].append(sum(got[o] for o in keys))
    rec = {"batch": B, "crt": args.crt, "steps": args.steps, "warmup": args.warmup, "label": args.label, "forms": {}}
    for name, ts in times.items():
        tot = [a + b for a, b in zip(ts, pres[name])]
        rec["forms"][name] = dict(info[name], ms=[round(t, 4) for t in ts], median_ms=round(statistics.median(ts), 4),
                                  spread_ms=round(max(ts) - min(ts), 4), key_ms=[round(t, 4) for t in pres[name]],
                                  key_median_ms=round(statistics.median(pres[name]), 4),
                                  total_median_ms=round(statistics.median(tot), 4),
                                  total_spread_ms=round(max(tot) - min(tot), 4))
    for name, r in rec["forms"].items():
        shape, _, variant = name.partition(".")
        if variant.startswith("heads"):
            for yard in ("sep", "one"):
                if f"{shape}.{yard}" in rec["forms"]:
                    r["ratio_to_" + yard] = round(r["total_median_ms"] / rec["forms"][f"{shape}.{yard}"]["total_median_ms"], 3)
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
