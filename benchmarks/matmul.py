"""The MatMul layer's kernel against an elementwise Mul of as many products, per-op hipEvent timers.

    python benchmarks/matmul.py --batch 24 --steps 7 --warmup 3 --out profiles/matmul_b24.json

One-layer-pair circuits at k = 7, one stream; every form gets its own HipEvaluator with set_profile(True), the forms
alternate over the timed steps, all in one process. Forms:
  f      MatMul (M, T, N) = (64, 16, 64): the non-local block's affinities theta^T phi at C / r = 16, H W = 64
  y      MatMul (16, 64, 64): its mix g f^T
         each as f.lane / f.blocked, y.lane / y.blocked: the same garbled circuits under both kernel forms
         (DASH_MATMUL_FORM, which the evaluator reads when it plans)
  mul    Mul over M T N = 65536 elements (both operands the circuit input, the generalized half gates): the same
         half gates without the on-chip sum, and with every product's label written to HBM
x is the circuit input, y a 0 / 1 dense selection of it. Reported per form: the times of the contraction op and of
its key pre-pass (".K": both operands' labels compressed once), medians and spread, the ratio of contraction + pre-pass
to the Mul's median of the same run, the launch form and the table bytes per output against 16 * matmul_entries.

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

SHAPES = {"f": (64, 16, 64), "y": (16, 64, 64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--crt", type=int, default=7)
    ap.add_argument("--forms", default="f.lane,f.blocked,y.lane,y.blocked,mul")
    ap.add_argument("--label", default="", help="free text kept in the record")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/matmul.py: no GPU visible (the benchmark has no CPU fallback)")

    import dash_amd as d
    from dash_amd.garbling import GarbledCircuit
    from dash_amd.ir.bases import crt_modulus, first_primes
    from dash_amd.native import native
    from dash_amd.runtime import HipEvaluator

    n = native()
    B = args.batch
    crt = first_primes(args.crt)
    half = crt_modulus(crt) // 2
    rng = np.random.default_rng(1)
    st = torch.cuda.current_stream()

    def circuit(form):
        """(circuit, contraction op, pre-pass op or None, input size, operand bound, outputs, T)"""
        if form == "mul":
            N = int(np.prod(SHAPES["f"]))
            return d.Circuit([d.Flatten((N,)), d.Mul((N,), -1)]), "mul#1", None, N, math.isqrt(half - 1), N, 0
        M, T, N = SHAPES[form.split(".")[0]]
        idx = (M * T - 1 - np.arange(T * N)) % (M * T)
        w = np.zeros((T * N, M * T), dtype=np.int64)
        w[np.arange(T * N), idx] = 1
        mm = d.MatMul((M, T), 0, (T, N))
        mm.in_src = -1
        c = d.Circuit([d.Dense.from_quantized(w, np.zeros(T * N, dtype=np.int64)), mm])
        return c, "matmul#1", "matmul#1.K", M * T, math.isqrt((half - 1) // T), M * N, T

    evs, info, garbled = {}, {}, {}
    for form in args.forms.split(","):
        shape, _, kform = form.partition(".")
        if shape not in garbled:  # both kernel forms of a shape evaluate the same garbled circuits
            c, op, pre, nin, lim, nout, T = circuit(form)
            xs = [rng.integers(-lim, lim + 1, nin) for _ in range(B)]
            gcs = [GarbledCircuit(c, args.crt, 100.0, seed=bytes([b + 1] * 16), device=0) for b in range(B)]
            garbled = {shape: (c, op, pre, nin, lim, nout, T, xs, gcs)}  # one shape's GCs at a time
        c, op, pre, nin, lim, nout, T, xs, gcs = garbled[shape]
        if kform:
            os.environ["DASH_MATMUL_FORM"] = kform
        else:
            os.environ.pop("DASH_MATMUL_FORM", None)
        ev = HipEvaluator(template=gcs[0].model, batch=B, device=0)
        for b, gc in enumerate(gcs):
            ev.load(b, gc.model)
            ev.encode_compressed_into(b, gc, xs[b])
        n.hip_launch_log_take()
        n.hip_launch_log(True)
        for _ in range(args.warmup):
            ev.upload_inputs_compressed(st)
            ev.run(st)
        n.hip_launch_log(False)
        log = [l.split()[0] for l in n.hip_launch_log_take() if l.startswith(("mul.", "matmul."))]
        ev.fetch_outputs(st)
        for b, gc in enumerate(gcs):
            assert np.array_equal(ev.decode(b, gc), gc.plain_q_eval(xs[b])), form
        ev.set_profile(True)
        evs[form] = (ev, op, pre)
        tab = sum(int(np.asarray(a).nbytes) for a in gcs[0].model.layer_arrays(len(c.layers) - 1).values())
        info[form] = {"op": op, "launch": sorted(set(log)), "table_bytes_per_output": tab / nout}
        if T:
            info[form]["shape"] = list(SHAPES[shape])
            assert info[form]["launch"] == ["matmul." + kform], info[form]
            info[form]["entries_x16"] = 16 * n.matmul_entries(crt, T)
            assert info[form]["table_bytes_per_output"] == info[form]["entries_x16"], info[form]
    times = {form: [] for form in evs}
    pres = {form: [] for form in evs}
    for _ in range(args.steps):
        for form, (ev, op, pre) in evs.items():  # the forms alternate
            ev.upload_inputs_compressed(st)
            ev.run(st)
            torch.cuda.synchronize()
            t = [ms for name, ms in ev.op_times() if name == op]  # the layer alone: no save, restore or dense op
            assert len(t) == 1, ev.op_times()
            times[form].append(t[0])
            if pre:
                k = [ms for name, ms in ev.op_times() if name == pre]
                assert len(k) == 1, ev.op_times()
                pres[form].append(k[0])
    rec = {"batch": B, "crt": args.crt, "steps": args.steps, "warmup": args.warmup, "label": args.label, "forms": {}}
    for form, ts in times.items():
        r = dict(info[form], ms=[round(t, 4) for t in ts], median_ms=round(statistics.median(ts), 4),
                 spread_ms=round(max(ts) - min(ts), 4))
        if pres[form]:
            r["key_ms"] = [round(t, 4) for t in pres[form]]
            r["key_median_ms"] = round(statistics.median(pres[form]), 4)
            tot = [a + b for a, b in zip(ts, pres[form])]
            r["total_median_ms"] = round(statistics.median(tot), 4)
            r["total_spread_ms"] = round(max(tot) - min(tot), 4)
        rec["forms"][form] = r
    if "mul" in rec["forms"]:
        y = rec["forms"]["mul"]["median_ms"]
        for form, r in rec["forms"].items():
            r["ratio_to_mul"] = round(r.get("total_median_ms", r["median_ms"]) / y, 3)
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
