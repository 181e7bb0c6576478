"""The Mul layer's kernels against the ReLU multiply, per-op hipEvent timers.

    python benchmarks/mul.py --batch 24 --steps 7 --warmup 3 --out profiles/mul_b24.json

One-layer circuits over (64, 16, 16), k = 7, one stream; every form gets its own HipEvaluator with set_profile(True),
the forms alternate over the timed steps, all in one process. Forms:
  elem       Mul(dims, src = -1) behind a Flatten: both operands are the circuit input, garbled as the generalized
             half gates (not the square projection), so this is the elementwise product's cost
  bcast      the same dims with a (64,) operand (a 0 / 1 dense selection of the input)
  square     Mul.square(dims)
  relu_mult  Relu(dims): its multiply op (launch_relu_mult: the same column walk with one more gather) is the
             yardstick. Under relu="mrs" the evaluator plans hash, sign chain and multiply as one op, so the
             layer is built with relu="approx", whose ".C" op is that multiply alone (the same kernel)
Reported per form: the op's times, median and spread, the ratio to relu_mult's median of the same run, the launch
form (mul.lane / mul.staged / mul.sq) and the table bytes per element against 16 * mul_entries. DASH_MRS_STAGE=0
keeps the per-lane form: run the script once per setting, in separate processes, to compare k_mul_s with k_mul.

The profiled steps run eagerly (set_profile turns graph replay off), so the times are those of the kernels alone.

Needs a GPU: there is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

DIMS = (64, 16, 16)
LIM = 505  # 505^2 < M / 2 at k = 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--crt", type=int, default=7)
    ap.add_argument("--forms", default="elem,bcast,square,relu_mult")
    ap.add_argument("--label", default="", help="free text kept in the record")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/mul.py: no GPU visible (the benchmark has no CPU fallback)")

    import dash_amd as d
    from dash_amd.garbling import GarbledCircuit
    from dash_amd.ir.bases import first_primes
    from dash_amd.native import native
    from dash_amd.runtime import HipEvaluator

    n = native()
    B, N, C = args.batch, int(np.prod(DIMS)), DIMS[0]
    crt = first_primes(args.crt)
    rng = np.random.default_rng(1)
    xs = [rng.integers(-LIM, LIM + 1, N) for _ in range(B)]
    st = torch.cuda.current_stream()

    def circuit(form):
        if form == "elem":
            return d.Circuit([d.Flatten(DIMS), d.Mul(DIMS, -1)]), "mul#1", {}
        if form == "bcast":
            w = np.zeros((C, N), dtype=np.int64)
            w[np.arange(C), np.arange(C) * (N // C)] = 1
            mul = d.Mul(DIMS, 0, (C,))
            mul.in_src = -1
            return d.Circuit([d.Dense.from_quantized(w, np.zeros(C, dtype=np.int64)), mul]), "mul#1", {}
        if form == "square":
            return d.Circuit([d.Mul.square(DIMS)]), "mul#0", {}
        return d.Circuit([d.Relu(DIMS)]), "approx_relu#0.C", {"relu": "approx"}

    evs, info = {}, {}
    for form in args.forms.split(","):
        c, op, kw = circuit(form)
        gcs = [GarbledCircuit(c, args.crt, 100.0, seed=bytes([b + 1] * 16), device=0, **kw) for b in range(B)]
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
        log = [l.split()[0] for l in n.hip_launch_log_take() if l.startswith(("mul.", "relu_mult."))]
        ev.fetch_outputs(st)
        for b, gc in enumerate(gcs):
            assert np.array_equal(ev.decode(b, gc), gc.plain_q_eval(xs[b])), form
        ev.set_profile(True)
        evs[form] = (ev, op)
        li = len(c.layers) - 1
        tab = sum(int(np.asarray(a).nbytes) for a in gcs[0].model.layer_arrays(li).values())
        info[form] = {"op": op, "launch": sorted(set(log)), "table_bytes_per_element": tab / N}
        if form != "relu_mult":
            info[form]["entries_x16"] = 16 * n.mul_entries(crt, form == "square")
    times = {form: [] for form in evs}
    for _ in range(args.steps):
        for form, (ev, op) in evs.items():  # the forms alternate
            ev.upload_inputs_compressed(st)
            ev.run(st)
            torch.cuda.synchronize()
            t = [ms for name, ms in ev.op_times() if name == op]  # the multiply alone: no save, restore or dense op
            assert len(t) == 1, ev.op_times()
            times[form].append(t[0])
    rec = {"dims": list(DIMS), "batch": B, "crt": args.crt, "steps": args.steps, "warmup": args.warmup,
           "stage": os.environ.get("DASH_MRS_STAGE", "1"), "label": args.label, "forms": {}}
    for form, ts in times.items():
        rec["forms"][form] = dict(info[form], ms=[round(t, 4) for t in ts], median_ms=round(statistics.median(ts), 4),
                                  spread_ms=round(max(ts) - min(ts), 4))
    if "relu_mult" in rec["forms"]:
        y = rec["forms"]["relu_mult"]["median_ms"]
        for form, r in rec["forms"].items():
            r["ratio_to_relu_mult"] = round(r["median_ms"] / y, 3)
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
