"""The PiecewiseLinear kernels next to the ReLU multiply they replace m of, per-op hipEvent timers.

    python benchmarks/pwl.py --batch 24 --steps 7 --warmup 3 --out profiles/pwl_b24.json

Circuits over (64, 16, 16), k = 7, one stream; every form gets its own HipEvaluator with set_profile(True), the
forms alternate over the timed steps, all in one process. Forms:
  relu_mult   Relu(dims) with relu="approx": its ".C" op is launch_relu_mult alone (k_relu_mult_s here)
  pwl_m2      PiecewiseLinear.hard_sigmoid (2 breakpoints), exact sign: ".K" is k_label_key, ".b<i>.mrs" the sign
              chains, ".C" launch_pwl_mult alone (k_pwl_mult_s<2>)
  pwl_m8      PiecewiseLinear.sigmoid (8 breakpoints): k_pwl_mult_s<8>
Reported per form: the multiply's times, median and spread; for the pwl forms also the key pass and the sum of the m
sign launches, and the ratio of the multiply's median to the ReLU multiply's median of the same run, to be read
against m (what the kernel replaces is m ReLU multiplies, each with its own read and write of the label).
DASH_MRS_STAGE=0 keeps the per-lane multiply (k_pwl_mult against k_relu_mult): a separate process.

The GCs are garbled on the device straight into the evaluator's slots. The profiled steps run eagerly (set_profile
turns graph replay off), so the times are those of the kernels alone.

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
L_BITS = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--crt", type=int, default=7)
    ap.add_argument("--slope-bits", type=int, default=8)
    ap.add_argument("--forms", default="relu_mult,pwl_m2,pwl_m8")
    ap.add_argument("--label", default="", help="free text kept in the record")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/pwl.py: no GPU visible (the benchmark has no CPU fallback)")

    import dash_amd as d
    from dash_amd.garbling import GarbledCircuit
    from dash_amd.native import native
    from dash_amd.runtime import HipEvaluator

    n = native()
    B, N = args.batch, int(np.prod(DIMS))
    rng = np.random.default_rng(1)
    xs = [rng.integers(-400, 401, N) for _ in range(B)]  # +-12.5 at l = 5: every segment of both functions
    st = torch.cuda.current_stream()

    def circuit(form):
        if form == "relu_mult":
            return d.Circuit([d.Relu(DIMS)]), {"relu": "approx"}
        ctor = d.PiecewiseLinear.hard_sigmoid if form == "pwl_m2" else d.PiecewiseLinear.sigmoid
        return d.Circuit([ctor(DIMS, slope_bits=args.slope_bits, q_parameter=L_BITS)]), {"relu": "mrs"}

    evs, info = {}, {}
    for form in args.forms.split(","):
        c, kw = circuit(form)
        name = c.layers[0].name
        first = GarbledCircuit(c, args.crt, 100.0, seed=bytes([1] * 16), device=0, **kw)
        ev = HipEvaluator(template=first.model, batch=B, device=0)
        ev.load(0, first.model)
        gcs = [first]
        for b in range(1, B):  # the tables go straight into the evaluator's slot
            gcs.append(GarbledCircuit(c, args.crt, 100.0, seed=bytes([b + 1] * 16), device=0, sink=ev.sink(b), **kw))
            ev.load(b, gcs[-1].model)
        for b, gc in enumerate(gcs):
            ev.encode_compressed_into(b, gc, xs[b])
        n.hip_launch_log_take()
        n.hip_launch_log(True)
        for _ in range(args.warmup):
            ev.upload_inputs_compressed(st)
            ev.run(st)
        n.hip_launch_log(False)
        log = [l.split()[0] for l in n.hip_launch_log_take() if l.startswith(("relu_mult.", "pwl_mult."))]
        ev.fetch_outputs(st)
        for b in (0, B - 1):
            assert np.array_equal(ev.decode(b, gcs[b]), gcs[b].plain_q_eval(xs[b])), form
        ev.set_profile(True)
        evs[form] = (ev, name)
        tab = sum(int(np.prod(a.shape)) * 16 for a in first.model.layer_arrays(0).values())
        m = len(c.layers[0].kept) if name == "pwl" else 1
        info[form] = {"m": m, "launch": sorted(set(log)), "table_bytes_per_element": tab / N}
    times = {form: {"mult": [], "key": [], "signs": []} for form in evs}
    for _ in range(args.steps):
        for form, (ev, name) in evs.items():  # the forms alternate
            ev.upload_inputs_compressed(st)
            ev.run(st)
            torch.cuda.synchronize()
            ops = ev.op_times()
            t = [ms for op, ms in ops if op == f"{name}#0.C"]
            assert len(t) == 1, ops
            times[form]["mult"].append(t[0])
            if name == "pwl":
                times[form]["key"].append(sum(ms for op, ms in ops if op == "pwl#0.K"))
                sg = [ms for op, ms in ops if op.startswith("pwl#0.b")]
                assert len(sg) == info[form]["m"], ops
                times[form]["signs"].append(sum(sg))
    rec = {"dims": list(DIMS), "batch": B, "crt": args.crt, "steps": args.steps, "warmup": args.warmup,
           "slope_bits": args.slope_bits, "q_parameter": L_BITS, "stage": os.environ.get("DASH_MRS_STAGE", "1"),
           "label": args.label, "forms": {}}

    def stat(ts):
        return {"ms": [round(t, 4) for t in ts], "median_ms": round(statistics.median(ts), 4),
                "spread_ms": round(max(ts) - min(ts), 4)}

    for form, ts in times.items():
        r = dict(info[form], **stat(ts["mult"]))
        if ts["key"]:
            r["key"] = stat(ts["key"])
            r["signs"] = stat(ts["signs"])
        rec["forms"][form] = r
    y = rec["forms"].get("relu_mult")
    for form, r in rec["forms"].items():
        if y and form != "relu_mult":
            r["ratio_to_relu_mult"] = round(r["median_ms"] / y["median_ms"], 3)
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
