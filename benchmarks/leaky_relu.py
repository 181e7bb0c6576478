"""The LeakyRelu kernels next to the ReLU kernels they are modelled on, per-op hipEvent timers.

    python benchmarks/leaky_relu.py --batch 24 --steps 7 --warmup 3 --out profiles/leaky_relu_b24.json

Circuits over (64, 16, 16), k = 7, one stream; every form gets its own HipEvaluator with set_profile(True), the
forms alternate over the timed steps, all in one process. Forms:
  relu_mult        Relu(dims) with relu="approx": its ".C" op is launch_relu_mult alone (k_relu_mult_s here)
  leaky_mult       LeakyRelu(dims), one slope: the ".C" op is launch_leaky_mult alone (k_leaky_mult_s)
  leaky_mult_pc    the same with one slope per channel
  relu_out         Rescale(5) + Relu, rescale="mrs", relu="joint": the ReLU's ".C" op is the fused output kernel
                   (k_rescale_relu_out_t at this batch)
  leaky_out        Rescale(5) + LeakyRelu, one slope: k_rescale_leaky_out_t
  leaky_out_pc     the same with one slope per channel
Reported per form: the op's times, median and spread, the launch log names of the op, and the ratio of each leaky
form's median to its ReLU form's median of the same run. DASH_MRS_STAGE=0 keeps the per-lane multiply
(k_leaky_mult against k_relu_mult): run the script once per setting, in separate processes.

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
S_BITS, L_BITS = 4, 5
YARDSTICK = {"leaky_mult": "relu_mult", "leaky_mult_pc": "relu_mult", "leaky_out": "relu_out", "leaky_out_pc": "relu_out"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--crt", type=int, default=7)
    ap.add_argument("--forms", default="relu_mult,leaky_mult,leaky_mult_pc,relu_out,leaky_out,leaky_out_pc")
    ap.add_argument("--label", default="", help="free text kept in the record")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/leaky_relu.py: no GPU visible (the benchmark has no CPU fallback)")

    import dash_amd as d
    from dash_amd.garbling import GarbledCircuit
    from dash_amd.ir.bases import crt_modulus, first_primes
    from dash_amd.native import native
    from dash_amd.runtime import HipEvaluator

    n = native()
    B, N, C = args.batch, int(np.prod(DIMS)), DIMS[0]
    M = crt_modulus(first_primes(args.crt))
    h = M // 2
    rng = np.random.default_rng(1)
    lim = (h - 1) >> S_BITS
    x_mult = [rng.integers(-lim, lim + 1, N) for _ in range(B)]           # 2^s x stays a signed CRT value
    x_out = [rng.integers(-h, h - (1 << L_BITS), N) for _ in range(B)]    # the rescale's non-wrapping domain
    st = torch.cuda.current_stream()
    top = (1 << S_BITS) - 1
    per_channel = [(0, top, 1, top // 2 + 1, 2)[c % 5] for c in range(C)]

    def act(form):
        if form.startswith("relu"):
            return d.Relu(DIMS)
        return d.LeakyRelu.from_quantized(DIMS, per_channel if form.endswith("_pc") else 3, S_BITS)

    def circuit(form):
        a = act(form)
        if form.endswith(("_mult", "_mult_pc")):
            return d.Circuit([a]), f"{a.name}#0.C", {"relu": "approx"}, x_mult
        return d.Circuit([d.Rescale(L_BITS, DIMS), a]), f"{a.name}#1.C", {"rescale": "mrs", "relu": "joint"}, x_out

    evs, info = {}, {}
    for form in args.forms.split(","):
        c, op, kw, xs = circuit(form)
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
        log = [l.split()[0] for l in n.hip_launch_log_take()
               if l.startswith(("relu_mult.", "leaky_mult.", "relu_out.", "leaky_out."))]
        ev.fetch_outputs(st)
        for b, gc in enumerate(gcs):
            assert np.array_equal(ev.decode(b, gc), gc.plain_q_eval(xs[b])), form
        ev.set_profile(True)
        evs[form] = (ev, op)
        li = len(c.layers) - 1
        tab = sum(int(np.asarray(a).nbytes) for a in gcs[0].model.layer_arrays(li).values())
        info[form] = {"op": op, "launch": sorted(set(log)), "table_bytes_per_element": tab / N}
    times = {form: [] for form in evs}
    for _ in range(args.steps):
        for form, (ev, op) in evs.items():  # the forms alternate
            ev.upload_inputs_compressed(st)
            ev.run(st)
            torch.cuda.synchronize()
            t = [ms for name, ms in ev.op_times() if name == op]
            assert len(t) == 1, ev.op_times()
            times[form].append(t[0])
    rec = {"dims": list(DIMS), "batch": B, "crt": args.crt, "steps": args.steps, "warmup": args.warmup,
           "slope_bits": S_BITS, "rescale_bits": L_BITS, "stage": os.environ.get("DASH_MRS_STAGE", "1"),
           "label": args.label, "forms": {}}
    for form, ts in times.items():
        rec["forms"][form] = dict(info[form], ms=[round(t, 4) for t in ts], median_ms=round(statistics.median(ts), 4),
                                  spread_ms=round(max(ts) - min(ts), 4))
    for form, r in rec["forms"].items():
        y = rec["forms"].get(YARDSTICK.get(form, ""))
        if y:
            r["ratio_to_" + YARDSTICK[form]] = round(r["median_ms"] / y["median_ms"], 3)
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
