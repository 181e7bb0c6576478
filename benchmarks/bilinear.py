"""The Bilinear layer's two kernel forms and the nearest Upsample of the same shapes, per-op hipEvent timers.

    python benchmarks/bilinear.py --batch 24 --steps 7 --warmup 3 --out profiles/bilinear_b24_run1.json

One-layer circuits at k = 7, one stream; every (shape, form) gets its own HipEvaluator with set_profile(True), the
forms alternate over the timed steps, all in one process. Shapes:
  c4    (4, 16, 16) -> (4, 32, 32), the score map of a segmentation head
  c64   (64, 16, 16) -> (64, 32, 32), a decoder feature map
each as <shape>.dword (k_bilinear4, the rule's pick for both), <shape>.byte (k_bilinear, forced with
DASH_BILINEAR_FORM=byte, which the evaluator reads when it plans; the same garbled circuits under both forms) and
<shape>.nearest (an Upsample layer by 2, k_copy_gather: the pure gather of the same bytes). Reported per form: the
op's times, median and spread, the launch line, the bytes the op must read and write once (label bytes of the input
plus those of the output, over all residues and GCs) and that bound's share of the time at the streaming rate
docs/ROOFLINE.md measures (5.6 TB/s; the HBM3E peak is 8 TB/s).

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

SHAPES = {"c4": (4, 16, 16), "c64": (64, 16, 16)}
STREAM_TBPS = 5.6  # docs/ROOFLINE.md: streaming whole rows of a buffer far larger than the caches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--crt", type=int, default=7)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--label", default="", help="free text kept in the record")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/bilinear.py: no GPU visible (the benchmark has no CPU fallback)")

    import dash_amd as d
    from dash_amd.garbling import GarbledCircuit
    from dash_amd.ir.bases import crt_modulus, first_primes
    from dash_amd.native import native
    from dash_amd.runtime import HipEvaluator

    n = native()
    B = args.batch
    base = first_primes(args.crt)
    comps = sum(int(math.floor(128.0 / math.log2(p))) for p in base)  # label bytes per element over all residues
    rng = np.random.default_rng(1)
    st = torch.cuda.current_stream()

    evs, info = {}, {}
    for shape in args.shapes.split(","):
        dims = SHAPES[shape]
        bl, up = d.Bilinear(dims, 2), d.Upsample(dims, 2)
        lim = (crt_modulus(base) // 2 - 1) >> bl.scale_bits  # the 2^s-scaled outputs stay signed CRT values
        for layer, forms in ((bl, ("dword", "byte")), (up, ("nearest",))):
            c = d.Circuit([layer])
            xs = [rng.integers(-lim, lim + 1, c.input_size) for _ in range(B)]
            gcs = [GarbledCircuit(c, args.crt, 100.0, seed=bytes([b + 1] * 16), device=0) for b in range(B)]
            for kform in forms:
                form = f"{shape}.{kform}"
                if kform == "byte":
                    os.environ["DASH_BILINEAR_FORM"] = "byte"
                else:
                    os.environ.pop("DASH_BILINEAR_FORM", None)
                ev = HipEvaluator(template=gcs[0].model, batch=B, device=0)
                os.environ.pop("DASH_BILINEAR_FORM", None)
                for b, gc in enumerate(gcs):
                    ev.load(b, gc.model)
                    ev.encode_compressed_into(b, gc, xs[b])
                n.hip_launch_log_take()
                n.hip_launch_log(True)
                for _ in range(args.warmup):
                    ev.upload_inputs_compressed(st)
                    ev.run(st)
                n.hip_launch_log(False)
                log = sorted({l for l in n.hip_launch_log_take() if l.startswith("bilinear.")})
                ev.fetch_outputs(st)
                for b, gc in enumerate(gcs):
                    assert np.array_equal(ev.decode(b, gc), gc.plain_q_eval(xs[b])), form
                ev.set_profile(True)
                op = f"{layer.name}#0"
                evs[form] = (ev, op)
                nbytes = B * comps * (layer.in_size + layer.out_size)
                info[form] = {"op": op, "launch": log, "nin": layer.in_size, "nout": layer.out_size, "bytes": nbytes,
                              "bound_ms": round(nbytes / (STREAM_TBPS * 1e12) * 1e3, 5)}
                if kform != "nearest":
                    assert all(l.startswith("bilinear." + kform) for l in log) and log, info[form]
    times = {form: [] for form in evs}
    for _ in range(args.steps):
        for form, (ev, op) in evs.items():  # the forms alternate
            ev.upload_inputs_compressed(st)
            ev.run(st)
            torch.cuda.synchronize()
            t = [ms for name, ms in ev.op_times() if name == op]
            assert len(t) == 1, ev.op_times()
            times[form].append(t[0])
    rec = {"batch": B, "crt": args.crt, "steps": args.steps, "warmup": args.warmup, "label": args.label,
           "stream_tbps": STREAM_TBPS, "forms": {}}
    for form, ts in times.items():
        med = statistics.median(ts)
        rec["forms"][form] = dict(info[form], ms=[round(t, 4) for t in ts], median_ms=round(med, 4),
                                  spread_ms=round(max(ts) - min(ts), 4),
                                  bound_over_median=round(info[form]["bound_ms"] / med, 3))
    for shape in args.shapes.split(","):
        dw, by, nn = (rec["forms"][f"{shape}.{k}"] for k in ("dword", "byte", "nearest"))
        dw["byte_over_dword"] = round(by["median_ms"] / dw["median_ms"], 3)
        dw["nearest_over_dword"] = round(nn["median_ms"] / dw["median_ms"], 3)
        dw["ahead_of_byte_in_every_pair"] = all(a < b for a, b in zip(dw["ms"], by["ms"]))
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
