"""Transposed conv through the sub-pixel view (launch_conv's scatter epilogue) against the dense conv of equal
work: the stride-1 Conv2d with the view's geometry (same MFMA count, same staged bytes, essentially the same output
bytes), which is what the layer costs without the scatter.

    python benchmarks/conv_transpose.py --batch 24 --repeats 5 --out profiles/conv_transpose_b24.json

For every shape it builds a one-layer circuit per form, garbles B GCs on the GPU, loads one HipEvaluator per form
and times the conv op with set_profile(True) / op_times() after warm-up. The forms alternate, each runs `repeats`
times, all in one process. Forms:
  convt      the transposed layer (wide four-byte stores where sw = 2, unless DASH_CONVT_WIDE=0 is set: the byte
             store A/B is a second run of this script, since the knob is read once per process)
  yardstick  the equal-work Conv2d
  convt_valu the transposed layer with the evaluator's mfma=False switch (information only)
`--forms yardstick` runs on a tree without the layer too (the parent commit's yardstick); `--yardstick-json` takes
such a run's output and judges the acceptance margin against it: the transposed layer's median is at most 1.25x
that yardstick's median plus the larger of the two spreads.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

# (name, C, F, H = W, k, stride, pad): decoder steps of an encoder-decoder on CIFAR-sized inputs
SHAPES = [("k2s2_c64_f32_16", 64, 32, 16, 2, 2, 0), ("k2s2_c128_f64_8", 128, 64, 8, 2, 2, 0),
          ("k4s2p1_c64_f32_16", 64, 32, 16, 4, 2, 1)]
MARGIN = 1.25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--crt", type=int, default=7)
    ap.add_argument("--forms", default="convt,yardstick,convt_valu")
    ap.add_argument("--yardstick-json", default=None, help="a --forms yardstick run of another tree to judge against")
    ap.add_argument("--label", default="", help="free text kept in the record (which tree / which knob)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.repeats >= 3
    want = args.forms.split(",")

    import torch

    import dash_amd as d
    from dash_amd.garbling import GarbledCircuit
    from dash_amd.runtime import HipEvaluator

    other = None
    if args.yardstick_json:
        with open(args.yardstick_json) as f:
            other = {r["name"]: r for r in json.load(f)["shapes"]}
    B = args.batch
    st = torch.cuda.current_stream()
    results = []
    for name, C, F, HW, k, s, p in SHAPES:
        rng = np.random.default_rng(C + F + HW + k)
        T = -(-k // s)
        forms = {}
        if "yardstick" in want:  # the view's geometry as a plain conv: T x T taps, pad T - 1, F s s filters
            forms["yardstick"] = (d.Conv2d.from_quantized(rng.integers(-8, 9, (F * s * s, C, T, T)),
                                                          rng.integers(-8, 9, F * s * s), HW, HW, C, F * s * s, T, T,
                                                          pad_width=T - 1, pad_height=T - 1), True)
        if "convt" in want or "convt_valu" in want:
            layer = d.ConvTranspose2d.from_quantized(rng.integers(-8, 9, (C, F, k, k)), rng.integers(-8, 9, F), HW, HW,
                                                     C, F, k, k, s, s, pad_width=p, pad_height=p)
            if "convt" in want:
                forms["convt"] = (layer, True)
            if "convt_valu" in want:
                forms["convt_valu"] = (layer, False)
        xs = [rng.integers(-8, 9, C * HW * HW) for _ in range(B)]
        evs = {}
        for fname, (layer, mfma) in forms.items():
            c = d.Circuit([layer])
            gcs = [GarbledCircuit(c, args.crt, None, seed=bytes([bb + 1] * 16), device=0, hardened=True)
                   for bb in range(B)]
            ev = HipEvaluator(template=gcs[0].model, batch=B, device=0, mfma=mfma)
            for bb, gc in enumerate(gcs):
                ev.load(bb, gc.model)
                ev.encode_compressed_into(bb, gc, xs[bb])
            for _ in range(args.warmup):
                ev.upload_inputs_compressed(st)
                ev.run(st)
            ev.fetch_outputs(st)
            for bb, gc in enumerate(gcs):
                assert np.array_equal(ev.decode(bb, gc), gc.plain_q_eval(xs[bb])), fname
            ev.set_profile(True)
            evs[fname] = ev
        times = {fname: [] for fname in forms}
        for _ in range(args.repeats):
            for fname, ev in evs.items():  # the forms alternate
                ev.upload_inputs_compressed(st)
                ev.run(st)
                torch.cuda.synchronize()
                conv = [t for op, t in ev.op_times() if "conv" in op]
                assert len(conv) == 1, ev.op_times()
                times[fname].append(conv[0])
        rec = {"name": name, "C": C, "F": F, "H": HW, "W": HW, "k": k, "stride": s, "pad": p, "batch": B,
               "crt": args.crt, "label": args.label}
        for fname, ts in times.items():
            rec[fname] = {"ms": [round(t, 4) for t in ts], "median_ms": round(statistics.median(ts), 4),
                          "spread_ms": round(max(ts) - min(ts), 4)}
        if "convt" in rec:
            for key, y in (("same_tree", rec.get("yardstick")), ("other_tree", other[name]["yardstick"] if other else None)):
                if y is None:
                    continue
                bound = MARGIN * y["median_ms"] + max(y["spread_ms"], rec["convt"]["spread_ms"])
                rec["vs_yardstick_" + key] = {"yardstick_median_ms": y["median_ms"], "yardstick_spread_ms": y["spread_ms"],
                                              "ratio": round(rec["convt"]["median_ms"] / y["median_ms"], 3),
                                              "bound_ms": round(bound, 4),
                                              "within_margin": bool(rec["convt"]["median_ms"] <= bound)}
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del evs
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"margin": MARGIN, "label": args.label, "shapes": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
