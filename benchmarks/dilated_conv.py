"""Dilated conv against the undilated conv of equal MFMA work: the same C, F and image with a 3x3 at p = 1, which has
the same output size and the same number of k-steps; only the staged halo (dense) or the tap packing (grouped)
differs. That conv is the yardstick, and it exists before dilation does, so it can be measured from the parent tree.

    python benchmarks/dilated_conv.py --batch 24 --repeats 5 --out profiles/dilated_conv_b24.json

For every shape it builds a one-layer circuit per form, garbles B GCs on the GPU, loads one HipEvaluator per form
and times the conv op with set_profile(True) / op_times() after warm-up. The forms alternate, each runs `repeats`
times, all in one process. Forms:
  dilated    3x3, dilation d, pad d
  yardstick  3x3, undilated, pad 1 (same outputs, same MFMAs)
  info       3x3, undilated, pad d (the same staged image, more outputs; information only)
`--forms yardstick,info` runs on a tree without dilation too (the parent commit's yardstick); `--yardstick-json`
takes such a run's output and judges the bound against it. Dense: the dilated median is at most max(1.25, r) times
the yardstick's median plus the larger of the two spreads, r the ratio of LDS bytes staged per image between the two
plans (hip_conv_plan's staged_bytes). Grouped (the one-tap-per-dword form issues kw dot instructions per row where
the packed form issues ceil(kw / 4)): 3x the yardstick's median plus the larger spread.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

# (name, C, F, H = W, dilation, groups)
SHAPES = [("d2_c64_f64_16", 64, 64, 16, 2, 1), ("d2_c128_f128_8", 128, 128, 8, 2, 1), ("d4_c64_f64_16", 64, 64, 16, 4, 1),
          ("dw_d2_c64_16", 64, 64, 16, 2, 64)]
MARGIN = 1.25
GROUPED_FACTOR = 3.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--crt", type=int, default=7)
    ap.add_argument("--forms", default="dilated,yardstick,info")
    ap.add_argument("--yardstick-json", default=None, help="a --forms yardstick,info run of another tree to judge against")
    ap.add_argument("--label", default="", help="free text kept in the record (which tree)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.repeats >= 3
    want = args.forms.split(",")

    import torch

    import dash_amd as d
    from dash_amd.garbling import GarbledCircuit
    from dash_amd.ir.bases import first_primes
    from dash_amd.native import native
    from dash_amd.runtime import HipEvaluator

    other = None
    if args.yardstick_json:
        with open(args.yardstick_json) as f:
            other = {r["name"]: r for r in json.load(f)["shapes"]}
    B = args.batch
    st = torch.cuda.current_stream()
    results = []
    for name, C, F, HW, dil, g in SHAPES:
        rng = np.random.default_rng(C + F + HW + dil)
        w, b = rng.integers(-8, 9, (F, C // g, 3, 3)), rng.integers(-8, 9, F)

        def layer(pad, dl):
            kw = dict(pad_width=pad, pad_height=pad, groups=g)
            if dl > 1:  # (a tree without dilation builds the other forms)
                kw.update(dilation_width=dl, dilation_height=dl)
            return d.Conv2d.from_quantized(w, b, HW, HW, C, F, 3, 3, **kw)

        forms = {}
        if "dilated" in want:
            forms["dilated"] = layer(dil, dil)
        if "yardstick" in want:
            forms["yardstick"] = layer(1, 1)
        if "info" in want:
            forms["info"] = layer(dil, 1)
        xs = [rng.integers(-8, 9, C * HW * HW) for _ in range(B)]
        evs = {}
        for fname, l in forms.items():
            c = d.Circuit([l])
            gcs = [GarbledCircuit(c, args.crt, None, seed=bytes([bb + 1] * 16), device=0, hardened=True)
                   for bb in range(B)]
            ev = HipEvaluator(template=gcs[0].model, batch=B, device=0)
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
        rec = {"name": name, "C": C, "F": F, "H": HW, "W": HW, "k": 3, "dilation": dil, "groups": g, "batch": B,
               "crt": args.crt, "label": args.label}
        for fname, ts in times.items():
            rec[fname] = {"ms": [round(t, 4) for t in ts], "median_ms": round(statistics.median(ts), 4),
                          "spread_ms": round(max(ts) - min(ts), 4)}
        if "dilated" in rec:
            factor = GROUPED_FACTOR
            if g == 1:  # r: LDS bytes staged per image, dilated plan over yardstick plan
                crt = first_primes(args.crt)
                pd = native().hip_conv_plan(C, HW, HW, F, 3, 3, 1, 1, dil, dil, crt, True, dh=dil, dw=dil)
                py = native().hip_conv_plan(C, HW, HW, F, 3, 3, 1, 1, 1, 1, crt, True)
                r = pd["staged_bytes"] / py["staged_bytes"]
                rec["plan"] = {"dilated": {k: pd[k] for k in ("band", "nbands", "band_input_rows", "ldsR", "staged_bytes")},
                               "yardstick": {k: py[k] for k in ("band", "nbands", "band_input_rows", "ldsR", "staged_bytes")},
                               "r": round(r, 4)}
                factor = max(MARGIN, r)
            rec["factor"] = round(factor, 4)
            for key, y in (("same_tree", rec.get("yardstick")), ("other_tree", other[name]["yardstick"] if other else None)):
                if y is None:
                    continue
                bound = factor * y["median_ms"] + max(y["spread_ms"], rec["dilated"]["spread_ms"])
                rec["vs_yardstick_" + key] = {"yardstick_median_ms": y["median_ms"], "yardstick_spread_ms": y["spread_ms"],
                                              "ratio": round(rec["dilated"]["median_ms"] / y["median_ms"], 3),
                                              "bound_ms": round(bound, 4),
                                              "within_bound": bool(rec["dilated"]["median_ms"] <= bound)}
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del evs
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"margin": MARGIN, "grouped_factor": GROUPED_FACTOR, "label": args.label, "shapes": results}, f,
                      indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
