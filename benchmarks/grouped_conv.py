"""Depthwise conv through k_conv_grp against the only form the dense-only code could run: the same layer as a
block-diagonal zero-expanded dense Conv2d through the MFMA conv kernel.

    python benchmarks/grouped_conv.py --batch 24 --repeats 5 --out profiles/grouped_conv_b24.json

For every shape it builds a one-layer circuit in each form, garbles B GCs on the GPU, loads one HipEvaluator per
form and times the conv op with set_profile(True) / op_times() after warm-up. The two forms alternate, each runs
`repeats` times, all in one process. The two forms are not wire-equivalent (every expanded zero weight adds a
Z_p term), so only their decoded outputs are compared. Also printed: the bytes the layer must move (input plus
output activation bytes over all residues and components) and the rate that makes of each time.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

# MobileNet-on-CIFAR depthwise 3x3, pad 1: (C, H = W, stride)
SHAPES = [(64, 32, 1), (64, 32, 2), (128, 16, 1), (128, 16, 2)]
HBM_PEAK = 8.0e12  # bytes/s, MI355X HBM3E spec peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--crt", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.repeats >= 3

    import torch

    import dash_amd as d
    from dash_amd.garbling import GarbledCircuit
    from dash_amd.ir.bases import first_primes
    from dash_amd.native import native
    from dash_amd.runtime import HipEvaluator

    B = args.batch
    sum_n = sum(native().nr_comps(p) for p in first_primes(args.crt))
    st = torch.cuda.current_stream()
    results = []
    for C, HW, s in SHAPES:
        rng = np.random.default_rng(C + HW + s)
        w = rng.integers(-8, 9, (C, 1, 3, 3))
        b = rng.integers(-8, 9, C)
        we = np.zeros((C, C, 3, 3), dtype=np.int64)
        we[np.arange(C), np.arange(C)] = w[:, 0]
        forms = {
            "depthwise": d.Conv2d.from_quantized(w, b, HW, HW, C, C, 3, 3, s, s, pad_width=1, pad_height=1, groups=C),
            "expanded": d.Conv2d.from_quantized(we, b, HW, HW, C, C, 3, 3, s, s, pad_width=1, pad_height=1),
        }
        xs = [rng.integers(-8, 9, C * HW * HW) for _ in range(B)]
        evs, outs = {}, {}
        for name, layer in forms.items():
            c = d.Circuit([layer])
            gcs = [GarbledCircuit(c, args.crt, None, seed=bytes([bb + 1] * 16), device=0) for bb in range(B)]
            ev = HipEvaluator(template=gcs[0].model, batch=B, device=0)
            for bb, gc in enumerate(gcs):
                ev.load(bb, gc.model)
                ev.encode_compressed_into(bb, gc, xs[bb])
            for _ in range(args.warmup):
                ev.upload_inputs_compressed(st)
                ev.run(st)
            ev.fetch_outputs(st)
            outs[name] = [ev.decode(bb, gc) for bb, gc in enumerate(gcs)]
            ref = [gc.plain_q_eval(x) for gc, x in zip(gcs, xs)]
            assert all(np.array_equal(o, r) for o, r in zip(outs[name], ref)), name
            ev.set_profile(True)
            evs[name] = ev
        times = {name: [] for name in forms}
        for _ in range(args.repeats):
            for name, ev in evs.items():  # the two forms alternate
                ev.upload_inputs_compressed(st)
                ev.run(st)
                torch.cuda.synchronize()
                conv = [t for op, t in ev.op_times() if "conv" in op]
                assert len(conv) == 1, ev.op_times()
                times[name].append(conv[0])
        OH = (HW + 2 - 3) // s + 1
        nbytes = B * sum_n * (C * HW * HW + C * OH * OH)
        rec = {"C": C, "H": HW, "W": HW, "stride": s, "batch": B, "crt": args.crt, "sum_n": sum_n,
               "bytes_moved": nbytes}
        for name, ts in times.items():
            med = statistics.median(ts)
            rec[name] = {"ms": [round(t, 4) for t in ts], "median_ms": round(med, 4),
                         "spread_ms": round(max(ts) - min(ts), 4),
                         "bytes_per_s": round(nbytes / (med * 1e-3), 0),
                         "share_of_hbm_peak": round(nbytes / (med * 1e-3) / HBM_PEAK, 4)}
        rec["speedup"] = round(rec["expanded"]["median_ms"] / rec["depthwise"]["median_ms"], 2)
        rec["faster_by_more_than_spread"] = bool(
            rec["expanded"]["median_ms"] - rec["depthwise"]["median_ms"]
            > max(rec["expanded"]["spread_ms"], rec["depthwise"]["spread_ms"]))
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del evs
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"hbm_peak_bytes_per_s": HBM_PEAK, "shapes": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
