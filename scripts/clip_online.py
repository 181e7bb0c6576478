"""Online time of one Clip layer against one Relu layer (docs/CLIP.md, "Measured").

    python scripts/clip_online.py [--n 16384] [--batch 24] [--steps 7] [--relu mrs]
    DASH_MRS_STAGE=0 python scripts/clip_online.py      # every staged kernel form off (per-lane forms)

Garbles B GCs of Circuit([Relu((N,))]) and of Circuit([Clip.from_quantized((N,), 0, 192)]) (hardened, k = 7),
loads each set into one evaluator (one stream), runs 3 warm-up steps and prints one JSON line with the median
per-op hipEvent times (HipEvaluator.set_profile, as scripts/ab_online.py --detail reports them) over the timed
steps, the layer totals, their ratio and the table bytes per element.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64 * 16 * 16)
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--relu", default="mrs", choices=["mrs", "approx"])
    args = ap.parse_args()
    import numpy as np
    import torch

    import dash_amd as d
    from dash_amd.garbling import GarbledCircuit
    from dash_amd.runtime import HipEvaluator

    N, B = args.n, args.batch
    rng = np.random.default_rng(0)
    res = {"device": torch.cuda.get_device_name(0), "N": N, "B": B, "steps": args.steps, "relu": args.relu,
           "DASH_MRS_STAGE": os.environ.get("DASH_MRS_STAGE", "")}
    for name, layer in (("relu", d.Relu((N,))), ("clip", d.Clip.from_quantized((N,), 0, 192))):
        c = d.Circuit([layer])
        gcs = [GarbledCircuit(c, 7, 100.0, seed=bytes([b + 1] * 16), relu=args.relu, hardened=True, device=0)
               for b in range(B)]
        res[name + "_table_bytes_per_elem"] = gcs[0].table_bytes / N
        ev = HipEvaluator(template=gcs[0].model, batch=B, device=0)
        for b, gc in enumerate(gcs):
            ev.load(b, gc.model)
            ev.encode_compressed_into(b, gc, rng.integers(-300, 500, N))
        st = torch.cuda.current_stream()
        for _ in range(3):
            ev.upload_inputs_compressed(st)
            ev.run(st)
        torch.cuda.synchronize()
        ev.set_profile(True)
        per_op, totals = {}, []
        for _ in range(args.steps):
            ev.upload_inputs_compressed(st)
            ev.run(st)
            torch.cuda.synchronize()
            layer_ops = [(op, ms) for op, ms in ev.op_times() if "." in op]  # the layer's ops: "<layer>#i.<phase>"
            for op, ms in layer_ops:
                per_op.setdefault(op, []).append(ms)
            totals.append(sum(ms for _, ms in layer_ops))
        res[name + "_ops_ms_median"] = {op: round(statistics.median(v), 4) for op, v in per_op.items()}
        res[name + "_layer_ms_median"] = round(statistics.median(totals), 4)
        del ev, gcs
    res["ratio"] = round(res["clip_layer_ms_median"] / res["relu_layer_ms_median"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
