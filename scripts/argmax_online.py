"""Online time of one ArgMax layer, split by level and op (docs/ARGMAX.md, "Measured").

    python scripts/argmax_online.py [--dims 21x32x32,10] [--batch 24] [--steps 7]

For each --dims entry: garbles B GCs of Circuit([ArgMax(dims)]) (hardened, k = 7), loads them into one evaluator
(one stream), checks the decoded outputs against np.argmax, runs 3 warm-up steps and prints one JSON line with
the median per-op hipEvent times (HipEvaluator.set_profile) over the timed steps, grouped by level
("lv<n>": {"diff", "idiff", "H", "iH", "mrs", "C"}; C is k_argmax_mult), the layer total, and the table bytes
per output against the entry formula of csrc/gadgets.h ArgMaxPlan.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))


def run(dims, B, steps):
    import numpy as np
    import torch

    import dash_amd as d
    from dash_amd.garbling import GarbledCircuit
    from dash_amd.ir.bases import first_primes
    from dash_amd.native import native
    from dash_amd.runtime import HipEvaluator

    K, P = dims[0], int(np.prod(dims[1:], dtype=np.int64))
    rng = np.random.default_rng(0)
    c = d.Circuit([d.ArgMax(dims)])
    gcs = [GarbledCircuit(c, 7, 100.0, seed=bytes([b + 1] * 16), device=0) for b in range(B)]
    xs = [rng.integers(-300, 500, K * P) for _ in range(B)]
    res = {"device": torch.cuda.get_device_name(0), "dims": list(dims), "B": B, "steps": steps,
           "table_bytes_per_output": gcs[0].table_bytes / P,
           "formula_bytes_per_output": 16 * native().argmax_entries(first_primes(7), K),
           "ops_per_level": [o for o, _ in native().argmax_op_entries(first_primes(7), K)]}
    ev = HipEvaluator(template=gcs[0].model, batch=B, device=0)
    for b, gc in enumerate(gcs):
        ev.load(b, gc.model)
        ev.encode_compressed_into(b, gc, xs[b])
    st = torch.cuda.current_stream()
    ev.upload_inputs_compressed(st)
    ev.run(st)
    ev.fetch_outputs()
    for b, gc in enumerate(gcs):
        assert np.array_equal(ev.decode(b, gc), np.argmax(xs[b].reshape(K, P), axis=0)), "wrong outputs"
    for _ in range(3):
        ev.upload_inputs_compressed(st)
        ev.run(st)
    torch.cuda.synchronize()
    ev.set_profile(True)
    per_op, totals = {}, []
    for _ in range(steps):
        ev.upload_inputs_compressed(st)
        ev.run(st)
        torch.cuda.synchronize()
        ops = [(op, ms) for op, ms in ev.op_times() if ".lv" in op]  # "argmax#0.lv<n>.<phase>"
        for op, ms in ops:
            per_op.setdefault(op, []).append(ms)
        totals.append(sum(ms for _, ms in ops))
    levels = {}
    for op, v in per_op.items():
        _, lv, phase = op.split(".", 2)
        levels.setdefault(lv, {})[phase] = round(statistics.median(v), 4)
    res["levels_ms_median"] = levels
    res["mult_ms_median"] = round(sum(l.get("C", 0.0) for l in levels.values()), 4)
    res["layer_ms_median"] = round(statistics.median(totals), 4)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="21x32x32,10", help="comma list of K or CxHxW")
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--steps", type=int, default=7)
    args = ap.parse_args()
    for spec in args.dims.split(","):
        run(tuple(int(v) for v in spec.split("x")), args.batch, args.steps)


if __name__ == "__main__":
    main()
