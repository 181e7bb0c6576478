"""Online time of one Clip layer against one Relu layer (docs/CLIP.md, "Measured").

    python scripts/clip_online.py [--n 16384] [--batch 24] [--steps 7] [--relu mrs]
    DASH_MRS_STAGE=0 python scripts/clip_online.py      # every staged kernel form off (per-lane forms)
    python scripts/clip_online.py --after-rescale [--clip separate,joint,joint-fused] [--n 16384,4096]
                                  [--batch 24,8,3] [--rounds 3]

Garbles B GCs of Circuit([Relu((N,))]) and of Circuit([Clip.from_quantized((N,), 0, 192)]) (hardened, k = 7),
loads each set into one evaluator (one stream), runs 3 warm-up steps and prints one JSON line with the median
per-op hipEvent times (HipEvaluator.set_profile, as scripts/ab_online.py --detail reports them) over the timed
steps, the layer totals, their ratio and the table bytes per element.

--after-rescale times a Rescale(5) + Clip(0, 192) pair (mixed-radix rescale, exact signs) instead, per op and in
total, for each --clip construction: "separate" (two sign chains of the Clip's own input), "joint" (docs/CLIP.md:
the lower sign from the rescale, the upper sign on the rescale's input; unfused kernels) and "joint-fused" (the
same GCs with hip_set_joint_fuse(1): k_rescale_clip_out_t). The evaluators of all constructions are built first;
then --rounds rounds alternate between them, each round 3 warm-up steps and --steps timed ones, so that the
constructions are compared on one device under the same neighbours. One JSON line per (N, batch): per
construction the median over all timed steps, the per-round medians (their spread is the run-to-run noise), the
per-op medians and the pair's table bytes per element.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))


def after_rescale(N, B, args):
    import numpy as np
    import torch

    import dash_amd as d
    from dash_amd.garbling import GarbledCircuit
    from dash_amd.native import native
    from dash_amd.runtime import HipEvaluator

    names = args.clip.split(",")
    assert names and all(n in ("separate", "joint", "joint-fused") for n in names), "bad --clip"
    rng = np.random.default_rng(0)
    c = d.Circuit([d.Rescale(5, (N,)), d.Clip.from_quantized((N,), 0, 192)])
    xs = [rng.integers(-300 * 32, 500 * 32, N) for _ in range(B)]
    res = {"device": torch.cuda.get_device_name(0), "N": N, "B": B, "steps": args.steps, "rounds": args.rounds}
    st = torch.cuda.current_stream()
    evs, outs = {}, {}
    base = native().hip_joint_fuse()
    for name in names:
        cons = "separate" if name == "separate" else "joint"
        gcs = [GarbledCircuit(c, 7, 100.0, seed=bytes([b + 1] * 16), rescale="mrs", relu="mrs", clip=cons, device=0)
               for b in range(B)]
        res[name + "_table_bytes_per_elem"] = gcs[0].table_bytes / N
        native().hip_set_joint_fuse(1 if name == "joint-fused" else 0)  # read when the evaluator plans
        try:
            ev = HipEvaluator(template=gcs[0].model, batch=B, device=0)
        finally:
            native().hip_set_joint_fuse(base)
        for b, gc in enumerate(gcs):
            ev.load(b, gc.model)
            ev.encode_compressed_into(b, gc, xs[b])
        ev.upload_inputs_compressed(st)
        ev.run(st)
        ev.fetch_outputs()
        outs[name] = [np.asarray(ev.decode(b, gc)) for b, gc in enumerate(gcs)]
        want = [np.clip(-((-x) // 32), 0, 192) for x in xs]
        assert all(np.array_equal(o, w) for o, w in zip(outs[name], want)), name + ": wrong outputs"
        evs[name] = ev
        del gcs
    per_op = {n: {} for n in names}
    totals = {n: [] for n in names}
    rounds = {n: [] for n in names}
    for _ in range(args.rounds):
        for name in names:
            ev = evs[name]
            ev.set_profile(False)
            for _ in range(3):
                ev.upload_inputs_compressed(st)
                ev.run(st)
            torch.cuda.synchronize()
            ev.set_profile(True)
            mine = []
            for _ in range(args.steps):
                ev.upload_inputs_compressed(st)
                ev.run(st)
                torch.cuda.synchronize()
                ops = [(op, ms) for op, ms in ev.op_times() if "." in op]
                for op, ms in ops:
                    per_op[name].setdefault(op, []).append(ms)
                mine.append(sum(ms for _, ms in ops))
            totals[name] += mine
            rounds[name].append(round(statistics.median(mine), 4))
    for name in names:
        res[name + "_pair_ms_median"] = round(statistics.median(totals[name]), 4)
        res[name + "_pair_ms_round_medians"] = rounds[name]
        res[name + "_ops_ms_median"] = {op: round(statistics.median(v), 4) for op, v in per_op[name].items()}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default=str(64 * 16 * 16), help="elements (with --after-rescale: a comma list)")
    ap.add_argument("--batch", default="24", help="GCs (with --after-rescale: a comma list)")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--relu", default="mrs", choices=["mrs", "approx"])
    ap.add_argument("--after-rescale", action="store_true", help="time a Rescale(5) + Clip(0, 192) pair")
    ap.add_argument("--clip", default="separate,joint", help="comma list of separate | joint | joint-fused")
    ap.add_argument("--rounds", type=int, default=3, help="alternations between the constructions")
    args = ap.parse_args()
    if args.after_rescale:
        for N in (int(v) for v in args.n.split(",")):
            for B in (int(v) for v in args.batch.split(",")):
                after_rescale(N, B, args)
        return
    args.n, args.batch = int(args.n), int(args.batch)
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
