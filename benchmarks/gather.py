"""The Gather layer's two kernel forms against each other, per-op hipEvent timers.

    python benchmarks/gather.py --batch 24 --steps 7 --warmup 3 --out profiles/gather_b24_run1.json

One-layer circuits at k = 7, one stream; every (shape, form) gets its own HipEvaluator with set_profile(True), the
forms alternate over the timed steps, all in one process. Shapes:
  shuffle  the channel shuffle with 2 groups of a (64, 16, 16) tensor (16384 -> 16384)
  halves   its channel halves, two Gathers of 8192 outputs; the second reads the circuit input through in_src, in
           place from the saved copy (the timed op)
  d2s      depth-to-space by 2 of a (64, 8, 8) tensor (4096 -> 4096, mode CRD: PixelShuffle)
  perm     a random permutation of 16384 elements
each as <shape>.dword (k_gather4, the rule's pick for all four) and <shape>.byte (the byte kernel k_copy_gather,
forced with DASH_GATHER_FORM=byte, which the evaluator reads when it plans): the same garbled circuits under both
forms. Reported per form: the op's times, median and spread, the launch line, and per shape the byte form's median
over the dword form's.

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

SHAPES = ("shuffle", "halves", "d2s", "perm")


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
        raise SystemExit("benchmarks/gather.py: no GPU visible (the benchmark has no CPU fallback)")

    import dash_amd as d
    from dash_amd.garbling import GarbledCircuit
    from dash_amd.ir.bases import crt_modulus, first_primes
    from dash_amd.native import native
    from dash_amd.runtime import HipEvaluator

    n = native()
    B = args.batch
    half = crt_modulus(first_primes(args.crt)) // 2
    rng = np.random.default_rng(1)
    st = torch.cuda.current_stream()

    def circuit(shape):
        """(circuit, timed op)"""
        if shape == "shuffle":
            return d.Circuit([d.Gather.channel_shuffle((64, 16, 16), 2)]), "gather#0"
        if shape == "halves":
            left, right = d.Gather.slice((64, 16, 16), 0, 0, 32), d.Gather.slice((64, 16, 16), 0, 32, 64)
            right.in_src = -1
            return d.Circuit([left, right]), "gather#1"
        if shape == "d2s":
            return d.Circuit([d.Gather.depth_to_space((64, 8, 8), 2, "CRD")]), "gather#0"
        return d.Circuit([d.Gather((16384,), np.random.default_rng(2).permutation(16384))]), "gather#0"

    evs, info = {}, {}
    for shape in args.shapes.split(","):
        c, op = circuit(shape)
        xs = [rng.integers(-half, half, c.input_size) for _ in range(B)]
        gcs = [GarbledCircuit(c, args.crt, 100.0, seed=bytes([b + 1] * 16), device=0) for b in range(B)]
        for kform in ("dword", "byte"):  # both kernel forms evaluate the same garbled circuits
            form = f"{shape}.{kform}"
            if kform == "byte":
                os.environ["DASH_GATHER_FORM"] = "byte"
            else:
                os.environ.pop("DASH_GATHER_FORM", None)
            ev = HipEvaluator(template=gcs[0].model, batch=B, device=0)
            os.environ.pop("DASH_GATHER_FORM", None)
            for b, gc in enumerate(gcs):
                ev.load(b, gc.model)
                ev.encode_compressed_into(b, gc, xs[b])
            n.hip_launch_log_take()
            n.hip_launch_log(True)
            for _ in range(args.warmup):
                ev.upload_inputs_compressed(st)
                ev.run(st)
            n.hip_launch_log(False)
            log = sorted({l for l in n.hip_launch_log_take() if l.startswith("gather.")})
            ev.fetch_outputs(st)
            for b, gc in enumerate(gcs):
                assert np.array_equal(ev.decode(b, gc), gc.plain_q_eval(xs[b])), form
            ev.set_profile(True)
            evs[form] = (ev, op)
            last = c.layers[-1]
            info[form] = {"op": op, "launch": log, "nin": last.in_size, "nout": last.out_size}
            assert all(l.startswith("gather." + kform) for l in log) and log, info[form]
    times = {form: [] for form in evs}
    for _ in range(args.steps):
        for form, (ev, op) in evs.items():  # the forms alternate
            ev.upload_inputs_compressed(st)
            ev.run(st)
            torch.cuda.synchronize()
            t = [ms for name, ms in ev.op_times() if name == op]  # the layer alone: no save op
            assert len(t) == 1, ev.op_times()
            times[form].append(t[0])
    rec = {"batch": B, "crt": args.crt, "steps": args.steps, "warmup": args.warmup, "label": args.label, "forms": {}}
    for form, ts in times.items():
        rec["forms"][form] = dict(info[form], ms=[round(t, 4) for t in ts], median_ms=round(statistics.median(ts), 4),
                                  spread_ms=round(max(ts) - min(ts), 4))
    for shape in args.shapes.split(","):
        dw, by = rec["forms"][shape + ".dword"], rec["forms"][shape + ".byte"]
        dw["byte_over_dword"] = round(by["median_ms"] / dw["median_ms"], 3)
        # the keep rule's first half: the dword form ahead in every alternating pair of this run
        dw["ahead_in_every_pair"] = all(a < b for a, b in zip(dw["ms"], by["ms"]))
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
