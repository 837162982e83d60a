#!/usr/bin/env python3
"""The deformable fusion front-ends timed on the MI355X in one process: hipGraph replays of the model alone on
resident inputs, bf16, the asymmetric shared model at B = 1 and 8 with

  * Attention_Fusion_Bimodal_LNSpecific (the default plan), Attention_Fusion_Bimodal, _LNSpecific_Sum and
    _LNSpecific_2 at 2 encoder layers -- the same launch list, only the weights behind it differ;
  * Attention_Fusion_Bimodal at 6 layers (the reference config's default): 28 more launches.

The sides alternate; each timing replays for at least --seconds after a warm-up and ends in a device
synchronise; --repeats timings per side give the median and the range (min, max).

    python tools/fusion_variants_time.py --out profiles/fusion_variants_time.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LNS = "Attention_Fusion_Bimodal_LNSpecific"
SIDES = [("lnspecific_2", LNS, 2), ("bimodal_2", "Attention_Fusion_Bimodal", 2), ("sum_2", LNS + "_Sum", 2),
         ("add2_2", LNS + "_2", 2), ("bimodal_6", "Attention_Fusion_Bimodal", 6)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fusion_variants_time.jsonl"))
    ap.add_argument("--variant", default="asym")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "multi-modal-tracking_amd"))
    import torch
    from mmt_amd import synthetic
    from mmt_amd.model import reference_state_dict_shapes
    from mmt_amd.runtime import MixFormerRGBTRuntime

    assert torch.cuda.is_available(), "needs the MI355X"
    out = open(args.out, "a")

    def timed(fn, seconds):
        """Calls of fn per second over at least `seconds`, ending in a synchronise."""
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        n, chunk = 0, 20
        t0 = time.perf_counter()
        while True:
            for _ in range(chunk):
                fn()
            torch.cuda.synchronize()
            n += chunk
            dt = time.perf_counter() - t0
            if dt >= seconds:
                return n / dt

    rts = {}
    for name, cls, layers in SIDES:
        keys = reference_state_dict_shapes(args.variant, fusion_layers=layers, fusion_class=cls)
        sd = {k: torch.from_numpy(v) for k, v in synthetic.synth_state_dict(keys).items()}
        rts[name] = MixFormerRGBTRuntime(sd, args.variant, dtype=torch.bfloat16)
    for B in [int(b) for b in args.batches.split(",")]:
        t, o, s = [[x.cuda() for x in grp] for grp in synthetic.synth_inputs(B)]
        graphs, launches = {}, {}
        for name, rt in rts.items():
            ws = rt.workspace(B)
            rt.load_inputs(ws, t, o, s)
            graphs[name] = rt.capture(B)
            launches[name] = len(ws["plan"])
        rates = {k: [] for k in graphs}
        for _ in range(args.repeats):
            for k, g in graphs.items():
                rates[k].append(B * timed(g.replay, args.seconds))
        base = statistics.median(rates["lnspecific_2"])
        rec = {"what": "fusion_front_end_graph_replay", "variant": args.variant, "dtype": "bf16", "B": B,
               "unit": "frames/s", "seconds": args.seconds, "repeats": args.repeats, "sides": {}}
        for k, r in rates.items():
            rec["sides"][k] = {"median": round(statistics.median(r), 1), "min": round(min(r), 1), "max": round(max(r), 1),
                               "launches": launches[k], "over_lnspecific_2": round(statistics.median(r) / base, 4)}
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()


if __name__ == "__main__":
    main()
