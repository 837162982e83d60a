#!/usr/bin/env python3
"""RGBT_Fusion_Cat timed on the MI355X in one process, bf16, the asymmetric shared model:

  * frames/s of hipGraph replays of the model alone on resident inputs, asym + RGBT_Fusion_Cat against asym +
    Attention_Fusion_Bimodal_LNSpecific (2 layers, the default plan), at B = 1 and 8, the two sides alternating
    --repeats times (median and range);
  * the in-frame time of each of the three fusion convs (tools/plan_entry_ab.time_entry: back-to-back launches of
    the plan entry, in place, in one hipGraph, HIP events), the kernel mmt_gemm_select chose for it, and the first
    conv under a few forced (impl, splitk) choices;
  * each conv's two floors: its weight bytes at the HBM rate and its FLOPs at the dense bf16 MFMA rate.

    python tools/fusion_cat_time.py --out profiles/fusion_cat_time.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-modal-tracking_amd"))
sys.path.insert(0, ROOT)
SIDES = [("cat", "RGBT_Fusion_Cat"), ("lnspecific_2", "Attention_Fusion_Bimodal_LNSpecific")]
HBM_BYTES_PER_US = 6.3e6   # MI355X: 8 TB/s peak, ~6.3 TB/s achievable by a streaming copy
MFMA_FLOP_PER_US = 2.5e9   # dense bf16 MFMA peak, 2.5 PFLOP/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fusion_cat_time.jsonl"))
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cfgs", default="3:1,3:0,2:0,1:0,4:0,-1:0")
    args = ap.parse_args()
    import torch
    from mmt_amd import _lib as L
    from mmt_amd import synthetic
    from mmt_amd.model import reference_state_dict_shapes
    from mmt_amd.runtime import MixFormerRGBTRuntime
    from tools.plan_entry_ab import time_entry

    assert torch.cuda.is_available(), "needs the MI355X"
    out = open(args.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    def timed(fn, seconds):
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
    for name, cls in SIDES:
        keys = reference_state_dict_shapes("asym", fusion_layers=2, fusion_class=cls)
        sd = {k: torch.from_numpy(v) for k, v in synthetic.synth_state_dict(keys).items()}
        rts[name] = MixFormerRGBTRuntime(sd, "asym", dtype=torch.bfloat16)
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
        rec = {"what": "fusion_cat_graph_replay", "variant": "asym", "dtype": "bf16", "B": B, "unit": "frames/s",
               "seconds": args.seconds, "repeats": args.repeats, "sides": {}}
        for k, r in rates.items():
            rec["sides"][k] = {"median": round(statistics.median(r), 1), "min": round(min(r), 1), "max": round(max(r), 1),
                               "launches": launches[k], "over_lnspecific_2": round(statistics.median(r) / base, 4)}
        emit(rec)
        # the three convs in place in the Cat plan
        rt = rts["cat"]
        plan = rt.workspace(B)["plan"]
        rt.run_plan(plan)
        torch.cuda.synchronize()
        for nm in ("fusion_cat1", "fusion_cat2", "fusion_cat3"):
            fn, fargs, _, p = next(e for e in plan if e[2] == nm)
            c = L.gemm_select(p, L.MMT_BF16)
            wbytes, flop = 2 * p.N * p.K, 2.0 * p.M * p.N * p.K
            row = {"what": "fusion_cat_conv_in_frame", "B": B, "name": nm, "M": p.M, "N": p.N, "K": p.K,
                   "k_split": p.k_split, "unit": "us",
                   "select": {"family": {L.GEMM_REG_TILE: "register-staged", L.GEMM_LDS_DMA: "LDS-DMA"}[c.family],
                              "cfg": c.cfg, "bm": c.bm, "bn": c.bn, "kgroups": c.kgroups, "nsk": c.nsk, "epi": c.epi,
                              "wgs": c.wgs},
                   "auto": round(time_entry(fn, fargs), 2),
                   "floor_weights_hbm": round(wbytes / HBM_BYTES_PER_US, 2), "floor_mfma": round(flop / MFMA_FLOP_PER_US, 2)}
            if nm == "fusion_cat1":
                saved = (p.impl, p.splitk)
                for cfg in args.cfgs.split(","):
                    p.impl, p.splitk = (int(v) for v in cfg.split(":"))
                    if L.gemm_select(p, L.MMT_BF16) is not None:
                        row["impl:splitk " + cfg] = round(time_entry(fn, fargs), 2)
                p.impl, p.splitk = saved
            emit(row)


if __name__ == "__main__":
    main()
