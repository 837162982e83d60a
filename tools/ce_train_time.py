#!/usr/bin/env python3
"""What candidate elimination costs and saves in training: the drop-in module's forward + backward (train() mode,
HIP ops, box loss, no optimizer) at 16 pairs (ViT-B, 128/320), captured in one hipGraph and timed by HIP events over
replays, for the asym module and for asym_ce at keep rates 0.7 and 0.85 (CTR_POINT mask); and the two kernels of the
differentiable part (mmt_ce_rows_gather, mmt_ce_index_invert) at the three bench stages (32 sequences, search
lengths 400 -> 280 -> 196 -> 138) and at the recovery.

    python tools/ce_train_time.py --out profiles/ce_train_time.jsonl
    python tools/ce_train_time.py --only asym --pkg <another checkout>/multi-modal-tracking_amd --tag parent ...

One JSON line per measurement, appended to --out.  --pkg times another checkout's package (the shared
backbone_forward_stacked before / after a change) with the same script; --repeats gives the run-to-run spread."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ce_train_time.jsonl"))
    ap.add_argument("--only", default="asym,asym_ce@0.7,asym_ce@0.85,kernels")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "multi-modal-tracking_amd"))
    ap.add_argument("--tag", default="")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, args.pkg)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import torch
    import mmt_amd.model as M
    import mmt_amd.train as T

    assert torch.cuda.is_available(), "needs the MI355X"
    out = open(args.out, "a")

    def emit(rec):
        rec["tag"] = args.tag
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    def module_time(variant, rate):
        torch.manual_seed(0)
        build = M.build_asymmetric_shared if variant == "asym" else M.build_asymmetric_shared_ce
        net = build(M.hot_path_cfg(), train=False).cuda().train()
        net.drop_path_rate = 0.0  # no random draws: the same work in every replay
        for m in net.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
        t, o, s, gt = T.synthetic_batch(args.batch, "cuda", torch.Generator().manual_seed(3))
        kw = {}
        if variant == "asym_ce":
            kw = {"ce_template_mask": T.ce_center_mask(args.batch, 8, "cuda"), "ce_keep_rate": rate}

        def fwd_bwd():
            _, coord = T.module_forward(net, t, o, s, T.HipOps, **kw)
            T.HipOps.box_loss(coord, gt)[0].backward()

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                net.zero_grad(set_to_none=True)
                fwd_bwd()
        torch.cuda.current_stream().wait_stream(side)
        net.zero_grad(set_to_none=True)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fwd_bwd()
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.replays):
                graph.replay()
            e1.record()
            torch.cuda.synchronize()
            ms.append(round(e0.elapsed_time(e1) / args.replays, 3))
        emit({"what": "module forward+backward, hipGraph replay", "variant": variant, "keep_rate": rate,
              "pairs": args.batch, "ms": ms, "ms_min": min(ms), "replays": args.replays})
        del graph

    def kernel_times():
        from gemm_ab import graph_time
        from mmt_amd.ops import ce_index_invert, ce_rows_gather
        S, C, n_t, N = 2 * args.batch, 768, 128, 400
        g = torch.Generator().manual_seed(1)
        lens = N
        for stage in range(3):
            keep = math.ceil(0.7 * lens)
            x = torch.randn(S, n_t + lens, C, device="cuda")
            order = torch.stack([torch.randperm(lens, generator=g)[:keep] for _ in range(S)]).int() + n_t
            idx = torch.cat([torch.arange(n_t, dtype=torch.int32).repeat(S, 1), order], 1).cuda()
            dy = torch.randn(S, n_t + keep, C, device="cuda")
            inv = ce_index_invert(idx, n_t + lens)
            mb = 2 * S * (n_t + keep) * C * 4 / 1e6
            for what, fn, moved in (("prune forward", lambda: ce_rows_gather(x, idx), mb),
                                    ("prune backward gather", lambda: ce_rows_gather(dy, inv),
                                     (S * (n_t + keep) + S * (n_t + lens)) * C * 4 / 1e6),
                                    ("index invert", lambda: ce_index_invert(idx, n_t + lens), None)):
                us = graph_time(fn, 200)
                emit({"what": "kernel " + what, "stage": stage, "S": S, "rows_in": n_t + lens, "rows_out": n_t + keep,
                      "us": round(us, 2), "GB_per_s": round(moved / us * 1e3, 1) if moved else None})
            lens = keep
        x = torch.randn(S, n_t + lens, C, device="cuda")
        gidx = torch.stack([torch.randperm(N, generator=g)[:lens] for _ in range(S)]).int() + n_t
        idx = ce_index_invert(torch.cat([torch.arange(n_t, dtype=torch.int32).repeat(S, 1), gidx], 1).cuda(), n_t + N)
        us = graph_time(lambda: ce_rows_gather(x, idx), 200)
        emit({"what": "kernel recover forward", "S": S, "rows_in": n_t + lens, "rows_out": n_t + N, "us": round(us, 2),
              "GB_per_s": round((S * (n_t + lens) + S * (n_t + N)) * C * 4 / 1e6 / us * 1e3, 1)})

    for item in args.only.split(","):
        if item == "kernels":
            kernel_times()
        elif item == "asym":
            module_time("asym", None)
        else:
            variant, rate = item.split("@")
            module_time(variant, float(rate))
    out.close()


if __name__ == "__main__":
    main()
