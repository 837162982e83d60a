#!/usr/bin/env python3
"""Native against composed cross-modal MAM attention in training (mmt_amd.train.ASYM_NATIVE), in one process with the
two sides alternated:

  op    forward + backward device time of HipOps.mam_attention_asym (mmt::mam_attention_asym_forward / _backward)
        and of asym_attention_from_mam(HipOps.mam_attention, ...) at the training shape (16 pairs: 32 sequences,
        128 template + 400 search tokens, 12 heads): each captured in a hipGraph (--per-graph calls), timed by HIP
        events over replays, --repeats timings per side; and the largest difference of the two sides' out / dqkv
  step  the captured TrainStep of build_asymmetric_shared at --batch pairs (forward, loss, backward, clip + AdamW in
        one hipGraph), one step object per side, replays timed in turn: samples/s, --repeats timings per side

    python tools/attn_asym_bwd_time.py --out profiles/attn_asym_bwd.jsonl

One JSON line per record, appended to --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-modal-tracking_amd"))
import torch  # noqa: E402


def _summary(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def op_time(args, emit):
    import mmt_amd.train as T
    Bh, n_t, n_s, H = args.batch, 128, 400, 12
    C = 64 * H
    g = torch.Generator().manual_seed(0)
    qkv = (torch.randn(2 * Bh, n_t + n_s, 3 * C, generator=g) * 0.5).bfloat16().cuda()
    dout = torch.randn(2 * Bh, n_t + n_s, C, generator=g).bfloat16().cuda()
    sides = {"native": lambda x: T._HipMamAttentionAsym.apply(x, Bh, n_t, H),
             "composed": lambda x: T.asym_attention_from_mam(T.HipOps.mam_attention, x, Bh, n_t, H)}
    graphs, results = {}, {}
    for name, fn in sides.items():
        x = qkv.clone().requires_grad_()

        def fwd_bwd(fn=fn, x=x):
            x.grad = None
            out = fn(x)
            out.backward(dout)
            return out

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                out = fwd_bwd()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        results[name] = (out.detach().float(), x.grad.detach().float())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(args.per_graph):
                fwd_bwd()
        graph.replay()
        torch.cuda.synchronize()
        graphs[name] = graph
    us = {name: [] for name in sides}
    for _ in range(args.repeats):
        for name, graph in graphs.items():  # alternated
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.replays):
                graph.replay()
            e1.record()
            torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / (args.replays * args.per_graph))
    (on, gn), (oc, gc) = results["native"], results["composed"]
    emit({"what": "op forward+backward, hipGraph replay", "sequences": 2 * Bh, "n_t": n_t, "n_s": n_s, "heads": H,
          "us_native": _summary(us["native"]), "us_composed": _summary(us["composed"]),
          "us_native_all": [round(x, 2) for x in us["native"]], "us_composed_all": [round(x, 2) for x in us["composed"]],
          "out_max_diff": (on - oc).abs().max().item(), "dqkv_max_diff": (gn - gc).abs().max().item(),
          "dqkv_max": gn.abs().max().item()})


def step_time(args, emit):
    import mmt_amd.model as M
    import mmt_amd.train as T
    steps, losses = {}, {}
    for name, native in (("native", True), ("composed", False)):
        torch.manual_seed(0)
        net = M.build_asymmetric_shared(M.hot_path_cfg(), train=False).cuda().train()
        batch = T.synthetic_batch(args.batch, "cuda", torch.Generator().manual_seed(3))
        T.ASYM_NATIVE = native  # read while the step is traced: the captured graph keeps its side
        try:
            step = T.TrainStep(net, T.HipOps, lr=1e-4)
            stats = step.capture(*batch, warmup=2)
            step.replay()
            torch.cuda.synchronize()
        finally:
            T.ASYM_NATIVE = True
        steps[name], losses[name] = step, float(stats["loss"])
    rate = {name: [] for name in steps}
    for _ in range(args.repeats):
        for name, step in steps.items():  # alternated
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                step.replay()
            e1.record()
            torch.cuda.synchronize()
            rate[name].append(args.batch * args.steps / (e0.elapsed_time(e1) * 1e-3))
    emit({"what": "captured TrainStep, build_asymmetric_shared", "pairs": args.batch, "steps_per_timing": args.steps,
          "samples_per_s_native": _summary(rate["native"]), "samples_per_s_composed": _summary(rate["composed"]),
          "native_all": [round(x, 1) for x in rate["native"]], "composed_all": [round(x, 1) for x in rate["composed"]],
          "loss_third_step_native": losses["native"], "loss_third_step_composed": losses["composed"]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_asym_bwd.jsonl"))
    ap.add_argument("--only", default="op,step")
    ap.add_argument("--batch", type=int, default=16, help="pairs (Bh): 2 x batch sequences")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--per-graph", type=int, default=10)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    out = open(args.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    if "op" in args.only.split(","):
        op_time(args, emit)
    if "step" in args.only.split(","):
        step_time(args, emit)
    out.close()


if __name__ == "__main__":
    main()
