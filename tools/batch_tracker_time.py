#!/usr/bin/env python3
"""Batched multi-sequence tracker against N single trackers, per sequence-frame, in one process:

  (a) N RGBTTrackerCore (one sequence each, one hipGraph replay and one host round trip per
      sequence-frame) stepped one after another -- code the batched tracker does not touch;
  (b) one RGBTBatchTrackerCore of N slots (one replay and one round trip per N sequence-frames)

on the same resident 480x640 uint8 frame pairs, bf16, update interval 200, the states put back to
the initial boxes before every step (as bench.py's tracker_step does: synthetic weights, the box
wanders).  The two sides alternate; each timing runs at least --seconds; --repeats gives the spread.

    python tools/batch_tracker_time.py --out profiles/batch_tracker_time.jsonl
    rocprofv3 --kernel-trace --stats -d <dir> -o bt -- python tools/batch_tracker_time.py --trace-run 64
    python tools/batch_tracker_time.py --kernel-stats <dir>/.../bt_kernel_stats.csv --slots 64

--trace-run N: only a few steps of side (b) at N slots, for the kernel trace; --kernel-stats CSV: the
crop-table and slot-update kernels' device time from that trace's stats file, appended to --out."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 480, 640
KERNELS = ("sample_target_table_kernel", "track_update_slots_kernel")


def kernel_stats(path, slots, variant):
    rec = {"what": "kernel_trace", "slots": slots, "variant": variant, "source": "rocprofv3 --kernel-trace --stats"}
    for row in csv.DictReader(open(path)):
        name = row.get("Name") or row.get("KernelName") or ""
        for k in KERNELS:
            if k in name:
                rec[k] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2),
                          "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_tracker_time.jsonl"))
    ap.add_argument("--slots", default="1,8,64")
    ap.add_argument("--variants", default="shared,rgbt")
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--trace-run", type=int, default=0)
    ap.add_argument("--kernel-stats", default="")
    args = ap.parse_args()
    out = open(args.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    if args.kernel_stats:
        emit(kernel_stats(args.kernel_stats, int(args.slots.split(",")[0]), args.variants.split(",")[0]))
        return

    sys.path.insert(0, os.path.join(ROOT, "multi-modal-tracking_amd"))
    import torch
    from mmt_amd import model as M
    from mmt_amd import synthetic
    from mmt_amd.tracking import RGBTBatchTrackerCore, RGBTTrackerCore

    assert torch.cuda.is_available(), "needs the MI355X"
    builders = {"shared": (M.build_mixformer_vit_rgbt_shared, True), "rgbt": (M.build_mixformer_vit_rgbt, False)}
    g = torch.Generator().manual_seed(5)
    frames = [[torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).cuda() for _ in range(2)]
              for _ in range(4)]

    def network(variant):
        net = builders[variant][0](M.hot_path_cfg(), train=False)
        keys = [(k, list(v.shape)) for k, v in net.state_dict().items()]
        net.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.synth_state_dict(keys).items()}, strict=True)
        return net.cuda().eval()

    def init_box(b):  # a different box per sequence, all well inside the frame
        return [W * 0.2 + 5.0 * (b % 32), H * 0.25 + 3.0 * (b % 24), 64.0, 48.0]

    def sides(net, variant, N):
        mm = builders[variant][1]
        singles = [RGBTTrackerCore(net, 2.0, 128, 5.0, 320, [200], multimodal=mm) for _ in range(N)]
        for b, c in enumerate(singles):
            c.initialize(frames[0], init_box(b))
        inits = [c.state.clone() for c in singles]
        batch = RGBTBatchTrackerCore(net, 2.0, 128, 5.0, 320, [200], multimodal=mm, slots=N)
        for b in range(N):
            batch.assign(b, frames[0], init_box(b))
        binit = batch.state.clone()

        def step_a(i):
            for b, c in enumerate(singles):
                c.state.copy_(inits[b])
                c.track(frames[(i + b) % 4])

        def step_b(i):
            batch.state.copy_(binit)
            r = batch.track({b: frames[(i + b) % 4] for b in range(N)})
            assert len(r) == N and not any(isinstance(v, Exception) for v in r.values())

        return step_a, step_b, batch

    def timed(step, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            step(i)
        return time.perf_counter() - t0  # every step ends in its host round trip

    if args.trace_run:
        variant = args.variants.split(",")[0]
        _, step_b, _ = sides(network(variant), variant, args.trace_run)
        timed(step_b, 30)
        return

    for variant in args.variants.split(","):
        net = network(variant)
        for N in [int(x) for x in args.slots.split(",")]:
            step_a, step_b, batch = sides(net, variant, N)
            n = {}
            for name, step in (("a", step_a), ("b", step_b)):  # warm-up (captures the graphs), then size the runs
                timed(step, 3)
                n[name] = max(5, int(args.seconds / (timed(step, 5) / 5)) + 1)
            rates = {"a": [], "b": []}
            for _ in range(args.repeats):
                for name, step in (("a", step_a), ("b", step_b)):
                    rates[name].append(N * n[name] / timed(step, n[name]))
            rec = {"what": "tracker_step", "variant": variant, "slots": N, "dtype": "bf16", "frame": [H, W],
                   "steps": n, "hip_graph": batch._graph is not None, "unit": "sequence-frames/s"}
            for name, key in (("a", "single_cores"), ("b", "batched_core")):
                r = sorted(rates[name])
                rec[key] = {"median": round(r[len(r) // 2], 1), "min": round(r[0], 1), "max": round(r[-1], 1)}
            rec["speedup_median"] = round(rec["batched_core"]["median"] / rec["single_cores"]["median"], 3)
            emit(rec)
            del step_a, step_b, batch
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
