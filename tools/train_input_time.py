#!/usr/bin/env python3
"""Training input: what the device form of the reference's MixformerProcessing costs, for one batch of 16 samples of
480x640 frames at the 128 / 320 output sizes (six crops per sample).

  launches  the two mmt_train_crops_table launches alone (TrainInputProcessor.launch on resident frames and
            tables) between two device events, 50 calls after 3 warm-ups, repeated
  batch     process_batch end to end on host frames: the box arithmetic and validity on the host, the staging
            copy, the uploads and the two launches, synchronised; wall clock per batch
  host      process_sample_reference (numpy / torch on this job's CPUs, one process) per sample

Medians and ranges over --repeats runs; one JSON line per measurement.

    python tools/train_input_time.py --out profiles/train_input_time.jsonl"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H, W = 16, 480, 640


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_input_time.jsonl"))
    ap.add_argument("--what", default="launches,batch,host")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    what = args.what.split(",")
    out = open(args.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    sys.path.insert(0, os.path.join(ROOT, "multi-modal-tracking_amd"))
    import numpy as np
    import torch
    from mmt_amd.train_input import TrainInputConfig, TrainInputProcessor, draw_rolls, plan_sample, process_sample_reference

    cfg = TrainInputConfig()
    rng = np.random.default_rng(1)
    random.seed(1), np.random.seed(1), torch.manual_seed(1)

    def sample(k):
        frames = [[rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(2)] for _ in range(3)]
        boxes = []
        for _ in range(3):  # LasHeR-like targets: 30..160 pixels, inside the frame
            w, h = rng.uniform(30, 160, 2)
            b = np.array([rng.uniform(0, W - w), rng.uniform(0, H - h), w, h], np.float32)
            boxes.append([b, b + np.float32(1.5)])
        return ({"template": frames[:2], "search": frames[2:]}, {"template": boxes[:2], "search": boxes[2:]})

    samples, rolls = [], []
    while len(samples) < B:  # valid samples only: every entry does its work
        s, r = sample(len(samples)), draw_rolls()
        if plan_sample(s[0], s[1], r, cfg)[1]:
            samples.append(s)
            rolls.append(r)

    def stats(t, digits=3):
        t = sorted(t)
        return {"median": round(t[len(t) // 2], digits), "min": round(t[0], digits), "max": round(t[-1], digits)}

    common = {"batch": B, "frame": [H, W], "sizes": [cfg.template_size, cfg.search_size], "crops": 6 * B}
    if "host" in what:
        process_sample_reference(samples[0][0], samples[0][1], rolls[0], cfg)
        t = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            for s, r in zip(samples, rolls):
                process_sample_reference(s[0], s[1], r, cfg)
            t.append((time.perf_counter() - t0) / B * 1e3)
        emit(dict(common, what="host_process_sample_reference", unit="ms/sample", cpus=len(os.sched_getaffinity(0)),
                  threads=torch.get_num_threads(), **stats(t)))
    if what == ["host"]:
        return

    assert torch.cuda.is_available(), "needs the MI355X"
    proc = TrainInputProcessor(cfg, B, "cuda", frame_hw=(H, W))
    res = proc.process_batch(samples, rolls)
    torch.cuda.synchronize()
    assert bool(res["valid"].all())
    if "launches" in what:
        t = []
        for _ in range(args.repeats):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            for _ in range(3):
                proc.launch()
            ev[0].record()
            for _ in range(50):
                proc.launch()
            ev[1].record()
            torch.cuda.synchronize()
            t.append(ev[0].elapsed_time(ev[1]) * 1e3 / 50)
        written = B * 2 * (2 * 128 * 128 + 320 * 320) * (3 * 4 + 1)
        emit(dict(common, what="train_crops_two_launches", unit="us/batch", bytes_written=written, **stats(t, 2)))
    if "batch" in what:
        t = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                proc.process_batch(samples, rolls)
                torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) / 5 * 1e3)
        emit(dict(common, what="process_batch_end_to_end", unit="ms/batch", upload_bytes=B * 6 * H * W * 3,
                  cpus=len(os.sched_getaffinity(0)), **stats(t)))


if __name__ == "__main__":
    main()
