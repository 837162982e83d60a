#!/usr/bin/env python3
"""The TRAIN.TRAIN_SCORE step (mmt_amd.train.ScoreTrainStep) three ways, in one process, alternating in the same
run, each side on its own equal-state copy of the weights:

  (a) ScoreTrainStep(net, rt): the frozen trunk on the inference runtime, the decoder as eager PyTorch in fp32,
      clip_grad_norm_ + torch.optim.AdamW;
  (b) ScoreTrainStep(net, rt, ops=HipOps), stepped eagerly;
  (c) the same after capture(): one hipGraph replay per step.

asym_online ViT-B 128/320, bf16 runtime, B = 16 synthetic pairs with random 0/1 labels.  Each timing runs at
least --seconds, --repeats gives the spread (median and range).  One `score_train_step` record (steps/s and
samples/s per side) is appended to --out.  --kernel-stats: a torch.profiler pass over a few replays of (c) adds
the share of device kernel time that is libmmt_hip's against aten / vendor-library kernels.

Every phase (set-up, each timing, the profile) runs under its own time limit (--phase-limit seconds: the alarm
ends the process), and the first failure ends the run.

    timeout -k 10 600 python tools/score_train_time.py --kernel-stats --out profiles/score_train_time.jsonl"""
import argparse
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_OURS = ("at::", "at_cuda_detail", "Cijk_", "rocblas", "hipblas", "miopen", "rocprim", "Memcpy", "Memset",
            "elementwise_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_train_time.jsonl"))
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--phase-limit", type=int, default=120)
    ap.add_argument("--kernel-stats", action="store_true")
    args = ap.parse_args()

    def phase(name):
        signal.alarm(args.phase_limit)  # SIGALRM's default action ends the process
        print("# " + name, file=sys.stderr, flush=True)

    phase("set-up")
    sys.path.insert(0, os.path.join(ROOT, "multi-modal-tracking_amd"))
    import torch
    from mmt_amd import synthetic
    from mmt_amd.model import build_asymmetric_shared_online_score, hot_path_cfg
    from mmt_amd.runtime import MixFormerRGBTRuntime
    from mmt_amd.train import HipOps, ScoreTrainStep

    assert torch.cuda.is_available(), "needs the MI355X"
    B = args.batch
    proto = build_asymmetric_shared_online_score(hot_path_cfg(), train=False)
    keys = [(k, list(v.shape)) for k, v in proto.state_dict().items()]
    sd = {k: torch.from_numpy(v) for k, v in synthetic.synth_state_dict(keys).items()}
    rt = MixFormerRGBTRuntime(sd, "asym_online", dtype=torch.bfloat16)

    def network():
        net = build_asymmetric_shared_online_score(hot_path_cfg(), train=False)
        net.load_state_dict(sd, strict=True)
        return net.cuda().eval()

    t, o, s = synthetic.synth_inputs(B)
    t, o, s = [x.cuda() for x in t], [x.cuda() for x in o], [x.cuda() for x in s]
    labels = torch.randint(0, 2, (B,), generator=torch.Generator().manual_seed(3)).float().cuda()
    steps = {"a": ScoreTrainStep(network(), rt), "b": ScoreTrainStep(network(), rt, ops=HipOps),
             "c": ScoreTrainStep(network(), rt, ops=HipOps)}
    steps["c"].capture(t, o, s, labels, warmup=2)
    run = {"a": lambda: steps["a"](t, o, s, labels), "b": lambda: steps["b"](t, o, s, labels),
           "c": lambda: steps["c"].replay()}

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    n = {}
    for name in "abc":
        phase("warm-up " + name)
        timed(run[name], 3)
        n[name] = max(5, int(args.seconds / (timed(run[name], 5) / 5)) + 1)
    rates = {k: [] for k in "abc"}
    for r in range(args.repeats):
        for name in "abc":
            phase("timing %s %d" % (name, r))
            rates[name].append(n[name] / timed(run[name], n[name]))
    rec = {"what": "score_train_step", "variant": "asym_online", "model": "vit_b_128_320", "dtype": "bf16", "batch": B,
           "steps": n, "seconds_min": args.seconds, "repeats": args.repeats}
    for name, key in (("a", "eager_torch"), ("b", "hip_eager"), ("c", "hip_graph_replay")):
        r = sorted(rates[name])
        rec[key] = {"steps_per_s": {"median": round(r[len(r) // 2], 2), "min": round(r[0], 2), "max": round(r[-1], 2)},
                    "samples_per_s": {"median": round(B * r[len(r) // 2], 1), "min": round(B * r[0], 1),
                                      "max": round(B * r[-1], 1)}}
    for name, key in (("b", "hip_eager"), ("c", "hip_graph_replay")):
        rec["speedup_median_%s_vs_eager_torch" % key] = round(
            rec[key]["steps_per_s"]["median"] / rec["eager_torch"]["steps_per_s"]["median"], 3)
    lo, hi = rec["hip_graph_replay"]["steps_per_s"]["min"], rec["eager_torch"]["steps_per_s"]["max"]
    rec["graph_replay_faster_beyond_ranges"] = bool(lo > hi)

    if args.kernel_stats:
        phase("kernel stats")
        acts = [torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]
        with torch.profiler.profile(activities=acts) as prof:
            for _ in range(3):
                run["c"]()
            torch.cuda.synchronize()
        dev = lambda e: getattr(e, "self_device_time_total", getattr(e, "self_cuda_time_total", 0.0))  # noqa: E731
        kern = [e for e in prof.key_averages() if dev(e) > 0 and e.self_cpu_time_total == 0]
        other = [e for e in kern if any(m in e.key for m in NOT_OURS)]
        total, oth = sum(dev(e) for e in kern), sum(dev(e) for e in other)
        rec["kernel_stats"] = {
            "source": "torch.profiler, 3 replays of the captured step", "launches_per_step": sum(e.count for e in kern) // 3,
            "device_us_per_step": round(total / 3, 1), "libmmt_hip_share": round(1 - oth / total, 4) if total else None,
            "aten_vendor_share": round(oth / total, 4) if total else None,
            "aten_vendor_launches_per_step": sum(e.count for e in other) // 3,
            "aten_vendor_top": [[e.key[:80], e.count // 3, round(dev(e) / 3, 1)]
                                for e in sorted(other, key=lambda e: -dev(e))[:6]]}
    signal.alarm(0)
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
