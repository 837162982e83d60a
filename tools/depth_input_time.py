#!/usr/bin/env python3
"""RGB-D input (aux_format="depth16"): what the device preparation of a raw depth frame costs.

  prepare   the prepare sequence alone (mmt_depth_prepare, five launches) between two device events, 50 calls after
            3 warm-ups, at 360x640 and 480x640, as one entry and as a 64-entry table (mmt_depth_prepare_table)
  step      the single tracker's and the 64-slot batched tracker's step with "depth16" (a resident raw depth frame
            per slot, prepared inside the step graph) against the same core fed resident prepared uint8 frames --
            the path every tracker had before; the sides alternate in one process, median and range of 3
  host      mmt_amd.depth.depth_to_3xd (numpy) in ms per frame on this job's CPUs
  rgb8      only the "rgb8" steps, from the package under --pkg (default: this tree).  Run alternately on this tree
            and on a build of the parent commit, it shows that the default path did not move.

    python tools/depth_input_time.py --out profiles/depth_input_time.jsonl
    python tools/depth_input_time.py --what rgb8 --pkg <tree of the parent commit, built> --tag parent"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(360, 640), (480, 640)]
INTERVAL = 200


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_input_time.jsonl"))
    ap.add_argument("--what", default="prepare,step,host")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "multi-modal-tracking_amd"))
    ap.add_argument("--tag", default="this")
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=1.5)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    what = args.what.split(",")
    out = open(args.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    sys.path.insert(0, args.pkg)
    import numpy as np
    import torch
    from mmt_amd import model as M
    from mmt_amd import synthetic
    from mmt_amd.tracking import RGBTBatchTrackerCore, RGBTTrackerCore

    def depth_frame(H, W, seed):  # a gamma-distributed range with 10 % holes, as depth frames look
        rng = np.random.default_rng(seed)
        d = np.minimum(rng.gamma(2.0, 900.0, (H, W)), 65535).astype(np.uint16)
        d[rng.random((H, W)) < 0.1] = 0
        return d

    if "host" in what:
        from mmt_amd.depth import depth_to_3xd
        for H, W in SIZES:
            frames = [depth_frame(H, W, s) for s in range(4)]
            depth_to_3xd(frames[0])
            t = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                for i in range(20):
                    depth_to_3xd(frames[i % 4])
                t.append((time.perf_counter() - t0) / 20 * 1e3)
            t.sort()
            emit({"what": "host_depth_to_3xd", "frame": [H, W], "unit": "ms/frame", "median": round(t[len(t) // 2], 3),
                  "min": round(t[0], 3), "max": round(t[-1], 3), "cpus": len(os.sched_getaffinity(0)),
                  "threads": torch.get_num_threads()})
    if what == ["host"]:
        return

    assert torch.cuda.is_available(), "needs the MI355X"
    st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731

    def events(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for _ in range(3):
            fn()
        ev[0].record()
        for _ in range(50):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3 / 50

    if "prepare" in what:
        from mmt_amd._lib import DEPTH_WORK_BYTES, LIB, DepthParams, check
        from mmt_amd.depth import depth_params
        for H, W in SIZES:
            for n in (1, args.slots):
                d = [torch.from_numpy(depth_frame(H, W, s).view(np.int16)).cuda() for s in range(n)]
                o = [torch.empty(H, W, 3, dtype=torch.uint8, device="cuda") for _ in range(n)]
                w = torch.empty(n, DEPTH_WORK_BYTES, dtype=torch.uint8, device="cuda")
                arr = (DepthParams * n)(*[depth_params(d[i], o[i], w[i]) for i in range(n)])
                if n == 1:
                    us = events(lambda: check(LIB.mmt_depth_prepare(arr, 1, st()), "mmt_depth_prepare"))
                else:
                    tab = torch.frombuffer(arr, dtype=torch.uint8).cuda()
                    us = events(lambda: check(LIB.mmt_depth_prepare_table(tab.data_ptr(), None, n, st()),
                                              "mmt_depth_prepare_table"))
                moved = n * H * W * (3 * 2 + 3)  # three reads of the 2-byte frame, one 3-byte write per pixel
                emit({"what": "depth_prepare", "frame": [H, W], "entries": n, "form": "host" if n == 1 else "table",
                      "launches": 5, "us_per_call": round(us, 2), "us_per_frame": round(us / n, 2),
                      "bytes_moved": moved, "TBps": round(moved / us / 1e6, 3)})

    if "step" not in what and "rgb8" not in what:
        return
    has_depth = "rgb8" not in what
    H, W = 480, 640
    net = M.build_mixformer_vit_rgbt_shared(M.hot_path_cfg(), train=False)
    keys = [(k, list(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.synth_state_dict(keys).items()}, strict=True)
    net = net.cuda().eval()
    raw = [depth_frame(H, W, 10 + s) for s in range(4)]
    g = torch.Generator().manual_seed(5)
    rgb = [torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).cuda() for _ in range(4)]
    if has_depth:
        from mmt_amd.depth import depth_to_3xd
        prepared = [torch.from_numpy(depth_to_3xd(d)).cuda() for d in raw]
    else:  # a parent build has no mmt_amd.depth: any resident uint8 frame serves the rgb8 step
        prepared = [torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).cuda() for _ in range(4)]
    raw_dev = [torch.from_numpy(d.view(np.int16)).cuda() for d in raw]

    def init_box(b):
        return [W * 0.2 + 5.0 * (b % 32), H * 0.25 + 3.0 * (b % 24), 64.0, 48.0]

    def timed(step, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            step(i)
        return time.perf_counter() - t0  # every step ends in its host round trip

    def single(aux):
        kw = {"aux_format": aux} if has_depth else {}
        c = RGBTTrackerCore(net, 2.0, 128, 5.0, 320, [INTERVAL], multimodal=True, **kw)
        second = raw_dev if aux == "depth16" else prepared
        c.initialize([rgb[0], second[0]], init_box(0))
        init = c.state.clone()

        def step(i):
            c.state.copy_(init)
            c.track([rgb[i % 4], second[i % 4]])
        return step

    def batched(aux, N):
        kw = {"aux_format": aux} if has_depth else {}
        c = RGBTBatchTrackerCore(net, 2.0, 128, 5.0, 320, [INTERVAL], multimodal=True, slots=N, **kw)
        second = raw_dev if aux == "depth16" else prepared
        for b in range(N):
            c.assign(b, [rgb[0], second[0]], init_box(b))
        init = c.state.clone()

        def step(i):
            c.state.copy_(init)
            r = c.track({b: [rgb[(i + b) % 4], second[(i + b) % 4]] for b in range(N)})
            assert len(r) == N and not any(isinstance(v, Exception) for v in r.values())
        return step

    for name, N, make in (("single", 1, lambda aux: single(aux)), ("batched", args.slots, lambda aux: batched(aux, args.slots))):
        auxes = ["rgb8", "depth16"] if has_depth else ["rgb8"]
        steps = {aux: make(aux) for aux in auxes}
        n = {}
        for aux, step in steps.items():  # warm-up (captures the graphs), then size the runs
            timed(step, 3)
            n[aux] = max(5, int(args.seconds / (timed(step, 5) / 5)) + 1)
        ms = {aux: [] for aux in auxes}
        for _ in range(args.repeats):
            for aux, step in steps.items():
                ms[aux].append(timed(step, n[aux]) / n[aux] * 1e3)
        rec = {"what": "tracker_step_aux_format", "core": name, "slots": N, "frame": [H, W], "dtype": "bf16",
               "tag": args.tag, "unit": "ms/step", "steps": n,
               "note": "both sides feed device-resident frames: no upload on either side"}
        for aux in auxes:
            t = sorted(ms[aux])
            rec[aux] = {"median": round(t[len(t) // 2], 4), "min": round(t[0], 4), "max": round(t[-1], 4)}
        if has_depth:
            rec["depth16_minus_rgb8_ms"] = round(rec["depth16"]["median"] - rec["rgb8"]["median"], 4)
        emit(rec)
        del steps
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
