#!/usr/bin/env python3
"""Batched multi-sequence tracker against N single trackers, per sequence-frame, in one process:

  (a) N RGBTTrackerCore (one sequence each, one hipGraph replay and one host round trip per
      sequence-frame) stepped one after another -- code the batched tracker does not touch;
  (b) one RGBTBatchTrackerCore of N slots (one replay and one round trip per N sequence-frames)

on the same resident 480x640 uint8 frame pairs, bf16, update interval 200, the states put back to
the initial boxes before every step (as bench.py's tracker_step does: synthetic weights, the box
wanders).  The two sides alternate; each timing runs at least --seconds; --repeats gives the spread.

    python tools/batch_tracker_time.py --out profiles/batch_tracker_time.jsonl
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o bt -- python tools/batch_tracker_time.py --trace-run 64
    python tools/batch_tracker_time.py --kernel-stats <dir>/.../bt_kernel_stats.csv --slots 64

--trace-run N: only a few steps of side (b) at N slots, for the kernel trace; --kernel-stats CSV: the
crop-table, slot-update and slot-copy kernels' device time from that trace's stats file, appended to --out.

--slot-cache: instead of (a) against (b), the batched tracker without (b) and with (c) the per-slot template
K/V cache (RGBTBatchTrackerCore(slot_cache=True, refresh_slots=--refresh-slots)), alternating in the same run
on the same frames; also the refresh replays per 1000 steps at the tool's update interval, the refresh graph's
time per replay, and the scatter launch of mmt_slot_copy alone between two device events with its achieved
bytes/s, read + written.  With --trace-run the cached side is traced, and --kernel-stats then also splits
mmt_slot_copy's launches by grid from the per-dispatch trace beside the stats file (the stats file sums the gather
and the scatter under one kernel name) and gives the scatter's bytes/s inside the refresh plan.

    python tools/batch_tracker_time.py --slot-cache --out profiles/batch_tracker_time.jsonl

--pack: the packed step (RGBTBatchTrackerCore(pack="auto")) on 64 slots with --active of them holding a sequence,
same protocol, three sides alternating: the packing core, the same core with pack off, and a core of slots = R (the
rung the packed step runs at) holding the same sequences.  The record carries the three rates, the step times, the
packed step's excess over the slots = R core, the run's own spread, and the device time of the launches the packed
step adds (packed crop, template gather, packed update: each alone between two device events), plus the bytes a rung
owns.  With --slot-cache all three cores use the per-slot cache.  --drain: track_sequences over 128 sequences of
long-tailed lengths (fixed seed, written into the record) on 64 slots, wall time and step_counts with pack="auto" and
with pack off (each side includes the capture of its graphs).

    python tools/batch_tracker_time.py --pack --drain --variants shared [--slot-cache]"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 480, 640
KERNELS = ("sample_target_table_kernel", "track_update_slots_kernel", "slot_copy_kernel")
INTERVAL = 200


def kernel_stats(path, slots, variant):
    rec = {"what": "kernel_trace", "slots": slots, "variant": variant, "source": "rocprofv3 --kernel-trace --stats"}
    for row in csv.DictReader(open(path)):
        name = row.get("Name") or row.get("KernelName") or ""
        for k in KERNELS:
            if k in name:
                rec[k] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2),
                          "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    # the stats file sums mmt_slot_copy's gather and scatter launches under one name: split them by grid in the
    # per-dispatch trace beside it (the scatter is the launch with the most segments, grid y)
    trace = path.replace("_kernel_stats.csv", "_kernel_trace.csv")
    if trace != path and os.path.exists(trace):
        by_grid = {}
        for row in csv.DictReader(open(trace)):
            if "slot_copy_kernel" in (row.get("Kernel_Name") or ""):
                grid = tuple(int(row["Grid_Size_" + a]) // max(1, int(row["Workgroup_Size_" + a])) for a in "XYZ")
                by_grid.setdefault(grid, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        rec["slot_copy_by_grid"] = {"x".join(map(str, g)): {"calls": len(t), "avg_us": round(sum(t) / len(t), 2),
                                                              "min_us": round(min(t), 2), "max_us": round(max(t), 2)}
                                    for g, t in sorted(by_grid.items())}
        if by_grid:
            g = max(by_grid, key=lambda k: k[1])  # ViT-B bf16: 24 segments of 128 rows x 3072 B per listed slot
            moved = 2 * g[2] * g[1] * 128 * 3072
            t = by_grid[g]
            rec["slot_copy_scatter"] = {"grid": list(g), "bytes_moved": moved, "avg_TBps": round(moved / (sum(t) / len(t)) / 1e6, 3),
                                        "best_TBps": round(moved / min(t) / 1e6, 3), "copy_ceiling_TBps": 6.3}
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
    ap.add_argument("--slot-cache", action="store_true")
    ap.add_argument("--refresh-slots", type=int, default=0, help="refresh capacity (0: the core's default)")
    ap.add_argument("--pack", action="store_true", help="the packed step: see the module docstring")
    ap.add_argument("--active", default="64,33,32,8,1", help="--pack: active slots of the 64 (empty: none)")
    ap.add_argument("--drain", action="store_true", help="--pack: also the 128-sequence drain")
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
        singles = [RGBTTrackerCore(net, 2.0, 128, 5.0, 320, [INTERVAL], multimodal=mm) for _ in range(N)]
        for b, c in enumerate(singles):
            c.initialize(frames[0], init_box(b))
        inits = [c.state.clone() for c in singles]
        batch = RGBTBatchTrackerCore(net, 2.0, 128, 5.0, 320, [INTERVAL], multimodal=mm, slots=N)
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

    def cache_sides(net, variant, N):
        """(b) the uncached batched tracker, (c) the same with the per-slot template K/V cache."""
        mm = builders[variant][1]
        cores = []
        for cached in (False, True):
            c = RGBTBatchTrackerCore(net, 2.0, 128, 5.0, 320, [INTERVAL], multimodal=mm, slots=N, slot_cache=cached,
                                     refresh_slots=(args.refresh_slots or None) if cached else None)
            for b in range(N):
                c.assign(b, frames[0], init_box(b))
            cores.append(c)
        binit = cores[0].state.clone()

        def stepper(c):
            def step(i):
                c.state.copy_(binit)
                r = c.track({b: frames[(i + b) % 4] for b in range(N)})
                assert len(r) == N and not any(isinstance(v, Exception) for v in r.values())
            return step
        return stepper(cores[0]), stepper(cores[1]), cores[0], cores[1]

    def refresh_times(core, N):
        """Host time per refresh replay (graph, synchronised) and device time of its scatter launch alone."""
        rt, sc = core._rt, core._sc
        D = sc["D"]
        slots = list(range(D))
        rt.refresh_template_slots(sc, slots)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            rt.refresh_template_slots(sc, slots)
        torch.cuda.synchronize()
        per_replay = (time.perf_counter() - t0) / 20
        fn, a, name, _ = sc["plan"][-1]
        assert name == "slot_scatter"
        st = torch.cuda.current_stream().cuda_stream
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for _ in range(3):
            fn(*a, st)
        ev[0].record()
        for _ in range(50):
            fn(*a, st)
        ev[1].record()
        torch.cuda.synchronize()
        us = ev[0].elapsed_time(ev[1]) * 1e3 / 50
        moved = 2 * D * sc["scatter_bytes_per_slot"]  # read + written, all D entries valid
        return {"refresh_slots": D, "refresh_replay_us": round(per_replay * 1e6, 1), "scatter_launch_us": round(us, 2),
                "scatter_bytes_moved": moved, "scatter_TBps": round(moved / us / 1e6, 3), "copy_ceiling_TBps": 6.3}

    def timed(step, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            step(i)
        return time.perf_counter() - t0  # every step ends in its host round trip

    if args.trace_run:
        variant = args.variants.split(",")[0]
        if args.slot_cache:
            _, step_c, _, core = cache_sides(network(variant), variant, args.trace_run)
            timed(step_c, 30)
            for _ in range(5):
                core._rt.refresh_template_slots(core._sc, list(range(core._sc["D"])))
            torch.cuda.synchronize()
            return
        _, step_b, _ = sides(network(variant), variant, args.trace_run)
        timed(step_b, 30)
        return

    def pack_sides(net, variant, N, A, cached):
        """(p) the packing core with A of N slots active, (o) the same core with pack off, (r) a core of
        slots = R -- the rung the packed step runs at, N when there is none -- holding the same A sequences."""
        from mmt_amd.tracking import choose_rung, pack_rungs
        mm = builders[variant][1]
        R = choose_rung(pack_rungs("auto", N), A) or N
        act = [i * N // A for i in range(A)]  # spread over the slots, ascending
        kw = dict(multimodal=mm, slot_cache=cached)
        cores = [RGBTBatchTrackerCore(net, 2.0, 128, 5.0, 320, [INTERVAL], slots=N, pack="auto",
                                      refresh_slots=(args.refresh_slots or None) if cached else None, **kw),
                 RGBTBatchTrackerCore(net, 2.0, 128, 5.0, 320, [INTERVAL], slots=N,
                                      refresh_slots=(args.refresh_slots or None) if cached else None, **kw),
                 RGBTBatchTrackerCore(net, 2.0, 128, 5.0, 320, [INTERVAL], slots=R,
                                      refresh_slots=(min(args.refresh_slots, R) or None) if cached else None, **kw)]
        where = [act, act, list(range(A))]
        steps = []
        for c, slots in zip(cores, where):
            for k, b in enumerate(slots):
                c.assign(b, frames[0], init_box(k))
            init = c.state.clone()

            def step(i, c=c, slots=slots, init=init):
                c.state.copy_(init)
                r = c.track({b: frames[(i + k) % 4] for k, b in enumerate(slots)})
                assert len(r) == A and not any(isinstance(v, Exception) for v in r.values())
            steps.append(step)
        return R, cores, steps

    def pack_launch_times(core, R):
        """Device time of the launches a packed step adds to the batch-R plan: the packed crop, the template gather
        and the packed update, each alone between two device events (50 launches after 3)."""
        pk = core._packs[R]
        st = torch.cuda.current_stream().cuda_stream
        saved = core.state.clone()
        out = {}
        for fn, a, name, _ in (pk["plan"][0], pk["plan"][1], pk["plan"][-1]):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            for _ in range(3):
                fn(*a, st)
            ev[0].record()
            for _ in range(50):
                fn(*a, st)
            ev[1].record()
            torch.cuda.synchronize()
            out[name + "_us"] = round(ev[0].elapsed_time(ev[1]) * 1e3 / 50, 2)
        core.state.copy_(saved)
        seen, total = set(), 0
        for v in list(pk.values()) + list(pk["ws"].values()):
            for t in (v if isinstance(v, (list, tuple)) else [v]):
                if isinstance(t, torch.Tensor) and t.data_ptr() not in seen:
                    seen.add(t.data_ptr())
                    total += t.numel() * t.element_size()
        out["rung_bytes"] = total
        return out

    def drain_lengths(n=128, seed=7):
        """Long-tailed sequence lengths (frames, the first one included) from a fixed seed."""
        import numpy as np
        rng = np.random.default_rng(seed)
        return [int(v) for v in np.clip(8 + 24 * rng.pareto(1.1, n), 8, 1000).astype(int)]

    if args.pack:
        from mmt_amd.tracking import track_sequences
        for variant in args.variants.split(","):
            net = network(variant)
            N = 64
            for A in [int(x) for x in args.active.split(",") if x]:
                R, cores, steps = pack_sides(net, variant, N, A, args.slot_cache)
                names = ("packed_core", "pack_off_core", "small_core")
                n = []
                for step in steps:
                    timed(step, 3)
                    n.append(max(5, int(args.seconds / (timed(step, 5) / 5)) + 1))
                rates = [[] for _ in steps]
                for _ in range(args.repeats):
                    for k, step in enumerate(steps):
                        rates[k].append(A * n[k] / timed(step, n[k]))
                rec = {"what": "tracker_step_packed", "variant": variant, "slots": N, "active": A, "batch": R,
                       "slot_cache": bool(args.slot_cache), "dtype": "bf16", "frame": [H, W], "steps": dict(zip(names, n)),
                       "update_interval": INTERVAL, "unit": "sequence-frames/s", "step_counts": {
                           k: {str(b): v for b, v in c.step_counts.items()} for k, c in zip(names, cores)}}
                for k, key in enumerate(names):
                    r = sorted(rates[k])
                    rec[key] = {"median": round(r[len(r) // 2], 1), "min": round(r[0], 1), "max": round(r[-1], 1)}
                ms = lambda key, q: 1e3 * A / rec[key][q]  # noqa: E731  step time in ms
                rec["step_ms"] = {key: round(ms(key, "median"), 4) for key in names}
                rec["packed_minus_small_ms"] = round(ms("packed_core", "median") - ms("small_core", "median"), 4)
                rec["spread_ms"] = round((ms("packed_core", "min") - ms("packed_core", "max"))
                                         + (ms("small_core", "min") - ms("small_core", "max")), 4)
                if R < N:
                    rec.update(pack_launch_times(cores[0], R))
                    rec["added_launches_ms"] = round((rec["track_sample_target_packed_us"] + rec["pack_gather_us"]
                                                      + rec["track_update_packed_us"]) / 1e3, 4)
                    rec["within_margin"] = rec["packed_minus_small_ms"] <= rec["spread_ms"] + rec["added_launches_ms"]
                else:  # full occupancy or no rung: the packing core and the pack-off core replay the same graph
                    rec["within_margin"] = abs(ms("packed_core", "median") - ms("pack_off_core", "median")) <= rec["spread_ms"]
                emit(rec)
                del cores, steps
                torch.cuda.empty_cache()
            if args.drain:
                lengths = drain_lengths()
                rec = {"what": "tracker_drain", "variant": variant, "slots": N, "slot_cache": bool(args.slot_cache),
                       "dtype": "bf16", "frame": [H, W], "update_interval": INTERVAL, "sequences": len(lengths),
                       "lengths_seed": 7, "lengths": lengths, "tracked_frames": sum(lengths) - len(lengths)}
                for key, pack in (("pack_auto", "auto"), ("pack_off", None)):
                    core = RGBTBatchTrackerCore(net, 2.0, 128, 5.0, 320, [INTERVAL], multimodal=builders[variant][1],
                                                slots=N, slot_cache=args.slot_cache, pack=pack,
                                                refresh_slots=(args.refresh_slots or None) if args.slot_cache else None)
                    seqs = [("q%d" % k, (frames[(k + i) % 4] for i in range(L)), init_box(k)) for k, L in enumerate(lengths)]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res = track_sequences(core, seqs)
                    wall = time.perf_counter() - t0
                    assert all(len(res["q%d" % k]) == L for k, L in enumerate(lengths))
                    rec[key] = {"wall_s": round(wall, 3), "step_counts": {str(b): v for b, v in sorted(core.step_counts.items())},
                                "sequence_frames_per_s": round(rec["tracked_frames"] / wall, 1)}
                    del core
                    torch.cuda.empty_cache()
                rec["speedup"] = round(rec["pack_off"]["wall_s"] / rec["pack_auto"]["wall_s"], 3)
                emit(rec)
        return

    if args.slot_cache:
        for variant in args.variants.split(","):
            net = network(variant)
            for N in [int(x) for x in args.slots.split(",")]:
                step_b, step_c, plain, cached = cache_sides(net, variant, N)
                n = {}
                for name, step in (("b", step_b), ("c", step_c)):
                    timed(step, 3)
                    n[name] = max(5, int(args.seconds / (timed(step, 5) / 5)) + 1)
                rates = {"b": [], "c": []}
                r0, f0 = cached.refresh_replays, cached.frame_id[0]
                for _ in range(args.repeats):
                    for name, step in (("b", step_b), ("c", step_c)):
                        rates[name].append(N * n[name] / timed(step, n[name]))
                steps_c = cached.frame_id[0] - f0
                rec = {"what": "tracker_step_slot_cache", "variant": variant, "slots": N, "dtype": "bf16", "frame": [H, W],
                       "steps": n, "update_interval": INTERVAL, "hip_graph": cached._graph is not None,
                       "unit": "sequence-frames/s",
                       "refresh_replays_per_1000_steps": round(1000.0 * (cached.refresh_replays - r0) / steps_c, 2)}
                for name, key in (("b", "batched_core"), ("c", "batched_core_slot_cache")):
                    r = sorted(rates[name])
                    rec[key] = {"median": round(r[len(r) // 2], 1), "min": round(r[0], 1), "max": round(r[-1], 1)}
                rec["speedup_median"] = round(rec["batched_core_slot_cache"]["median"] / rec["batched_core"]["median"], 3)
                rec.update(refresh_times(cached, N))
                emit(rec)
                del step_b, step_c, plain, cached
                torch.cuda.empty_cache()
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
