#!/usr/bin/env python3
"""Candidate elimination with the template K/V cache, timed on the MI355X in one process:

  * asym_ce at each batch size and 16-bit type: the hipGraph replay of the full forward against the replay of
    the cached search pass (the template pass runs once, outside the timing), and asym the same way for
    context;
  * the packed typed gather (mmt_ce_rows_gather_cast) at the stage-1 shape -- S = 16 sequences, 400 -> 280
    rows, C = 768, fp32 rows + the bf16 copy -- against mmt_ce_gather on the pitch-528 streams at that shape
    (which also copies the 128 template rows of every sequence).

The sides of a comparison alternate; each timing replays for at least --seconds after a warm-up and ends in
a device synchronise; --repeats timings per side give the median and the spread (min, max).

    python tools/ce_cache_time.py --out profiles/ce_cache_time.jsonl

--full-ab PKG: instead, the asym_ce full forward (bf16, B = 1 and 8, graph replay) of another build of the package
(PKG = the `multi-modal-tracking_amd` directory of the parent commit's tree, built) against this tree's, each
timing in a fresh child process, three rounds in alternating order; a third side runs PKG's Python on this
tree's library.  The rate of one process differs from the next by more than a process's own spread, so the sides
are compared over the processes' range."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def full_forward_child(pkg):
    """One process of --full-ab: frames/s of the asym_ce full-forward graph replay from the package at pkg."""
    sys.path.insert(0, pkg)
    import torch
    from mmt_amd import synthetic
    from mmt_amd.runtime import MixFormerRGBTRuntime
    keys = json.load(open(os.path.join(ROOT, "tests", "golden", "state_dict_asym_ce.json")))
    sd = {k: torch.from_numpy(v) for k, v in synthetic.synth_state_dict(keys).items()}
    rt = MixFormerRGBTRuntime(sd, "asym_ce", dtype=torch.bfloat16)
    res = {}
    for B in (1, 8):
        t, o, s = [[x.cuda() for x in grp] for grp in synthetic.synth_inputs(B)]
        ws = rt.workspace(B)
        rt.load_inputs(ws, t, o, s)
        g = rt.capture(B)
        for _ in range(20):
            g.replay()
        torch.cuda.synchronize()
        rates = []
        for _ in range(5):
            n, t0 = 0, time.perf_counter()
            while True:
                for _ in range(20):
                    g.replay()
                torch.cuda.synchronize()
                n += 20
                dt = time.perf_counter() - t0
                if dt >= 1.0:
                    break
            rates.append(B * n / dt)
        res[B] = {"median": round(statistics.median(rates), 1), "min": round(min(rates), 1), "max": round(max(rates), 1),
                  "box": ws["BOX"].cpu().tolist()[0]}
    print("RESULT " + json.dumps(res))


def full_forward_ab(pkg, emit):
    import subprocess
    this = os.path.join(ROOT, "multi-modal-tracking_amd")
    newlib = os.path.join(this, "mmt_amd", "_lib", "libmmt_hip.so")
    order = [("parent", pkg, None), ("parent_python_this_library", pkg, newlib), ("this", this, None)]
    for rnd in range(3):
        for name, path, lib in (order if rnd % 2 == 0 else order[::-1]):
            env = dict(os.environ)
            env.pop("MMT_HIP_LIB", None)
            if lib:
                env["MMT_HIP_LIB"] = lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--full-forward-child", path], env=env,
                               capture_output=True, text=True, timeout=240)
            if p.returncode != 0:
                print(p.stdout[-2000:], p.stderr[-4000:])
                sys.exit(1)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]
            emit({"what": "asym_ce_full_forward_ab", "side": name, "round": rnd, "dtype": "bf16", "unit": "frames/s",
                  "rates": json.loads(line)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--full-ab", default="", help="the parent build's multi-modal-tracking_amd directory")
    ap.add_argument("--full-forward-child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ce_cache_time.jsonl"))
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--dtypes", default="bf16,fp16")
    ap.add_argument("--variants", default="asym_ce,asym")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if args.full_forward_child:
        return full_forward_child(args.full_forward_child)
    if args.full_ab:
        out = open(args.out, "a")

        def emit_ab(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
        return full_forward_ab(os.path.abspath(args.full_ab), emit_ab)
    sys.path.insert(0, os.path.join(ROOT, "multi-modal-tracking_amd"))
    import torch
    from mmt_amd import synthetic
    from mmt_amd._lib import LIB, MMT_BF16, check
    from mmt_amd.runtime import MixFormerRGBTRuntime

    assert torch.cuda.is_available(), "needs the MI355X"
    out = open(args.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

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

    def compare(sides, seconds, repeats):
        """{name: [rate per repeat]}, the sides alternating."""
        rates = {k: [] for k in sides}
        for _ in range(repeats):
            for k, fn in sides.items():
                rates[k].append(timed(fn, seconds))
        return rates

    def summary(r, scale=1.0, nd=1):
        return {"median": round(statistics.median(r) * scale, nd), "min": round(min(r) * scale, nd),
                "max": round(max(r) * scale, nd)}

    golden = os.path.join(ROOT, "tests", "golden")
    dts = {"bf16": torch.bfloat16, "fp16": torch.float16}
    for variant in args.variants.split(","):
        keys = json.load(open(os.path.join(golden, "state_dict_%s.json" % variant)))
        sd = {k: torch.from_numpy(v) for k, v in synthetic.synth_state_dict(keys).items()}
        for dname in args.dtypes.split(","):
            rt = MixFormerRGBTRuntime(sd, variant, dtype=dts[dname])
            for B in [int(b) for b in args.batches.split(",")]:
                t, o, s = [[x.cuda() for x in grp] for grp in synthetic.synth_inputs(B)]
                ws = rt.cache_workspace(B)
                rt.load_inputs(ws, t, o, s)
                rt.run_plan(ws["plan_t"])
                g_full = rt.capture_plan(ws["plan"])
                g_search = rt.capture_plan(ws["plan_s"])
                g_full.replay()
                box_full = ws["BOX"].clone()
                g_search.replay()
                torch.cuda.synchronize()
                diff = (ws["BOX"] - box_full).abs().max().item()
                r = compare({"full": g_full.replay, "search": g_search.replay}, args.seconds, args.repeats)
                emit({"what": "graph_replay", "variant": variant, "dtype": dname, "B": B, "unit": "frames/s",
                      "full": summary(r["full"], B), "search_cached": summary(r["search"], B),
                      "search_over_full": round(statistics.median(r["search"]) / statistics.median(r["full"]), 3),
                      "box_diff_cached_vs_full": diff, "launches": {"full": len(ws["plan"]), "search": len(ws["plan_s"])},
                      "seconds": args.seconds, "repeats": args.repeats})
            del rt
    # the gather at the stage-1 shape
    S, n_t, k, keep, C = 16, 128, 400, 280, 768
    pitch = n_t + k
    g = torch.Generator().manual_seed(3)
    order = torch.stack([torch.randperm(k, generator=g)[:k] for _ in range(S)]).int().cuda()  # [S][ns_full]
    x_p = torch.randn(S, pitch, C, generator=g).cuda()
    xc_p, xn_p = torch.empty_like(x_p), torch.empty(S, pitch, C, dtype=torch.bfloat16, device="cuda")
    x_c = x_p[:, n_t:].contiguous()
    xc_c = torch.empty(S, keep, C, device="cuda")
    xn_c = torch.empty(S, keep, C, dtype=torch.bfloat16, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    old = lambda: check(LIB.mmt_ce_gather(x_p.data_ptr(), xc_p.data_ptr(), xn_p.data_ptr(), order.data_ptr(), S, pitch,  # noqa: E731
                                          n_t, keep, k, C, MMT_BF16, st), "ce_gather")
    new = lambda: check(LIB.mmt_ce_rows_gather_cast(x_c.data_ptr(), k, xc_c.data_ptr(), xn_c.data_ptr(), keep,  # noqa: E731
                                                    order.data_ptr(), k, S, C, MMT_BF16, st), "rows_gather_cast")
    graphs = {"ce_gather": old, "rows_gather_cast": new}

    def device_us(fn, n=200):  # device time per launch from events around n back-to-back launches

        for _ in range(20):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n
    us = {"ce_gather": [], "rows_gather_cast": []}
    for _ in range(max(args.repeats, 5)):
        for name, fn in graphs.items():
            us[name].append(device_us(fn))
    assert torch.equal(xc_c, xc_p[:, n_t:n_t + keep]) and torch.equal(xn_c, xn_p[:, n_t:n_t + keep])
    moved_new = S * keep * C * (4 + 4 + 2)
    moved_old = S * (n_t + keep) * C * (4 + 4 + 2)
    emit({"what": "gather_stage1", "S": S, "rows": [k, keep], "C": C, "unit": "us per launch, back-to-back launches "
          "between two device events (includes the launch gaps)",
          "ce_gather_pitch528_with_template_rows": summary(us["ce_gather"], 1.0, 2),
          "rows_gather_cast_packed": summary(us["rows_gather_cast"], 1.0, 2),
          "bytes_moved": {"ce_gather": moved_old, "rows_gather_cast": moved_new}, "outputs_equal": True})


if __name__ == "__main__":
    main()
