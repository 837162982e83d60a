#!/usr/bin/env python3
"""Digest of the training forward + backward, to compare two checkouts bit for bit: for one variant and one ops
choice, seed torch, build the net, run two consecutive TrainStep.backward calls (train() mode, DropPath 0.1, the
fusion dropouts as built, BatchNorms on running statistics) and append one JSON line with the loss, pred_boxes and a
SHA-256 over the raw bytes of every parameter gradient after each call.  A line holds each call's gradient digests
folded into one ("grads_sha": the SHA-256 over every (name, gradient SHA-256) in named_parameters order, equal exactly
when every one is), which keeps a committed record to a few hundred bytes; --per-param writes them all out under
"grads" (name -> digest) to find which gradient differs.

    python tools/train_forward_digest.py --ops torch --variant rgbt --template 32 --search 64 --out a.jsonl
    python tools/train_forward_digest.py --ops hip --variant asym_ce --ce-keep-rate 0.7 --ce-mask --out a.jsonl
    python tools/train_forward_digest.py --ops hip --variant rgbt --no-pair --pkg <other checkout>/multi-modal-tracking_amd ...

ops: hip (HipOps, the MI355X), torch / torchpair (the fp32 stand-ins of tests/test_train.py, CPU).  --pkg takes
another checkout's package with this same script; the lines name no checkout, so two files from the same sequence of
invocations are equal byte for byte exactly when every digest is."""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--ops", choices=("hip", "torch", "torchpair"), required=True)
    ap.add_argument("--variant", required=True)
    ap.add_argument("--pkg", default=os.path.join(ROOT, "multi-modal-tracking_amd"))
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--template", type=int, default=128)
    ap.add_argument("--search", type=int, default=320)
    ap.add_argument("--no-pair", action="store_true", help="train.PAIR = False")
    ap.add_argument("--no-token-rows", action="store_true", help="train.TOKEN_ROWS = False")
    ap.add_argument("--ce-keep-rate", type=float, default=None)
    ap.add_argument("--ce-mask", action="store_true", help="asym_ce: the CTR_POINT template mask")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--per-param", action="store_true", help="also write every gradient's own digest")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(args.pkg)), "tests"))
    sys.path.insert(0, args.pkg)
    import mmt_amd.model as M
    import mmt_amd.train as T

    if args.ops == "hip":
        assert torch.cuda.is_available(), "needs the MI355X"
        ops, dev = T.HipOps, "cuda"
    else:
        import test_train
        torch.set_num_threads(8)
        ops, dev = (test_train.TorchOps if args.ops == "torch" else test_train.TorchPairOps), "cpu"
    T.PAIR, T.TOKEN_ROWS = not args.no_pair, not args.no_token_rows

    torch.manual_seed(args.seed)
    net = M.BUILDERS[args.variant](M.hot_path_cfg(search=args.search, template=args.template), train=False)
    with torch.no_grad():  # non-trivial corner heatmaps (the default init is near-flat)
        for br in ("tl", "br"):
            getattr(net.box_head, "conv5_" + br).weight.mul_(30.0)
    net = net.to(dev).train()
    net.drop_path_rate = 0.1
    for m in net.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.eval()
    kw = {}
    if args.ce_keep_rate is not None:
        kw["ce_keep_rate"] = args.ce_keep_rate
    if args.ce_mask:
        kw["ce_template_mask"] = T.ce_center_mask(args.batch, args.template // 16, dev)
    step = T.TrainStep(net, ops, **kw)
    rec = {"ops": args.ops, "variant": args.variant, "batch": args.batch, "template": args.template,
           "search": args.search, "pair": T.PAIR, "token_rows": T.TOKEN_ROWS, "ce_keep_rate": args.ce_keep_rate,
           "ce_mask": args.ce_mask, "seed": args.seed, "calls": []}
    for call in range(2):
        t, o, s, gt = T.synthetic_batch(args.batch, dev, torch.Generator().manual_seed(3 + call), args.template,
                                        args.search)
        seen = []
        hook = step.model.register_forward_hook(lambda m, i, out: seen.append(out.detach()))
        stats = step.backward(t, o, s, gt)
        hook.remove()
        if dev == "cuda":
            torch.cuda.synchronize()
        grads = {n: _sha(p.grad) for n, p in net.named_parameters() if p.grad is not None}
        fold = hashlib.sha256("".join(n + " " + h + "\n" for n, h in grads.items()).encode()).hexdigest()
        rec["calls"].append({"loss": float(stats["loss"]), "loss_sha": _sha(stats["loss"]),
                             "pred_boxes": seen[0].float().cpu().view(-1, 4).tolist(), "pred_boxes_sha": _sha(seen[0]),
                             "n_grads": len(grads), "grads_sha": fold, **({"grads": grads} if args.per_param else {})})
    line = json.dumps(rec, sort_keys=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    print(json.dumps({k: v for k, v in rec.items() if k != "calls"}), "loss", [c["loss"] for c in rec["calls"]],
          "grads", [c["n_grads"] for c in rec["calls"]], flush=True)


if __name__ == "__main__":
    main()
