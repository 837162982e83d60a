"""Child process of tests/test_gpu_syncbn_rccl.py: the corner head with SyncBatchNorm in train mode over a REAL RCCL
process group (backend "nccl", one rank on cuda:0), its cross-rank batch norm forced on (SYNC_BN_COLLECTIVE =
"always") against the local HIP batch norm ("auto" at one rank).

Run as its own process (MASTER_ADDR / MASTER_PORT from the parent).  Writes a JSON record to argv[1] and exits 0 when
every check holds:
  (a) eager: outputs, the input gradient, every parameter gradient, every running statistic and num_batches_tracked
      bitwise equal between the two; "always" issues one all_gather_into_tensor per SyncBatchNorm in the forward and as
      many all_reduce in the backward, "auto" none;
  (b) the "always" forward + backward captured as one hipGraph (the RCCL collectives recorded into it) and replayed on
      two inputs: outputs and gradients bitwise equal to the eager "always" results on the same inputs and state.
"""
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "multi-modal-tracking_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

B = 2


def main(out_path):
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    import mmt_amd.model as M
    import mmt_amd.train as T
    from mmt_amd.train import HipOps, head_forward

    counts = {"gather": 0, "reduce": 0}
    real_gather, real_reduce = dist.all_gather_into_tensor, dist.all_reduce

    def gather(*a, **k):
        counts["gather"] += 1
        return real_gather(*a, **k)

    def reduce(*a, **k):
        counts["reduce"] += 1
        return real_reduce(*a, **k)
    dist.all_gather_into_tensor, dist.all_reduce = gather, reduce

    torch.manual_seed(4)
    hd = M.Pyramid_Corner_Predictor(inplanes=64, channel=64, feat_sz=20, stride=16)
    hd = torch.nn.SyncBatchNorm.convert_sync_batchnorm(hd).cuda().train()
    n_sync = sum(type(m) is torch.nn.SyncBatchNorm for m in hd.modules())
    xs = [torch.randn(B, 64, 20, 20, device="cuda").bfloat16().float() for _ in range(2)]
    wgt = torch.linspace(0.5, 1.5, B * 4, device="cuda").view(B, 4)
    rec = {"backend": dist.get_backend(), "world": dist.get_world_size(), "sync_bn_modules": n_sync}

    def run(h, x):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = head_forward(h, x, HipOps).float()
        (out * wgt).sum().backward()
        return out

    def eager(h, knob, x):
        """One forward + backward from cleared gradients -> (out, dx, {parameter gradients}, {buffers}, counts)."""
        T.SYNC_BN_COLLECTIVE = knob
        counts["gather"] = counts["reduce"] = 0
        h.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        out = run(h, xi).detach().clone()
        torch.cuda.synchronize()
        T.SYNC_BN_COLLECTIVE = "auto"
        return (out, xi.grad.clone(), {k: p.grad.clone() for k, p in h.named_parameters()},
                {k: b.clone() for k, b in h.named_buffers()}, dict(counts))

    def differing(a, b):
        names = []
        for tag, u, v in (("out", a[0], b[0]), ("dx", a[1], b[1])):
            if not torch.equal(u, v):
                names.append(tag)
        for tag, u, v in (("grad ", a[2], b[2]), ("buffer ", a[3], b[3])):
            assert set(u) == set(v)
            names += [tag + k for k in u if not torch.equal(u[k], v[k])]
        return names

    # (a) eager: forced collectives against the local path, two steps each (the second from updated statistics)
    h_auto, h_always, h_graph = copy.deepcopy(hd), copy.deepcopy(hd), copy.deepcopy(hd)
    always = []
    for i, x in enumerate(xs):
        ra, rb = eager(h_auto, "auto", x), eager(h_always, "always", x)
        always.append(rb)
        neq = differing(ra, rb)
        rec["eager%d" % i] = {"not_bitwise": neq[:8], "auto": ra[4], "always": rb[4],
                              "tracked": int(rb[3]["conv1_tl.1.num_batches_tracked"])}
        print(json.dumps(rec), flush=True)
        assert not neq, neq[:8]
        assert ra[4] == {"gather": 0, "reduce": 0}, ra[4]
        assert rb[4] == {"gather": n_sync, "reduce": n_sync}, (rb[4], n_sync)
        assert rec["eager%d" % i]["tracked"] == i + 1

    # (b) captured: forward + backward under "always" as one hipGraph, replayed on the two inputs
    T.SYNC_BN_COLLECTIVE = "always"
    counts["gather"] = counts["reduce"] = 0
    h_graph.zero_grad(set_to_none=True)
    static_x = xs[0].clone().requires_grad_(True)
    graph = torch.cuda.CUDAGraph()
    mode = T.graph_capture_mode(True)
    with torch.cuda.graph(graph, capture_error_mode=mode):
        static_out = run(h_graph, static_x)
    T.SYNC_BN_COLLECTIVE = "auto"
    rec["captured_collectives"] = dict(counts)
    assert counts == {"gather": n_sync, "reduce": n_sync}, counts
    for i, x in enumerate(xs):
        with torch.no_grad():
            static_x.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        got = (static_out.detach(), static_x.grad, {k: p.grad for k, p in h_graph.named_parameters()},
               {k: b for k, b in h_graph.named_buffers()})
        neq = differing(always[i], got)
        rec["replay%d" % i] = {"not_bitwise": neq[:8]}
        print(json.dumps(rec), flush=True)
        assert not neq, neq[:8]
    rec["ok"] = True
    with open(out_path, "w") as f:
        json.dump(rec, f)
    del graph
    dist.destroy_process_group()


if __name__ == "__main__":
    try:
        main(sys.argv[1])
    except AssertionError as e:
        print("CHECK FAILED:", repr(e)[:2000], file=sys.stderr, flush=True)
        raise
