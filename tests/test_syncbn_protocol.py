"""The cross-rank batch norm's exchange protocol (mmt_amd.train.sync_batchnorm_relu: moments all-gathered and folded
in rank order, backward sums all-reduced) over a gloo group on the CPU, with the fp64 torch phases of
tests/syncbn_ref.py in place of the HIP kernels, against nn.BatchNorm2d in fp64 on the concatenated batch."""
import os
import socket

import pytest
import torch

from syncbn_ref import RefPhases, full_batch_reference

H, C, MOM, EPS = 5, 3, 0.1, 1e-5
TOL = 1e-9  # both sides fp64, differing in summation order only


def _data(batches):
    """Per-rank maps with mean 4r - 3 and std 1 + r (the between-rank term dominates the variance), and the
    module's parameters and running statistics."""
    g = torch.Generator().manual_seed(17 + len(batches))
    xs = [torch.randn(b, H, H, C, generator=g, dtype=torch.float64) * (1 + r) + (4 * r - 3) for r, b in enumerate(batches)]
    dys = [torch.randn(b, H, H, C, generator=g, dtype=torch.float64) for b in batches]
    par = {"weight": torch.rand(C, generator=g, dtype=torch.float64) + 0.5,
           "bias": torch.randn(C, generator=g, dtype=torch.float64) * 0.3,
           "running_mean": torch.randn(C, generator=g, dtype=torch.float64) * 0.1,
           "running_var": torch.rand(C, generator=g, dtype=torch.float64) + 0.5}
    return xs, dys, par


def _worker(rank, world, port, batches, out_dir):
    import torch.distributed as dist
    import mmt_amd.train as T
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        xs, dys, par = _data(batches)
        x = xs[rank].clone().requires_grad_(True)
        w, b = par["weight"].clone().requires_grad_(True), par["bias"].clone().requires_grad_(True)
        rm, rv = par["running_mean"].clone(), par["running_var"].clone()
        y = T.sync_batchnorm_relu(x, w, b, rm, rv, MOM, EPS, C, None, RefPhases)
        y.backward(dys[rank])
        rec = {"y": y.detach(), "dx": x.grad, "dgamma": w.grad, "dbeta": b.grad, "running_mean": rm, "running_var": rv}
        # the dispatch: a training SyncBatchNorm in a group of more than one rank is the HIP path's, unless "off"
        bn = torch.nn.SyncBatchNorm(8).train()
        old = T.SYNC_BN_COLLECTIVE
        try:
            for knob in ("auto", "off", "always"):
                T.SYNC_BN_COLLECTIVE = knob
                rec["ok_" + knob] = T._hip_bn_ok(bn)
        finally:
            T.SYNC_BN_COLLECTIVE = old
        rec["ok_eval_off"] = T._hip_bn_ok(torch.nn.SyncBatchNorm(8).eval())
        rec["ok_cumulative"] = T._hip_bn_ok(torch.nn.SyncBatchNorm(8, momentum=None).train())
        torch.save(rec, os.path.join(out_dir, "rank%d.pt" % rank))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("batches", [(1, 1), (1, 2, 1)])
def test_sync_batchnorm_protocol_matches_full_batch(batches, tmp_path):
    import torch.multiprocessing as mp
    W = len(batches)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mp.spawn(_worker, args=(W, port, batches, str(tmp_path)), nprocs=W, join=True)
    recs = [torch.load(os.path.join(str(tmp_path), "rank%d.pt" % r)) for r in range(W)]
    xs, dys, par = _data(batches)
    ref = full_batch_reference(torch.cat(xs), torch.cat(dys), par["weight"], par["bias"], par["running_mean"],
                               par["running_var"], MOM, EPS)
    rel = lambda a, r: ((a - r).norm() / r.norm().clamp_min(1e-300)).item()  # noqa: E731
    r0 = 0
    for r, b in enumerate(batches):
        sl = slice(r0, r0 + b)
        r0 += b
        ey, edx = rel(recs[r]["y"], ref["y"][sl]), rel(recs[r]["dx"], ref["dx"][sl])
        print("W %d rank %d: y %.3g dx %.3g" % (W, r, ey, edx))
        assert ey <= TOL and edx <= TOL, (r, ey, edx)
        # every rank folds the same gathered triples in the same order: the same bits
        assert torch.equal(recs[r]["running_mean"], recs[0]["running_mean"])
        assert torch.equal(recs[r]["running_var"], recs[0]["running_var"])
    # dgamma / dbeta stay local sums (DDP averages them): their sum over the ranks is the full batch's
    eg = rel(sum(q["dgamma"] for q in recs), ref["dgamma"])
    eb = rel(sum(q["dbeta"] for q in recs), ref["dbeta"])
    em, ev = rel(recs[0]["running_mean"], ref["running_mean"]), rel(recs[0]["running_var"], ref["running_var"])
    print("W %d: dgamma %.3g dbeta %.3g running mean %.3g var %.3g" % (W, eg, eb, em, ev))
    assert eg <= TOL and eb <= TOL and em <= TOL and ev <= TOL
    # the statistics really are the group's: rank 0's own batch gives a different running mean by far
    own = (1 - MOM) * par["running_mean"] + MOM * xs[0].reshape(-1, C).mean(0)
    assert rel(own, ref["running_mean"]) > 1e3 * TOL
    if W == 2:
        for q in recs:
            assert q["ok_auto"] is True and q["ok_always"] is True and q["ok_off"] is False
            assert q["ok_eval_off"] is True and q["ok_cumulative"] is False


def _tracked_worker(rank, world, port, out_dir):
    """HipOps.bn_relu's dispatch and bookkeeping with the HIP phases swapped for the fp64 ones (no GPU here)."""
    import torch.distributed as dist
    import mmt_amd.train as T
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        xs, _, par = _data((1, 1))
        xs = [x.bfloat16().double() for x in xs]  # bn_relu takes bf16 maps
        bn = torch.nn.SyncBatchNorm(C, eps=EPS, momentum=MOM).double().train()
        with torch.no_grad():
            bn.weight.copy_(par["weight"])
            bn.bias.copy_(par["bias"])
        real = T.sync_batchnorm_relu
        calls = []

        def with_ref(x, w, b, rm, rv, mom, eps, c, group=None, phases=None):
            calls.append((mom, eps, c, group))
            return real(x.double(), w, b, rm, rv, mom, eps, c, group, RefPhases)
        T.sync_batchnorm_relu = with_ref
        try:
            y = T.HipOps.bn_relu(F_pad8(xs[rank]), bn)  # 8-channel rows in (a keep_pad conv): padded rows out
        finally:
            T.sync_batchnorm_relu = real
        torch.save({"tracked": int(bn.num_batches_tracked), "calls": len(calls), "args": calls[0][:3],
                    "shape": tuple(y.shape), "pad": float(y.detach()[..., C:].abs().max()),
                    "running_mean": bn.running_mean.clone()}, os.path.join(out_dir, "t%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def F_pad8(x):
    return torch.nn.functional.pad(x, (0, 8 - x.shape[-1]))


def test_bn_relu_takes_the_sync_path_and_tracks_once(tmp_path):
    import torch.multiprocessing as mp
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mp.spawn(_tracked_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    recs = [torch.load(os.path.join(str(tmp_path), "t%d.pt" % r)) for r in range(2)]
    xs, dys, par = _data((1, 1))
    xs = [x.bfloat16().double() for x in xs]
    ref = full_batch_reference(torch.cat(xs), torch.cat(dys), par["weight"], par["bias"], torch.zeros(C), torch.ones(C),
                               MOM, EPS)
    for q in recs:
        assert q["tracked"] == 1 == ref["tracked"] and q["calls"] == 1
        assert q["args"] == (MOM, EPS, C)
        assert q["shape"] == (1, H, H, 8) and q["pad"] == 0.0
        assert torch.equal(q["running_mean"], recs[0]["running_mean"])
        assert ((q["running_mean"] - ref["running_mean"]).norm() / ref["running_mean"].norm()).item() <= TOL
