"""Candidate elimination in training on the MI355X: the two new kernels behind mmt::ce_rows_gather /
mmt::ce_index_invert (copies: bitwise), the mmt::ce_select op (scores + sorted top-k) in fp32 and bf16, the
asymmetric_shared_ce module's train()-mode gradients on the HIP ops at the bench geometry (whose CE stages are
the ragged 408 / 324 / 266-row sequences), and its capture as a hipGraph (module forward + backward, then the
whole TrainStep)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

N_T = 8


def _prune_idx(S, n_t, lens, keep, g):
    """[0..n_t-1, n_t + a random order of `keep` of the `lens` search rows] per sequence (int32)."""
    head = torch.arange(n_t, dtype=torch.int32).repeat(S, 1)
    order = torch.stack([torch.randperm(lens, generator=g)[:keep] for _ in range(S)]).int()
    return torch.cat([head, order + n_t], 1)


@pytest.mark.parametrize("C", [768, 1024])
def test_rows_gather_forward_backward_bitwise(C):
    """(g) S = 4, n_t = 8, 25 search rows pruned to 18 and then 13 (odd row counts, no multiple of 4), then an
    index vector with -1 entries and one out-of-range entry: bitwise torch.index_select / zero rows; the backward
    bitwise index_add on the distinct indices."""
    import mmt_amd.ops  # noqa: F401
    g = torch.Generator().manual_seed(C)
    S = 4
    x0 = torch.randn(S, N_T + 25, C, generator=g)
    idx1 = _prune_idx(S, N_T, 25, 18, g)
    idx2 = _prune_idx(S, N_T, 18, 13, g)
    idx3 = torch.stack([torch.randperm(N_T + 13, generator=g) for _ in range(S)]).int()  # a recover-like vector
    idx3 = torch.cat([idx3, torch.full((S, 6), -1, dtype=torch.int32)], 1)[:, torch.randperm(N_T + 19, generator=g)]
    idx3[1, 2] = N_T + 13  # one past the last source row
    idx3[2, 5] = 1 << 30
    idx3[3, 0] = -(1 << 31)

    def ref_gather(x, idx):
        out = []
        for s in range(x.shape[0]):
            ok = (idx[s] >= 0) & (idx[s] < x.shape[1])
            y = torch.index_select(x[s], 0, idx[s].clamp(0, x.shape[1] - 1).long())
            out.append(torch.where(ok[:, None], y, torch.zeros(())))
        return torch.stack(out)

    xg = x0.cuda().requires_grad_(True)
    y1 = torch.ops.mmt.ce_rows_gather(xg, idx1.cuda())
    y2 = torch.ops.mmt.ce_rows_gather(y1, idx2.cuda())
    y3 = torch.ops.mmt.ce_rows_gather(y2, idx3.cuda())
    r1 = ref_gather(x0, idx1)
    r2 = ref_gather(r1, idx2)
    r3 = ref_gather(r2, idx3)
    for got, ref in ((y1, r1), (y2, r2), (y3, r3)):
        assert got.shape == ref.shape and torch.equal(got.detach().cpu(), ref)
    dy = torch.randn(r3.shape, generator=g)
    y3.backward(dy.cuda())

    def ref_scatter(d, idx, rows):  # index_add over the valid (distinct) indices
        out = []
        for s in range(d.shape[0]):
            ok = (idx[s] >= 0) & (idx[s] < rows)
            out.append(torch.zeros(rows, d.shape[2]).index_add_(0, idx[s][ok].long(), d[s][ok]))
        return torch.stack(out)

    d2 = ref_scatter(dy, idx3, N_T + 13)
    d1 = ref_scatter(d2, idx2, N_T + 18)
    d0 = ref_scatter(d1, idx1, N_T + 25)
    assert torch.equal(xg.grad.cpu(), d0)


def test_rows_gather_opcheck():
    import mmt_amd.ops  # noqa: F401
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4, N_T + 25, 768, generator=g).cuda().requires_grad_(True)
    idx = _prune_idx(4, N_T, 25, 18, g).cuda()
    torch.library.opcheck(torch.ops.mmt.ce_rows_gather.default, (x, idx))
    torch.library.opcheck(torch.ops.mmt.ce_index_invert.default, (idx, N_T + 25))


@pytest.mark.parametrize("n_in,n_out", [(26, 33), (33, 26), (300, 528), (1, 2048)])
def test_index_invert_exact(n_in, n_out):
    """(h) against scatter_, entries outside [0, n_out) skipped (negative, n_out itself, huge)."""
    import mmt_amd.ops  # noqa: F401
    g = torch.Generator().manual_seed(n_in)
    S = 4
    m = min(n_in, n_out)
    idx = torch.full((S, n_in), -1, dtype=torch.int32)
    for s in range(S):
        idx[s, torch.randperm(n_in, generator=g)[:m]] = torch.randperm(n_out, generator=g)[:m].int()
    if n_in > 3:
        idx[0, 0], idx[1, 1], idx[2, 2] = n_out, 1 << 30, -5
    ref = torch.full((S, n_out + 1), -1, dtype=torch.int32)
    ok = (idx >= 0) & (idx < n_out)
    ref.scatter_(1, torch.where(ok, idx, torch.full_like(idx, n_out)).long(), torch.arange(n_in, dtype=torch.int32).repeat(S, 1))
    got = torch.ops.mmt.ce_index_invert(idx.cuda(), n_out)
    assert torch.equal(got.cpu(), ref[:, :n_out])


@pytest.mark.parametrize("with_gidx", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n_s", [16, 25])
@pytest.mark.parametrize("dname", ["f32", "bf16"])
def test_ce_select_op(dname, n_s, masked, with_gidx):
    """(i) Bm = 2, H = 12, n_t = 8; n_s = 16: one MFMA key block of 32, n_s = 25: 50 keys, a ragged last block;
    keep = ceil(0.7 n_s).  order = the stable descending sort of the op's own attn_mean (exact), gidx_out =
    gidx_in[order], attn_mean within 1e-5 of its maximum of oracle.forward.ce_attn_mean (bf16: the oracle in fp32
    on the same bf16-rounded values; measured at most 2.4e-7 of the maximum in either dtype, so the 1e-5 bar holds)."""
    import mmt_amd.ops  # noqa: F401
    from oracle.forward import ce_attn_mean
    Bm, H, C = 2, 12, 768
    keep = math.ceil(0.7 * n_s)
    g = torch.Generator().manual_seed(100 * n_s + 2 * masked + with_gidx)
    qkv = torch.randn(2 * Bm, N_T + n_s, 3 * C, generator=g)
    if dname == "bf16":
        qkv = qkv.bfloat16()
    mask = None
    if masked:  # 4 per frame, one of each template grid's 4 queries
        mask = torch.zeros(Bm, 4, 4, dtype=torch.bool)
        for b in range(Bm):
            for q in range(4):
                mask[b, q, int(torch.randint(4, (1,), generator=g))] = True
        mask = mask.view(Bm, 2 * N_T)
    gin = torch.stack([torch.randperm(400, generator=g)[:n_s] for _ in range(2 * Bm)]).int() if with_gidx else None
    order, gout, am = torch.ops.mmt.ce_select(qkv.cuda(), None if mask is None else mask.cuda(),
                                              None if gin is None else gin.cuda(), N_T, H, keep)
    order, gout, am = order.cpu(), gout.cpu(), am.cpu()
    assert order.shape == (2 * Bm, keep) and gout.shape == (2 * Bm, keep) and am.shape == (Bm, 2 * n_s)
    for s in range(2 * Bm):
        m, b = s // Bm, s % Bm
        ref = torch.sort(am[b, m * n_s:(m + 1) * n_s], descending=True, stable=True)[1][:keep]
        assert torch.equal(order[s].long(), ref), s
        assert torch.equal(gout[s].long(), ref if gin is None else gin[s].long()[ref]), s
    q, k, _ = qkv.float().view(2 * Bm, N_T + n_s, 3, H, 64).permute(2, 0, 3, 1, 4).unbind(0)
    ref = ce_attn_mean(q[:Bm], q[Bm:], k[:Bm], k[Bm:], N_T, 64 ** -0.5, mask)
    err = ((am - ref).abs().max() / ref.abs().max()).item()
    print("ce_select %s n_s=%d masked=%s attn_mean err %.3g of its maximum" % (dname, n_s, masked, err))
    assert err <= 1e-5, err


# ----------------------------------------------------------------------------- the module at the bench geometry
def _bench_net():
    """The asym case of test_gpu_train_ops.test_module_forward_training_gpu_grads: head gain x6, the offset-bias
    nudge, BatchNorm in eval, dropout and stochastic depth off."""
    import mmt_amd.model as M
    torch.manual_seed(0)
    net = M.build_asymmetric_shared_ce(M.hot_path_cfg(), train=False)
    with torch.no_grad():
        for br in ("tl", "br"):
            getattr(net.box_head, "conv5_" + br).weight.mul_(6.0)
        for m in net.modules():
            if hasattr(m, "sampling_offsets"):
                m.sampling_offsets.bias.add_(1.0 / 3.0)
    net.train()
    net.drop_path_rate = 0.0
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eval()
    return net


@pytest.mark.parametrize("masked", [False, True])
def test_module_training_gpu_grads(masked):
    """(j) net(t, o, s, ce_template_mask=..., gt_bboxes=...) in train() mode on the HIP ops (bf16) at 128/320,
    B = 2: search lengths 400 -> 280 -> 196 -> 138.  The HIP run's selections are replayed (ce_forced) by the
    fp32 stand-in on the CPU and by the PyTorch-bf16 stand-in on the GPU, so all three compute the same function:
    loss within 2e-2 of fp32, each parameter group's gradient within max(3e-2, 1.2 x torch-bf16's own distance)
    (relative L2).  The HIP selections against an unforced fp32 run: kept-set overlap >= 0.9 per stage.
    masked: the CTR_POINT mask of the reference-made fixture."""
    sys.path.insert(0, os.path.dirname(__file__))
    from test_train import TorchOps
    from test_gpu_train_ops import _TorchBf16Ops
    import mmt_amd.train as T
    net = _bench_net()
    mask = torch.from_numpy(np.load(GOLDEN + "/model_asym_ce_mask_b2.npz")["ce_template_mask"]).bool() if masked else None
    t, o, s, gt = T.synthetic_batch(2, "cpu", torch.Generator().manual_seed(7))

    def run(ops, dev, forced=None):
        net.zero_grad(set_to_none=True)
        net.train_ops, net.ce_forced, net.ce_trace = ops, forced, []
        args = [[x.to(dev) for x in z] for z in (t, o, s)]
        _, coord = net(*args, gt_bboxes=None, ce_template_mask=None if mask is None else mask.to(dev))
        loss, _ = T.box_loss(coord, gt.to(dev))
        loss.backward()
        trace, net.ce_trace, net.ce_forced = net.ce_trace, None, None
        return loss.item(), {n: p.grad.float().cpu().clone() for n, p in net.named_parameters() if p.grad is not None}, trace

    net.cuda()
    hip_loss, hip, trace = run(None, "cuda")  # None = HipOps, the product path
    sel = [(gv.cpu(), gi.cpu()) for (gv, gi), _ in trace]
    assert [x[0].shape[1] for x in sel] == [280, 196, 138]
    tb_loss, tb, _ = run(_TorchBf16Ops, "cuda", sel)
    net.cpu()
    ref_loss, ref, _ = run(TorchOps, "cpu", sel)
    net.train_ops, net.ce_trace = TorchOps, []
    with torch.no_grad():  # the fp32 stand-in's own selections (forward only)
        T.module_forward(net, t, o, s, TorchOps, ce_template_mask=mask)
    free, net.ce_trace = net.ce_trace, None
    overlap = []
    for (gv, gi), ((fv, fi), _) in zip(sel, free):
        for a, b in ((gv, fv), (gi, fi)):
            overlap.append(min(len(set(a[r].tolist()) & set(b[r].tolist())) / a.shape[1] for r in range(2)))
    print("asym_ce masked=%s loss hip %.5f torch-bf16 %.5f fp32 %.5f; kept-set overlap with unforced fp32 %s"
          % (masked, hip_loss, tb_loss, ref_loss, ["%.3f" % x for x in overlap]))
    assert abs(hip_loss - ref_loss) <= 2e-2
    assert min(overlap) >= 0.9, overlap
    bad = []
    for grp in ("backbone", "fusion_vi", "box_head"):
        names = [n for n in ref if n.startswith(grp + ".")]
        r = torch.cat([ref[n].flatten() for n in names])
        g = torch.cat([hip[n].flatten() for n in names])
        b = torch.cat([tb[n].flatten() for n in names])
        rel, rel_tb = ((g - r).norm() / r.norm()).item(), ((b - r).norm() / r.norm()).item()
        print("asym_ce masked=%s %s grad rel L2: hip %.3g, torch-bf16 %.3g" % (masked, grp, rel, rel_tb))
        if rel > max(3e-2, 1.2 * rel_tb):
            bad.append((grp, rel, rel_tb))
    assert not bad, bad


def test_module_capture_and_train_step():
    """(k) the module's forward + backward (no optimizer) captured in one torch.cuda.graph after two eager
    warm-ups, replayed on new inputs copied into the static ones: gradients bitwise equal to an eager run on those
    inputs.  Then a captured TrainStep on asym_ce (CTR_POINT mask, keep rate 0.7): the loss falls over five
    replays on a fixed batch, and replay raises after the keep rate is changed."""
    import mmt_amd.train as T
    net = _bench_net().cuda()
    g = torch.Generator().manual_seed(5)
    b0, b1 = T.synthetic_batch(2, "cuda", g), T.synthetic_batch(2, "cuda", g)
    static = [[x.clone() for x in z] for z in b0[:3]] + [b0[3].clone()]

    def fwd_bwd(t, o, s, gt):
        _, coord = net(t, o, s, gt_bboxes=None)
        loss, _ = T.box_loss(coord, gt)
        loss.backward()
        return loss

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            net.zero_grad(set_to_none=True)
            fwd_bwd(*static)
    torch.cuda.current_stream().wait_stream(side)
    net.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fwd_bwd(*static)
    for dst, src in zip(static[0] + static[1] + static[2] + [static[3]], b1[0] + b1[1] + b1[2] + [b1[3]]):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    replayed = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    net.zero_grad(set_to_none=True)
    fwd_bwd(*b1)
    torch.cuda.synchronize()
    eager = {n: p.grad for n, p in net.named_parameters() if p.grad is not None}
    assert set(eager) == set(replayed) and len(eager) > 100
    diff = [n for n in eager if not torch.equal(eager[n], replayed[n])]
    assert not diff, diff[:5]
    del graph
    net.zero_grad(set_to_none=True)

    step = T.TrainStep(net, T.HipOps, lr=1e-4, ce_template_mask=T.ce_center_mask(2, 8, "cuda"), ce_keep_rate=0.7)
    step.capture(*static, warmup=1)
    losses = []
    for _ in range(5):
        losses.append(float(step.replay(*b1, ce_template_mask=T.ce_center_mask(2, 8, "cuda"))["loss"]))
    torch.cuda.synchronize()
    print("asym_ce captured step: losses of five replays %s" % ["%.5f" % x for x in losses])
    assert losses[-1] < losses[0], losses
    step.ce_keep_rate = 0.85
    with pytest.raises(RuntimeError, match="hyper-parameters changed"):
        step.replay(*b1)
