"""Candidate elimination in training (asymmetric_shared_ce.py:228-282, :372-447) on the CPU: the drop-in
module's train()-mode forward with the fp32 op stand-in of tests/test_train.py against autograd through the
oracle's restatement -- boxes, every parameter gradient and the discrete selections -- plus the ce_forced
replay hook, the keep-rate override, the rate-1.0 identity with the asym module, and the argument checks of
the two C entry points and the registered ops (no kernel runs here; GPU: tests/test_gpu_ce_train.py).

64 px search / 32 px template, B = 2: 16 search tokens, n_t = 8, 16 template queries; ratios 0.7 at blocks
3 / 6 / 9 keep 12, 9 and 7 tokens."""
import ctypes
import os
import sys

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

sys.path.insert(0, os.path.dirname(__file__))
from test_train import SEARCH, TEMPLATE, TorchOps, _batch  # noqa: E402

SEED = 0


def _ce_net(builder="build_asymmetric_shared_ce", seed=SEED):
    """As test_train._train_net: train() mode, fp32 stand-in ops, dropout and stochastic depth off, BatchNorm
    on running statistics."""
    import mmt_amd.model as M
    torch.manual_seed(seed)
    net = getattr(M, builder)(M.hot_path_cfg(search=SEARCH, template=TEMPLATE), train=False)
    with torch.no_grad():
        for br in ("tl", "br"):
            getattr(net.box_head, "conv5_" + br).weight.mul_(30.0)
    net.train()
    net.train_ops = TorchOps
    net.drop_path_rate = 0.0
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eval()
    return net


def _grid_mask(B):
    """One query of each of the four 2 x 2 template grids per frame ([template_V, online_V, template_I,
    online_I]), a different one per grid and frame."""
    m = torch.zeros(B, 4, 4, dtype=torch.bool)
    for b in range(B):
        for g in range(4):
            m[b, g, (g + b) % 4] = True
    return m.view(B, 16)


def _run(net, t, o, s, gt, **kw):
    from mmt_amd.train import box_loss
    net.zero_grad(set_to_none=True)
    net.ce_trace = []
    gt_xyxy = torch.cat([gt[:, :2], gt[:, :2] + gt[:, 2:]], 1)
    out, coord = net(t, o, s, run_score_head=False, gt_bboxes=gt_xyxy, **kw)
    assert out["pred_boxes"] is coord and coord.requires_grad
    loss, _ = box_loss(coord, gt)
    loss.backward()
    trace, net.ce_trace = net.ce_trace, None
    return coord.detach(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}, trace


def _oracle(net, t, o, s, gt, mask=None):
    from mmt_amd.train import box_loss
    from oracle.forward import forward as oracle_forward
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    leaves = {k: sd[k].requires_grad_() for k, p in net.named_parameters() if p.requires_grad}
    out, _, aux = oracle_forward.__wrapped__(sd, "asym_ce", t, o, s, return_aux=True, ce_template_mask=mask)
    loss, _ = box_loss(out["pred_boxes"], gt)
    loss.backward()
    return out["pred_boxes"].detach(), leaves, aux["ce_stages"]


def _check_against_oracle(kept, mask=None, **kw):
    torch.set_num_threads(8)
    net = _ce_net()
    t, o, s, gt = _batch(2, 3)
    coord, grads, trace = _run(net, t, o, s, gt, ce_template_mask=mask, **kw)
    ref, leaves, stages = _oracle(net, t, o, s, gt, mask)
    assert len(trace) == len(stages) == 3
    for ((gv, gi), am), (ram, rgv, rgi), k in zip(trace, stages, kept):
        lens = ram.shape[1] // 2
        for half in (ram[:, :lens], ram[:, lens:]):  # the cut is well above fp32 reordering (else: another SEED)
            srt = half.detach().sort(1, descending=True)[0]
            gap = ((srt[:, k - 1] - srt[:, k]) / srt[:, 0]).min().item()
            print("kept %d of %d, relative gap at the cut %.3g" % (k, lens, gap))
            assert gap >= 1e-4, gap
        assert gv.shape == (2, k) and gi.shape == (2, k)
        assert torch.equal(gv.long(), rgv) and torch.equal(gi.long(), rgi)
        assert (am - ram.detach()).abs().max().item() <= 1e-5 * ram.abs().max().item()
    assert (coord - ref).abs().max().item() < 1e-5
    n = 0
    for k, p in net.named_parameters():
        if not p.requires_grad or leaves[k].grad is None:
            continue
        g, rg = grads.get(k), leaves[k].grad
        assert g is not None, k
        assert (g - rg).abs().max().item() <= 1e-3 * rg.abs().max().item() + 1e-6, k
        n += 1
    assert n > 100


def test_module_grads_match_oracle():
    """(a) boxes, every parameter gradient and the selections (12, 9, 7 kept) against the oracle."""
    _check_against_oracle((12, 9, 7))


def test_module_grads_match_oracle_with_template_mask():
    """(b) the same with a ce_template_mask selecting one query of each of the four template grids."""
    _check_against_oracle((12, 9, 7), mask=_grid_mask(2))


def test_keep_rate_replaces_every_ratio(monkeypatch):
    """(c) ce_keep_rate = 0.85 replaces the ratio of every CE block: 14, 12 and 11 tokens kept."""
    import oracle.forward as OF
    monkeypatch.setattr(OF, "CE_KEEP", (0.85,) * 3)
    _check_against_oracle((14, 12, 11), ce_keep_rate=0.85)


def test_keep_rate_one_is_the_asym_module():
    """(d) ce_keep_rate >= 1 disables the elimination: bitwise the asym module on the same weights."""
    torch.set_num_threads(8)
    net = _ce_net()
    ref = _ce_net("build_asymmetric_shared")
    ref.load_state_dict(net.state_dict(), strict=True)
    t, o, s, gt = _batch(2, 3)
    coord, grads, trace = _run(net, t, o, s, gt, ce_keep_rate=1.0)
    assert trace == []
    from mmt_amd.train import box_loss
    _, rc = ref(t, o, s)
    box_loss(rc, gt)[0].backward()
    assert torch.equal(coord, rc.detach())
    rg = {k: p.grad for k, p in ref.named_parameters() if p.grad is not None}
    assert set(rg) == set(grads) and len(rg) > 100
    for k in rg:
        assert torch.equal(rg[k], grads[k]), k


def test_ce_forced_replays_and_is_live():
    """(e) ce_forced with a run's own selections reproduces it bitwise; another valid selection (the last kept
    token of the first stage swapped for a pruned one) moves the boxes: the hook is live."""
    torch.set_num_threads(8)
    net = _ce_net()
    t, o, s, gt = _batch(2, 3)
    coord, grads, trace = _run(net, t, o, s, gt)
    forced = [sel for sel, _ in trace]
    net.ce_forced = forced
    c2, g2, tr2 = _run(net, t, o, s, gt)
    assert torch.equal(c2, coord)
    for k in grads:
        assert torch.equal(g2[k], grads[k]), k
    for (sel, _), (sel2, _) in zip(trace, tr2):
        assert torch.equal(sel[0], sel2[0]) and torch.equal(sel[1], sel2[1])
    gv = forced[0][0].clone()
    for b in range(2):  # a pruned position in place of the last kept one (later stages keep earlier slots)
        pruned = sorted(set(range(16)) - set(gv[b].tolist()))
        later = set(forced[1][0][b].tolist())
        slot = [j for j in range(gv.shape[1]) if int(gv[b, j]) not in later][0]
        gv[b, slot] = pruned[0]
    net.ce_forced = [(gv, forced[0][1])] + forced[1:]
    c3, _, _ = _run(net, t, o, s, gt)
    net.ce_forced = None
    assert (c3 - coord).abs().max().item() > 1e-6
    bad = forced[1][0].clone()
    bad[0, 0] = sorted(set(range(16)) - set(forced[0][0][0].tolist()))[0]  # pruned at stage 1
    net.ce_forced = [forced[0], (bad, forced[1][1]), forced[2]]
    with pytest.raises(ValueError, match="pruned"):  # stage 2 may keep only what stage 1 kept
        _run(net, t, o, s, gt)
    net.ce_forced = None


def test_mask_validation_runs_in_training_mode():
    net = _ce_net()
    t, o, s, gt = _batch(2, 3)
    with pytest.raises(ValueError, match="shape"):
        net(t, o, s, ce_template_mask=torch.ones(2, 8, dtype=torch.bool))
    m = _grid_mask(2)
    m[1, 0] = m[1, 1] = True
    with pytest.raises(ValueError, match="same nonzero number"):
        net(t, o, s, ce_template_mask=m)
    # all-true means no mask
    c0, _, _ = _run(net, t, o, s, gt)
    c1, _, _ = _run(net, t, o, s, gt, ce_template_mask=torch.ones(2, 16, dtype=torch.bool))
    assert torch.equal(c0, c1)
    with pytest.raises(TypeError):  # the other variants take no CE arguments
        _ce_net("build_asymmetric_shared")(t, o, s, ce_keep_rate=0.7)


def test_center_mask_matches_reference_fixture():
    """ce_center_mask restates generate_mask_cond's CTR_POINT mask (ce_utils.py:14-38): the golden fixture's."""
    import numpy as np
    from conftest import GOLDEN
    from mmt_amd.train import ce_center_mask
    z = np.load(os.path.join(GOLDEN, "model_asym_ce_mask_b2.npz"))
    assert np.array_equal(z["ce_template_mask"].astype(bool), ce_center_mask(2, 8).numpy())
    for g, c in ((8, 3), (12, 5), (7, 3), (14, 6)):
        m = ce_center_mask(1, g).view(4, g, g)
        assert int(m.sum()) == 4 and bool(m[:, c, c].all())


# ----------------------------------------------------------------------------- C entry points, registry
def test_bad_arguments_rejected_without_gpu_work():
    """(f) mmt_ce_rows_gather / mmt_ce_index_invert validate on the host before any launch (MMT_EBADARG)."""
    from mmt_amd import _lib
    fake, other = 1 << 20, 1 << 22  # 16-B aligned, never dereferenced
    bad = -10000

    def gather(src=fake, src_rows=25, dst=other, dst_rows=18, idx=fake, S=4, C=768):
        return _lib.LIB.mmt_ce_rows_gather(src, src_rows, dst, dst_rows, idx, S, C, None)

    for kw in (dict(src=None), dict(dst=None), dict(idx=None), dict(C=770), dict(C=1028), dict(C=0), dict(dst=fake),
               dict(S=0), dict(src_rows=0), dict(dst_rows=0), dict(dst_rows=-3), dict(S=1 << 16)):
        assert gather(**kw) == bad, kw

    def invert(idx_in=fake, n_in=18, idx_out=other, n_out=25, S=4):
        return _lib.LIB.mmt_ce_index_invert(idx_in, n_in, idx_out, n_out, S, None)

    for kw in (dict(idx_in=None), dict(idx_out=None), dict(idx_out=fake), dict(n_in=0), dict(n_out=0), dict(S=0),
               dict(n_out=2049), dict(S=-1)):
        assert invert(**kw) == bad, kw
    _ = ctypes


OPS = ["ce_select", "ce_rows_gather", "ce_index_invert"]


@pytest.mark.parametrize("name", OPS)
def test_op_registered(name):
    import mmt_amd.ops  # noqa: F401
    assert hasattr(torch.ops.mmt, name)
    assert torch._C._dispatch_has_kernel_for_dispatch_key("mmt::" + name, "Meta")  # the fake kernel


def test_rows_gather_has_autograd():
    import mmt_amd.ops  # noqa: F401
    assert torch._C._dispatch_has_kernel_for_dispatch_key("mmt::ce_rows_gather", "Autograd")


def test_fake_shapes():
    import mmt_amd.ops  # noqa: F401
    with FakeTensorMode():
        q = torch.empty(4, 8 + 25, 3 * 768, dtype=torch.bfloat16)
        order, gidx, am = torch.ops.mmt.ce_select(q, torch.empty(2, 16, dtype=torch.uint8),
                                                  torch.empty(4, 25, dtype=torch.int32), 8, 12, 18)
        assert order.shape == (4, 18) and order.dtype == torch.int32
        assert gidx.shape == (4, 18) and gidx.dtype == torch.int32
        assert am.shape == (2, 50) and am.dtype == torch.float32
        x = torch.empty(4, 33, 768)
        idx = torch.empty(4, 26, dtype=torch.int32)
        y = torch.ops.mmt.ce_rows_gather(x, idx)
        assert y.shape == (4, 26, 768) and y.dtype == torch.float32
        inv = torch.ops.mmt.ce_index_invert(idx, 33)
        assert inv.shape == (4, 33) and inv.dtype == torch.int32


def test_cpu_tensors_raise():
    import mmt_amd.ops  # noqa: F401
    idx = torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CUDA"):
        torch.ops.mmt.ce_rows_gather(torch.zeros(2, 5, 8), idx)
    with pytest.raises(RuntimeError, match="CUDA"):
        torch.ops.mmt.ce_index_invert(idx, 5)
    with pytest.raises(RuntimeError, match="CUDA"):
        torch.ops.mmt.ce_select(torch.zeros(2, 24, 2304), None, None, 8, 12, 12)
