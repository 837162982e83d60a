"""RGBT_Fusion_Cat (fusion_utils.py:86-110), the concat-conv fusion front-end, on the MI355X: the inference plan
(three implicit-GEMM 3x3 convs with the BatchNorms folded, the first reading the two modalities' search rows in place
through the conv mode's channel split) against the reference's own forward (tests/golden/make_golden_cat.py), the
cached passes, the score head, hipGraph replay, the batched tracker, and the training forward / backward on the HIP
ops.  Bars are the project's own: boxes within 1e-3 (fp32) / 1e-2 (bf16, fp16) of the reference (BASELINE.md,
tests/test_gpu_model.py)."""
import copy
import json

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CAT = "RGBT_Fusion_Cat"
DTYPES = {"f32": (torch.float32, 1e-3), "bf16": (torch.bfloat16, 1e-2), "f16": (torch.float16, 1e-2)}
GOLD = {"asym": "model_asym_fusion_cat", "shared": "model_shared_fusion_cat"}
_RT, _SD = {}, {}


def _weights(variant):
    if variant not in _SD:
        from mmt_amd import synthetic
        from mmt_amd.model import reference_state_dict_shapes
        keys = reference_state_dict_shapes("asym" if variant == "asym_ce" else variant, fusion_class=CAT)
        _SD[variant] = {k: torch.from_numpy(v) for k, v in synthetic.synth_state_dict(keys).items()}
    return _SD[variant]


def _runtime(variant, dtype):
    if (variant, dtype) not in _RT:
        from mmt_amd.runtime import MixFormerRGBTRuntime
        _RT[(variant, dtype)] = MixFormerRGBTRuntime(_weights(variant), variant, dtype=dtype)
    return _RT[(variant, dtype)]


def _inputs(B):
    from mmt_amd import synthetic
    t, o, s = synthetic.synth_inputs(B)
    return [x.cuda() for x in t], [x.cuda() for x in o], [x.cuda() for x in s]


# ----------------------------------------------------------------------------- model vs golden
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("variant,B", [("asym", 1), ("shared", 2)])
def test_model_matches_reference(variant, B, dname):
    dtype, tol = DTYPES[dname]
    rt = _runtime(variant, dtype)
    assert rt.d.cat and rt.d.fusion_layers == 0 and "enc" not in rt.w
    box, _ = rt.forward(*_inputs(B))
    torch.cuda.synchronize()
    gold = np.load(GOLDEN + "/%s_b%d.npz" % (GOLD[variant], B))
    err = np.abs(box.cpu().numpy() - gold["pred_boxes"].reshape(B, 4)).max()
    ws = rt.workspace(B)
    maps = ws["MAPS"].cpu().numpy()
    merr = max(np.abs(maps[g] - gold[nm].reshape(B, -1)).max() / max(1.0, np.abs(gold[nm]).max())
               for g, nm in enumerate(("score_map_tl", "score_map_br")))
    # the fused map (fp32 copy, channels-last) against the golden's subsample of the reference's NCHW output
    fused = ws["FUS"].view(B, rt.d.ns, rt.d.C).permute(0, 2, 1).reshape(-1).double().cpu()
    step = max(1, fused.numel() // 4096)
    fsub = fused[::step][:4096].numpy()
    ferr = np.abs(fsub - gold["fused_sub"]).max() / np.abs(gold["fused_sub"]).max()
    print("%s + Cat B=%d %s: box err %.3g, rel map err %.3g, rel fused err %.3g" % (variant, B, dname, err, merr, ferr))
    assert err <= tol, err
    assert merr <= (1e-4 if dname == "f32" else 5e-2), merr  # tests/test_gpu_model.py's map bars
    names = [e[2] for e in ws["plan"]]
    assert [n for n in names if n.startswith("fusion")][:3] == ["fusion_cat1", "fusion_cat2", "fusion_cat3"]
    assert not any(n in names for n in ("fusion_adjust", "fusion_gn", "msda_bimodal", "fusion_adjust_cat"))


def test_first_conv_reads_the_backbone_output_in_place():
    """No concat copy: the first conv's two A pointers are the two modality row blocks of the backbone output, its
    split is C and its image pitch the sequence length; mmt_gemm_select answers the LDS-DMA kernel for all three."""
    from mmt_amd import _lib as L
    rt = _runtime("asym", torch.bfloat16)
    ws, d = rt.workspace(1), rt.d
    ent = {e[2]: e[3] for e in ws["plan"] if e[2].startswith("fusion_cat")}
    p = ent["fusion_cat1"]
    es = ws["XN"].element_size()
    assert p.a[0] == ws["XN"].data_ptr() + d.n_t * d.C * es
    assert p.a1[0] == ws["XN"].data_ptr() + (d.ntok + d.n_t) * d.C * es
    assert (p.k_split, p.conv_cin, p.a_stride_a, p.lda, p.conv_h) == (d.C, 2 * d.C, d.ntok, d.C, d.gs)
    for nm, q in ent.items():
        c = L.gemm_select(q, L.MMT_BF16)
        assert c is not None and c.family == L.GEMM_LDS_DMA and c.conv == 1, nm


@pytest.mark.parametrize("head", ["f32", "f16"])
def test_head_storage_type_other_than_the_compute_dtype(head):
    """bf16 backbone and fusion with the head's activations and weights in another type (runtime head_dtype): an
    fp32 head reads the third conv's fp32 map itself, a 16-bit head of another type gets it through a cast launch.
    The 16-bit box bar holds (the backbone is bf16)."""
    from mmt_amd.runtime import MixFormerRGBTRuntime
    rt = MixFormerRGBTRuntime(_weights("asym"), "asym", dtype=torch.bfloat16, head_dtype=DTYPES[head][0])
    box, _ = rt.forward(*_inputs(1))
    torch.cuda.synchronize()
    gold = np.load(GOLDEN + "/%s_b1.npz" % GOLD["asym"])
    err = np.abs(box.cpu().numpy() - gold["pred_boxes"].reshape(1, 4)).max()
    names = [e[2] for e in rt.workspace(1)["plan"]]
    print("asym + Cat bf16, %s head: box err %.3g" % (head, err))
    assert err <= 1e-2
    assert ("fusion_cat_cast" in names) == (head == "f16")


def test_graph_replay_is_bitwise_eager():
    rt = _runtime("asym", torch.bfloat16)
    t, o, s = _inputs(1)
    b0 = rt.forward(t, o, s)[0].clone()
    b1, _ = rt.forward(t, o, s, use_graph=True)
    torch.cuda.synchronize()
    assert torch.equal(b0, b1)


# ----------------------------------------------------------------------------- cached passes, score head
@pytest.mark.parametrize("dname", ["f32", "bf16"])
@pytest.mark.parametrize("variant", ["asym", "asym_ce"])
def test_cached_forward_matches_full_and_golden(variant, dname):
    """tests/test_gpu_fusion_variants.py::test_cached_forward_matches_full_and_golden's bars: the cached pass within
    the dtype's tolerance of the full forward (and, where the reference has the case, of the golden boxes).  asym_ce
    has the asym model's parameters; the reference ships no Cat yaml for it, so it is held to its own full forward."""
    dtype, tol = DTYPES[dname]
    rt = _runtime(variant, dtype)
    t, o, s = _inputs(1)
    full = rt.forward(t, o, s)[0].clone()
    rt.set_template(t, o)
    box, _ = rt.forward_search(s)
    torch.cuda.synchronize()
    err_f = (box - full).abs().max().item()
    assert bool(torch.isfinite(box).all())
    if variant == "asym":
        gold = np.load(GOLDEN + "/%s_b1.npz" % GOLD[variant])
        err_g = np.abs(box.cpu().numpy() - gold["pred_boxes"].reshape(1, 4)).max()
        print("%s + Cat %s: cached vs golden %.3g, vs full %.3g" % (variant, dname, err_g, err_f))
        assert err_g <= tol
    else:
        print("%s + Cat %s: cached vs full %.3g" % (variant, dname, err_f))
    assert err_f <= tol


@pytest.mark.parametrize("dname,tol", [("f32", 1e-3), ("bf16", 1e-2)])
def test_online_score_head_full_and_cached(dname, tol):
    """asym_online + Cat: the score head's RoI pool reads the fp32 fused map the third conv writes; scores finite,
    and the cached pass equals the full pass within tests/test_gpu_cache.py's bar (boxes and scores within tol)."""
    rt = _runtime("asym_online", DTYPES[dname][0])
    t, o, s = _inputs(1)
    box_full, sc_full = rt.forward(t, o, s, run_score_head=True)
    box_full, sc_full = box_full.clone(), sc_full.clone()
    rt.set_template(t, o)
    box, sc = rt.forward_search(s, run_score_head=True)
    torch.cuda.synchronize()
    print("asym_online + Cat %s: score %.5f, cached vs full: box %.3g, score %.3g"
          % (dname, sc_full.item(), (box - box_full).abs().max().item(), (sc - sc_full).abs().max().item()))
    assert bool(torch.isfinite(sc_full).all()) and bool(torch.isfinite(sc).all())
    assert (box - box_full).abs().max().item() <= tol and (sc - sc_full).abs().max().item() <= tol


def test_module_forward_set_online_forward_test():
    from mmt_amd.model import build_asymmetric_shared_online_score, hot_path_cfg
    model = build_asymmetric_shared_online_score(hot_path_cfg(fusion_class=CAT), train=False)
    model.load_state_dict(_weights("asym_online"), strict=True)
    model = model.cuda().eval()
    t, o, s = _inputs(1)
    with torch.no_grad():
        full, _ = model(t, o, s, run_score_head=True)
        model.set_online(t, o)
        out, _ = model.forward_test(s, run_score_head=True)
    assert bool(torch.isfinite(full["pred_scores"]).all())
    assert (out["pred_boxes"] - full["pred_boxes"]).abs().max().item() <= 1e-2
    assert (out["pred_scores"] - full["pred_scores"]).abs().max().item() <= 1e-2


# ----------------------------------------------------------------------------- batched tracker
def _tracker_params(**over):
    from types import SimpleNamespace

    from mmt_amd.model import hot_path_cfg
    cfg = hot_path_cfg(fusion_class=CAT)
    cfg.TEST.UPDATE_INTERVALS = {"SYNTH": [3]}
    p = SimpleNamespace(cfg=cfg, template_factor=2.0, template_size=128, search_factor=5.0, search_size=320,
                        checkpoint=None, save_all_boxes=False)
    for k, v in over.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("slot_cache", [False, True])
def test_batched_tracker_equals_single_trackers(slot_cache):
    """lib/test/tracker/asymmetric_shared with a Cat cfg, fp32 HIP path: 2 slots over 3 tracked frames of synthetic
    64x80 sequences equal two single trackers on the same frames within tests/test_gpu_batch_tracker.py's bar
    (1e-3 of the search crop: 1e-3 * 320 / resize_factor px); with the per-slot template cache the two assigns cost
    one refresh before the first step and none after (the frame-3 re-crop is refreshed by the step after it)."""
    from lib.test.tracker import asymmetric_shared
    from test_gpu_batch_tracker import _seq
    sd = _weights("asym")
    over = dict(slot_cache=True) if slot_cache else {}
    trk = asymmetric_shared.get_batch_tracker_class()(_tracker_params(**over), "synth", 2)
    trk.network.load_state_dict(sd, strict=True)
    trk.network.set_compute_dtype(torch.float32)
    assert type(trk.network.fusion_vi).__name__ == CAT
    seqs = [_seq(4, H=64, W=80, x0=20 + 6 * b, y0=14 + 4 * b, side=16, seed=b) for b in range(2)]
    singles = []
    for b, (frames, init) in enumerate(seqs):
        trk.initialize(b, frames[0], {"init_bbox": [init, init]})
        one = asymmetric_shared.get_tracker_class()(_tracker_params(), "synth")
        one.network.load_state_dict(sd, strict=True)
        one.network.set_compute_dtype(torch.float32)
        one.core._plan = one.core._graph = None
        one.initialize(frames[0], {"init_bbox": [init, init]})
        singles.append(one)
    counts = []
    for f in range(1, 4):
        out = trk.track({b: seqs[b][0][f] for b in range(2)})
        rf = trk.core.search_crop[:, 0, 3].tolist()
        counts.append(trk.core.refresh_replays)
        for b in range(2):
            ref = singles[b].track(seqs[b][0][f], {})["target_bbox"]
            tol = 1e-3 * 320 / rf[b]
            err = max(abs(x - y) for x, y in zip(out[b]["target_bbox"], ref))
            print("slot_cache %s frame %d slot %d: batched vs single %.3g px (tol %.3g)" % (slot_cache, f, b, err, tol))
            assert err <= tol, (f, b, out[b]["target_bbox"], ref)
    assert counts == ([1, 1, 1] if slot_cache else [0, 0, 0])
    assert trk.core._graph is not None


# ----------------------------------------------------------------------------- training
def _stack(c):
    """The reference's module chain written out: Conv3x3(bias=False) -> BatchNorm2d -> ReLU, three times."""
    return nn.Sequential(nn.Conv2d(2 * c, 2 * c, 3, 1, 1, bias=False), nn.BatchNorm2d(2 * c), nn.ReLU(),
                         nn.Conv2d(2 * c, c, 3, 1, 1, bias=False), nn.BatchNorm2d(c), nn.ReLU(),
                         nn.Conv2d(c, c, 3, 1, 1, bias=False), nn.BatchNorm2d(c), nn.ReLU())


def _bf16_st(x):
    """x rounded to bf16 in the forward, identity in the backward: where the HIP path stores a bf16 map."""
    return x + (x.bfloat16().float() - x).detach()


def _run_stack(stack, x):
    for i in range(0, 9, 3):
        x = _bf16_st(stack[i](x))                 # the conv's bf16 output map
        x = _bf16_st(stack[i + 2](stack[i + 1](x)))  # the norm + ReLU's bf16 output map
    return x


def _cat_pair(c, seed):
    """(RGBT_Fusion_Cat(c) on the device, the written-out stack on the CPU) with the same bf16-representable conv
    weights and non-trivial norm parameters and running statistics, both in train mode."""
    from mmt_amd.model import RGBT_Fusion_Cat
    torch.manual_seed(seed)
    fu, st = RGBT_Fusion_Cat(c), _stack(c)
    with torch.no_grad():
        for i in (1, 2, 3):
            cv, bn = getattr(fu, "fusion%d" % i), getattr(fu, "fusion%d_bn" % i)
            cv.weight.copy_(cv.weight.bfloat16().float())
            bn.weight.copy_(1 + 0.2 * torch.randn_like(bn.weight))
            bn.bias.copy_(0.2 * torch.randn_like(bn.bias))
            bn.running_mean.copy_(0.1 * torch.randn_like(bn.running_mean))
            bn.running_var.copy_(1 + 0.2 * torch.rand_like(bn.running_var))
            st[3 * i - 3].load_state_dict(cv.state_dict())
            st[3 * i - 2].load_state_dict(bn.state_dict())
    return fu.cuda().train(), st.train()


def _rel(a, r):
    return ((a.detach().float().cpu() - r.detach()).norm() / r.detach().norm().clamp_min(1e-12)).item()


def test_training_forward_backward_small():
    """RGBT_Fusion_Cat(8) (16 -> 16 -> 8 -> 8 channels), 4 x 4 maps, B = 2, train mode: fusion_forward on HipOps
    against the written-out nn.Conv2d / nn.BatchNorm2d stack in fp32 on the same bf16-rounded operands (inputs,
    weights, and each map the HIP path stores in bf16).  Bars, relative L2, from tests/test_gpu_train_ops.py:
      output 1e-2          (test_hip_conv3x3_autograd's y, test_hip_batchnorm_relu's y)
      dX, dW 2e-2          (test_hip_conv3x3_autograd's dx / dw, test_hip_batchnorm_relu's dX)
      dgamma, dbeta 1e-3   for fusion3_bn, whose dY is the test's own (test_hip_batchnorm_relu's condition: a given
                           dY rounded to bf16); 2e-2 for fusion1_bn / fusion2_bn, whose dY is the dX of the ops
                           behind them and so carries that bar
      running mean / variance rtol 1e-5 / 1e-4 (test_hip_batchnorm_relu), num_batches_tracked exactly."""
    from mmt_amd.train import HipOps, fusion_forward
    c, B, h = 8, 2, 4
    fu, st = _cat_pair(c, 5)
    g = torch.Generator().manual_seed(9)
    sv = torch.randn(B, c, h, h, generator=g).bfloat16().float()
    si = torch.randn(B, c, h, h, generator=g).bfloat16().float()
    dy = torch.randn(B, c, h, h, generator=g).bfloat16().float()
    rv, ri = sv.clone().requires_grad_(True), si.clone().requires_grad_(True)
    yr = _run_stack(st, torch.cat([rv, ri], 1))
    yr.backward(dy)
    dv, di = sv.cuda().requires_grad_(True), si.cuda().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        yd = fusion_forward(fu, dv, di, HipOps)
    assert tuple(yd.shape) == (B, c, h, h)
    yd.backward(dy.cuda().to(yd.dtype))
    torch.cuda.synchronize()
    figs = {"y": (_rel(yd, yr), 1e-2), "dx_v": (_rel(dv.grad, rv.grad), 2e-2), "dx_i": (_rel(di.grad, ri.grad), 2e-2)}
    for i in (1, 2, 3):
        cv, bn = getattr(fu, "fusion%d" % i), getattr(fu, "fusion%d_bn" % i)
        figs["dw%d" % i] = (_rel(cv.weight.grad, st[3 * i - 3].weight.grad), 2e-2)
        tol = 1e-3 if i == 3 else 2e-2
        figs["dgamma%d" % i] = (_rel(bn.weight.grad, st[3 * i - 2].weight.grad), tol)
        figs["dbeta%d" % i] = (_rel(bn.bias.grad, st[3 * i - 2].bias.grad), tol)
    print("Cat(8) training, relative L2 (bar): " + ", ".join("%s %.3g (%.0e)" % (k, v, t) for k, (v, t) in figs.items()))
    bad = {k: v for k, (v, t) in figs.items() if not v <= t}
    assert not bad, bad
    for i in (1, 2, 3):
        bn, rb = getattr(fu, "fusion%d_bn" % i), st[3 * i - 2]
        assert torch.allclose(bn.running_mean.cpu(), rb.running_mean, rtol=1e-5, atol=1e-6), i
        assert torch.allclose(bn.running_var.cpu(), rb.running_var, rtol=1e-4, atol=1e-6), i
        assert int(bn.num_batches_tracked) == int(rb.num_batches_tracked) == 1
    # token rows (2B, ns, C) bf16, as the two-stream backbones hand them over: the same maps, the same result
    rows = torch.cat([sv, si], 0).flatten(2).transpose(1, 2).contiguous().bfloat16().cuda()
    fu2, _ = _cat_pair(c, 5)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y2 = fusion_forward(fu2, rows, None, HipOps)
    assert torch.equal(y2.float(), yd.detach().float())
    # eval: the running statistics, nothing advances
    fu.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        ye = fusion_forward(fu, dv.detach(), di.detach(), HipOps)
    st.eval()
    with torch.no_grad():
        ere = _run_stack(st, torch.cat([sv, si], 1))
    assert _rel(ye, ere) <= 1e-2 and int(fu.fusion1_bn.num_batches_tracked) == 1


def test_training_forward_full_width():
    """The same stack at full width (C = 768, 20 x 20, B = 2, train mode), forward only: output within 1e-2
    relative L2 (test_hip_conv3x3_autograd's and test_hip_batchnorm_relu's output bar)."""
    from mmt_amd.train import HipOps, fusion_forward
    c, B, h = 768, 2, 20
    fu, st = _cat_pair(c, 6)
    g = torch.Generator().manual_seed(10)
    rows = torch.randn(2 * B, h * h, c, generator=g).bfloat16()
    x = rows.float().transpose(1, 2).reshape(2 * B, c, h, h)
    with torch.no_grad():
        yr = _run_stack(st, torch.cat([x[:B], x[B:]], 1))
        with torch.autocast("cuda", dtype=torch.bfloat16):
            yd = fusion_forward(fu, rows.cuda(), None, HipOps)
    torch.cuda.synchronize()
    err = _rel(yd, yr)
    print("Cat(768) training forward: relative L2 %.3g" % err)
    assert tuple(yd.shape) == (B, c, h, h) and err <= 1e-2
    # (the running statistics' own bars hold for one norm on one input, test_training_forward_backward_small; here
    # each norm's input already differs from the stack's by the rounding of the ops before it)
    for i in (1, 2, 3):
        assert int(getattr(fu, "fusion%d_bn" % i).num_batches_tracked) == 1


def test_captured_train_step_asym_cat():
    """asym + Cat (experiments/asymmetric_shared/attention_lasher_cat_3layer.yaml), 2 pairs, BatchNorm in train mode:
    TrainStep.capture / replay against the same steps run eagerly from the same weights -- the replayed loss and
    every parameter within 1e-6 of the eager ones (tests/test_gpu_train_ops.py::
    test_train_step_graph_replay_matches_eager's bar) -- and, as tests/test_gpu_fusion_variants.py::
    test_captured_train_step_asym_ce_add2 checks, every trainable parameter has a gradient and the fusion's move.
    param_groups: every fusion_vi parameter at the fusion's 1.0 lr."""
    import mmt_amd.model as M
    import mmt_amd.train as T
    torch.manual_seed(0)
    net = M.build_asymmetric_shared(M.hot_path_cfg(fusion_class=CAT), train=False)
    with torch.no_grad():
        for br in ("tl", "br"):
            getattr(net.box_head, "conv5_" + br).weight.mul_(6.0)
    net.drop_path_rate = 0.0
    net_b = copy.deepcopy(net)
    net, net_b = net.cuda().train(), net_b.cuda().train()
    gen = torch.Generator().manual_seed(5)
    batches = [T.synthetic_batch(2, "cuda", gen) for _ in range(3)]
    before = {n: p.detach().clone() for n, p in net_b.named_parameters() if n.startswith("fusion_vi.")}
    assert len(before) == 9
    eager, graphed = T.TrainStep(net, T.HipOps, lr=1e-4), T.TrainStep(net_b, T.HipOps, lr=1e-4)
    fus = {id(p) for n, p in net.named_parameters() if n.startswith("fusion_vi.")}
    for grp in T.param_groups(net, 1e-4):
        if any(id(p) in fus for p in grp["params"]):
            assert "lr" not in grp and {id(p) for p in grp["params"]} == fus
    le = [float(eager(*b)["loss"]) for b in batches]
    static = [[x.clone() for x in z] if isinstance(z, list) else z.clone() for z in batches[0]]
    graphed.capture(*static, warmup=1)  # one eager warm-up step on batch 0
    graphed.replay(*batches[1])
    lg = float(graphed.replay(*batches[2])["loss"])
    torch.cuda.synchronize()
    print("asym + Cat: eager losses %s, replayed third step %.6f" % (["%.6f" % x for x in le], lg))
    assert abs(le[2] - lg) <= 1e-6 * max(1.0, abs(le[2])), (le, lg)
    params_b = dict(net_b.named_parameters())
    for n, pa in net.named_parameters():
        if pa.requires_grad:
            err = (pa - params_b[n]).abs().max().item()
            assert err <= 1e-6 * max(1.0, pa.abs().max().item()), (n, err)
    assert not [n for n, p in params_b.items() if p.requires_grad and p.grad is None]
    assert all(not torch.equal(params_b[n].detach(), before[n]) for n in before)
    for i in (1, 2, 3):
        assert int(getattr(net_b.fusion_vi, "fusion%d_bn" % i).num_batches_tracked) == 3
