"""The deformable fusion front-ends Attention_Fusion_Bimodal / _LNSpecific_Sum / _LNSpecific_2 and the
uni-backbone model on the MI355X.  Each is Attention_Fusion_Bimodal_LNSpecific with weights tied
(runtime._prepare_fusion, model.fusion_parts / layer_norms), so the launch list is the LNSpecific plan's and
the bars are the project's own: boxes within 1e-3 (fp32) / 1e-2 (bf16, fp16) of the reference's
own forward (tests/golden/make_golden_fusion.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(__file__))
from test_fusion_variants_host import CLASSES, LNS, _tied_grads, _twin, tie_to_lnspecific  # noqa: E402

pytestmark = pytest.mark.gpu

# name -> (runtime variant, fusion class, layers, golden stem)
MODELS = {"asym_bimodal": ("asym", CLASSES["bimodal"], 2, "model_asym_fusion_bimodal"),
          "asym_sum": ("asym", CLASSES["sum"], 2, "model_asym_fusion_sum"),
          "asym_add2": ("asym", CLASSES["add2"], 2, "model_asym_fusion_add2"),
          "rgbt_bimodal6": ("rgbt", CLASSES["bimodal"], 6, "model_rgbt_fusion_bimodal6"),
          "uni": ("uni", LNS, 2, "model_uni")}
DTYPES = {"f32": (torch.float32, 1e-3), "bf16": (torch.bfloat16, 1e-2), "f16": (torch.float16, 1e-2)}
_RT = {}


def _weights(name):
    from mmt_amd import synthetic
    from mmt_amd.model import reference_state_dict_shapes
    variant, cls, layers, _ = MODELS[name]
    keys = reference_state_dict_shapes(variant, fusion_layers=layers, fusion_class=cls)
    return {k: torch.from_numpy(v) for k, v in synthetic.synth_state_dict(keys).items()}


def _runtime(name, dtype):
    if (name, dtype) not in _RT:
        from mmt_amd.runtime import MixFormerRGBTRuntime
        _RT[(name, dtype)] = MixFormerRGBTRuntime(_weights(name), MODELS[name][0], dtype=dtype)
    return _RT[(name, dtype)]


def _inputs(B):
    from mmt_amd import synthetic
    t, o, s = synthetic.synth_inputs(B)
    return [x.cuda() for x in t], [x.cuda() for x in o], [x.cuda() for x in s]


# ----------------------------------------------------------------------------- G1
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name,B", [("asym_bimodal", 1), ("asym_sum", 1), ("asym_add2", 1), ("rgbt_bimodal6", 1),
                                    ("uni", 1), ("uni", 2)])
def test_model_matches_reference(name, B, dname):
    dtype, tol = DTYPES[dname]
    rt = _runtime(name, dtype)
    box, _ = rt.forward(*_inputs(B))
    torch.cuda.synchronize()
    gold = np.load(GOLDEN + "/%s_b%d.npz" % (MODELS[name][3], B))
    err = np.abs(box.cpu().numpy() - gold["pred_boxes"].reshape(B, 4)).max()
    maps = rt.workspace(B)["MAPS"].cpu().numpy()
    merr = max(np.abs(maps[g] - gold[nm].reshape(B, -1)).max() / max(1.0, np.abs(gold[nm]).max())
               for g, nm in enumerate(("score_map_tl", "score_map_br")))
    print("%s B=%d %s: box err %.3g, rel map err %.3g" % (name, B, dname, err, merr))
    assert err <= tol, err
    assert merr <= (1e-4 if dname == "f32" else 5e-2), merr  # tests/test_gpu_model.py's map bars


def test_tied_entries_are_one_device_tensor():
    """A tied pair is the same tensor behind both W[...] entries (it cannot drift, and no memory is added)."""
    w = _runtime("asym_add2", torch.bfloat16).w
    assert w["adj_v.w"] is w["adj_i.w"] and w["adj_v.gn"] is w["adj_i.gn"]
    assert tuple(w["adj_cat.w"].shape) == (768, 1024) and torch.equal(w["adj_cat.w"][:, :512], w["adj_cat.w"][:, 512:])
    e = _runtime("asym_bimodal", torch.bfloat16).w["enc"][0]
    assert e["norm1_v"] is e["norm1_i"] and e["norm2_v"] is e["norm2_i"]
    blk = _runtime("uni", torch.bfloat16).w["bb"][0]["blocks"][0]
    assert blk["attn.qkv.fw"][0] is blk["attn.qkv.fw"][1] and blk["mlp.fc1.fcs"][0] is blk["mlp.fc1.fcs"][1]
    assert _runtime("uni", torch.float32).w["bb"][0]["blocks"][0]["norm1_v"] is \
        _runtime("uni", torch.float32).w["bb"][0]["blocks"][0]["norm1_i"]


def test_six_layers_add_28_launches():
    """Four more encoder layers = 4 x 7 launches; nothing else in the plan depends on the layer count."""
    from mmt_amd.runtime import MixFormerRGBTRuntime
    sd = _weights("rgbt_bimodal6")
    sd2 = {k: v for k, v in sd.items() if not any(".encoder.layers.%d." % i in k for i in range(2, 6))}
    n6 = len(_runtime("rgbt_bimodal6", torch.bfloat16).workspace(1)["plan"])
    n2 = len(MixFormerRGBTRuntime(sd2, "rgbt", dtype=torch.bfloat16).workspace(1)["plan"])
    assert n6 - n2 == 28


# ----------------------------------------------------------------------------- G2
def test_graph_replay_is_bitwise_eager():
    rt = _runtime("asym_add2", torch.bfloat16)
    t, o, s = _inputs(1)
    b0 = rt.forward(t, o, s)[0].clone()
    b1, _ = rt.forward(t, o, s, use_graph=True)
    torch.cuda.synchronize()
    assert torch.equal(b0, b1)


# ----------------------------------------------------------------------------- G3
@pytest.mark.parametrize("dname", ["f32", "bf16"])
@pytest.mark.parametrize("name,B", [("asym_add2", 1), ("uni", 2)])
def test_cached_forward_matches_full_and_golden(name, B, dname):
    """tests/test_gpu_cache.py's bars for asym / shared: the cached pass within the dtype's tolerance of the
    golden boxes and of the full forward."""
    dtype, tol = DTYPES[dname]
    rt = _runtime(name, dtype)
    t, o, s = _inputs(B)
    full = rt.forward(t, o, s)[0].clone()
    rt.set_template(t, o)
    box, _ = rt.forward_search(s)
    torch.cuda.synchronize()
    gold = np.load(GOLDEN + "/%s_b%d.npz" % (MODELS[name][3], B))
    err_g = np.abs(box.cpu().numpy() - gold["pred_boxes"].reshape(B, 4)).max()
    err_f = (box - full).abs().max().item()
    print("%s B=%d %s: cached vs golden %.3g, vs full %.3g" % (name, B, dname, err_g, err_f))
    assert err_g <= tol and err_f <= tol


def test_uni_module_set_online_forward_test():
    from mmt_amd.model import build_mixformer_vit_rgbt_uni, hot_path_cfg
    model = build_mixformer_vit_rgbt_uni(hot_path_cfg(), train=False)
    model.load_state_dict(_weights("uni"), strict=True)
    model = model.cuda().eval()
    t, o, s = _inputs(1)
    with torch.no_grad():
        full, _ = model(t, o, s)
        model.set_online(t, o)
        out, _ = model.forward_test(s)
    assert (out["pred_boxes"] - full["pred_boxes"]).abs().max().item() <= 1e-2


# ----------------------------------------------------------------------------- G4
NAN = float("nan")
PAD = 8


def _poisoned(x):
    """x (rows, cols) followed by PAD rows of NaN, on the device; returns (storage, view of x's rows)."""
    st = torch.cat([x, torch.full((PAD,) + tuple(x.shape[1:]), NAN, dtype=x.dtype)]).cuda()
    return st, st[:x.shape[0]]


def _same(a, b):
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


@pytest.mark.parametrize("ns", [1, 400])
def test_layernorm_same_pointer_for_both_sets(ns):
    """mmt_layernorm with two affine sets alternating every rows0 = ns rows (the encoder's enc_ln1 / enc_ln2 at
    B = 1, d_model = 512, with the residual add of enc_ln1): (gamma, beta) passed twice == two separate copies,
    bit for bit, guard rows of the output untouched."""
    from mmt_amd._lib import LIB, MMT_BF16, check
    g = torch.Generator().manual_seed(ns)
    dm = 512
    x_st, _ = _poisoned(torch.randn(2 * ns, dm, generator=g))
    add_st, _ = _poisoned(torch.randn(ns, dm, generator=g))
    gam, _ = _poisoned(1 + 0.1 * torch.randn(dm, generator=g))
    bet, _ = _poisoned(0.1 * torch.randn(dm, generator=g))
    gam2, bet2 = gam.clone(), bet.clone()
    outs = []
    for g1, b1 in ((gam, bet), (gam2, bet2)):
        o32 = torch.full((2 * ns + PAD, dm), NAN, device="cuda")
        o16 = torch.full((2 * ns + PAD, dm), NAN, device="cuda", dtype=torch.bfloat16)
        check(LIB.mmt_layernorm(x_st.data_ptr(), add_st.data_ptr(), ns, o32.data_ptr(), o16.data_ptr(), gam.data_ptr(),
                                bet.data_ptr(), g1.data_ptr(), b1.data_ptr(), 2 * ns, ns, dm, 1e-5, MMT_BF16,
                                torch.cuda.current_stream().cuda_stream), "mmt_layernorm")
        torch.cuda.synchronize()
        outs.append((o32, o16))
    for a, b in zip(outs[0], outs[1]):
        assert _same(a, b)
        assert bool(torch.isfinite(a[:2 * ns].float()).all()) and bool(torch.isnan(a[2 * ns:].float()).all())


@pytest.mark.parametrize("ns", [1, 400])
def test_groupnorm_same_pointer_for_both_sets(ns):
    """mmt_groupnorm over [2][ns][512] (fusion_gn at B = 1: one instance per affine set)."""
    from mmt_amd._lib import LIB, MMT_BF16, check
    g = torch.Generator().manual_seed(10 + ns)
    dm = 512
    x_st, _ = _poisoned(torch.randn(2 * ns, dm, generator=g))
    gam, _ = _poisoned(1 + 0.1 * torch.randn(dm, generator=g))
    bet, _ = _poisoned(0.1 * torch.randn(dm, generator=g))
    gam2, bet2 = gam.clone(), bet.clone()
    outs = []
    for g1, b1 in ((gam, bet), (gam2, bet2)):
        o32 = torch.full((2 * ns + PAD, dm), NAN, device="cuda")
        o16 = torch.full((2 * ns + PAD, dm), NAN, device="cuda", dtype=torch.bfloat16)
        check(LIB.mmt_groupnorm(x_st.data_ptr(), o32.data_ptr(), o16.data_ptr(), gam.data_ptr(), bet.data_ptr(),
                                g1.data_ptr(), b1.data_ptr(), 2, 1, ns, dm, 32, 1e-5, MMT_BF16,
                                torch.cuda.current_stream().cuda_stream), "mmt_groupnorm")
        torch.cuda.synchronize()
        outs.append((o32, o16))
    for a, b in zip(outs[0], outs[1]):
        assert _same(a, b)
        assert bool(torch.isfinite(a[:2 * ns].float()).all()) and bool(torch.isnan(a[2 * ns:].float()).all())


@pytest.mark.parametrize("ns", [1, 400])
def test_two_group_gemm_same_weight_pointer(ns):
    """The fusion_adjust launch at B = 1 (two groups of M = ns rows, K = 768, N = d_model = 512, bf16 -> fp32):
    (W, bias) of group 0 passed for group 1 too == a separate copy of them, bit for bit; every buffer carries PAD
    NaN rows / elements of surplus (a read of them turns the result into NaN, a write shows in the guard)."""
    from mmt_amd._lib import LIB, GemmParams, MMT_BF16, check
    g = torch.Generator().manual_seed(20 + ns)
    K, N = 768, 512
    a = [_poisoned(torch.randn(ns, K, generator=g).bfloat16())[0] for _ in range(2)]
    w, _ = _poisoned((torch.randn(N, K, generator=g) * K ** -0.5).bfloat16())
    bias, _ = _poisoned(0.1 * torch.randn(N, generator=g))
    w2, bias2 = w.clone(), bias.clone()
    sk_ws = torch.empty(8 << 20, device="cuda")
    sk_cnt = torch.zeros(1 << 16, device="cuda", dtype=torch.int32)
    outs = []
    for w1, b1 in ((w, bias), (w2, bias2)):
        c = [torch.full((ns + PAD, N), NAN, device="cuda") for _ in range(2)]
        p = GemmParams()
        for q, (wq, bq) in enumerate(((w, bias), (w1, b1))):
            p.a[q], p.w[q], p.bias[q], p.c[q] = a[q].data_ptr(), wq.data_ptr(), bq.data_ptr(), c[q].data_ptr()
        p.lda, p.ldc = K, N
        p.a_seg_rows, p.a_segs_a = ns, 1
        p.M, p.N, p.K, p.groups, p.c_f32 = ns, N, K, 2, 1
        p.sk_ws, p.sk_ws_floats, p.sk_cnt, p.sk_cnt_n = sk_ws.data_ptr(), sk_ws.numel(), sk_cnt.data_ptr(), sk_cnt.numel()
        check(LIB.mmt_gemm(ctypes.byref(p), MMT_BF16, torch.cuda.current_stream().cuda_stream), "mmt_gemm")
        torch.cuda.synchronize()
        outs.append(c)
    for q in range(2):
        assert _same(outs[0][q], outs[1][q])
        assert bool(torch.isfinite(outs[0][q][:ns]).all()) and bool(torch.isnan(outs[0][q][ns:]).all())
        ref = a[q][:ns].double().cpu() @ w[:N].double().cpu().t() + bias[:N].double().cpu()
        assert (outs[0][q][:ns].double().cpu() - ref).abs().max().item() <= 1e-4 * max(1.0, ref.abs().max().item())


# ----------------------------------------------------------------------------- G5
def _fusion_gpu(cls, seed=3):
    from mmt_amd import model as M
    torch.manual_seed(seed)
    fu = M.FUSION_CLASSES[cls](768, 512, 2, 2)
    with torch.no_grad():  # non-trivial offsets, norms and level embedding (the containers start near identity)
        for n, p in fu.named_parameters():
            if p.dim() == 1:
                p.copy_(0.1 * torch.randn_like(p) + (1.0 if n.endswith("weight") else 0.0))
        for layer in fu.fusion_attention.encoder.layers:
            layer.self_attn.sampling_offsets.weight.normal_(0, 0.02)
            layer.self_attn.sampling_offsets.bias.uniform_(-2, 2)
            layer.self_attn.attention_weights.weight.normal_(0, 0.02)
        fu.fusion_attention.level_embed.normal_()
    return fu.eval()  # dropout 0


@pytest.mark.parametrize("cls", list(CLASSES.values()))
def test_training_fusion_equals_lnspecific_twin(cls):
    """Fusion + corner head on the HIP ops, random bf16 search-token rows (2B, 400, 768), B = 2, dropout 0: the
    fused map is torch.equal to that of an LNSpecific twin carrying copies of the tied weights, and every
    parameter's gradient (the tied ones included) torch.equal to the sum of the twin's gradients the tying maps
    onto it.  The summed tail runs in the [W | W] form (train._HipLinearDup), i.e. the twin's own GEMM calls, so
    equality holds for adjust_sum / adjust_out and everything that feeds them too."""
    from mmt_amd import model as M
    from mmt_amd.train import HipOps, fusion_forward, head_forward
    fu = _fusion_gpu(cls)
    tw = _twin(fu, 768, 512).cuda()
    fu = fu.cuda()
    torch.manual_seed(1)
    head = M._head(M.hot_path_cfg()).cuda().eval()
    with torch.no_grad():
        for br in ("tl", "br"):
            getattr(head, "conv5_" + br).weight.mul_(6.0)
    g = torch.Generator().manual_seed(11)
    rows = torch.randn(4, 400, 768, generator=g).bfloat16().cuda()
    wts = torch.arange(1, 5, device="cuda", dtype=torch.float32)
    res = []
    for net in (fu, tw):
        head.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            fused = fusion_forward(net, rows, None, HipOps)
            xyxy = head_forward(head, fused, HipOps)
        (xyxy.float() * wts).sum().backward()
        torch.cuda.synchronize()
        res.append(fused.detach().float().clone())
    assert torch.equal(res[0], res[1])
    assert bool(torch.isfinite(res[0]).all()) and res[0].abs().max().item() > 0.1
    want = _tied_grads(fu, tw)
    bad = [k for k, p in fu.named_parameters() if p.grad is None or not torch.equal(p.grad, want[k])]
    assert not bad, bad
    assert all(p.grad.abs().max().item() > 0 for k, p in fu.named_parameters() if "adjust" in k or "norm" in k)


# ----------------------------------------------------------------------------- G6
def test_captured_train_step_asym_ce_add2():
    """asym_ce + Attention_Fusion_Bimodal_LNSpecific_2 (experiments/asymmetric_shared_ce/
    attention_lasher_newfusionAdd_2layer.yaml), 2 pairs: one captured TrainStep, the loss falls over five replays
    on a fixed batch (as tests/test_gpu_ce_train.py checks for LNSpecific), the tied parameters move, and every
    trainable parameter has a gradient."""
    import mmt_amd.model as M
    import mmt_amd.train as T
    torch.manual_seed(0)
    net = M.build_asymmetric_shared_ce(M.hot_path_cfg(fusion_class=CLASSES["add2"]), train=False)
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
    net.cuda()
    gen = torch.Generator().manual_seed(5)
    b0, b1 = T.synthetic_batch(2, "cuda", gen), T.synthetic_batch(2, "cuda", gen)
    static = [[x.clone() for x in z] for z in b0[:3]] + [b0[3].clone()]
    tied = [n for n, _ in net.named_parameters() if "adjust_in" in n or "adjust_out" in n]
    assert len(tied) == 8
    before = {n: p.detach().clone() for n, p in net.named_parameters() if n in tied}
    step = T.TrainStep(net, T.HipOps, lr=1e-4, ce_template_mask=T.ce_center_mask(2, 8, "cuda"), ce_keep_rate=0.7)
    step.capture(*static, warmup=1)
    losses = [float(step.replay(*b1, ce_template_mask=T.ce_center_mask(2, 8, "cuda"))["loss"]) for _ in range(5)]
    torch.cuda.synchronize()
    print("asym_ce + add2 captured step: losses of five replays %s" % ["%.5f" % x for x in losses])
    assert losses[-1] < losses[0], losses
    params = dict(net.named_parameters())
    assert all(not torch.equal(params[n].detach(), before[n]) for n in tied)
    assert not [n for n, p in params.items() if p.requires_grad and p.grad is None]


# ----------------------------------------------------------------------------- G7
def test_uni_tracker_matches_oracle():
    """lib/test/tracker/mixformer_vit_rgbt_unibackbone: three frames of tests/test_gpu_tracker.py's synthetic
    sequence, teacher-forced against the oracle's "shared" forward on the tied state dict, within that test's
    bound (1e-3 of the search crop, fp32 HIP path)."""
    from oracle import preprocess as pp
    from oracle.forward import forward as oracle_forward
    from test_gpu_tracker import _seq, _tracker
    trk, sd = _tracker("uni", "mixformer_vit_rgbt_unibackbone")
    assert trk.network.variant == "uni"
    tsd = tie_to_lnspecific(sd)
    frames, init = _seq(4)
    lut = pp.jet_lut()
    trk.initialize(frames[0], {"init_bbox": [init, init]})
    H, W = frames[0][0].shape[:2]

    def prep(im_pair, box, factor, sz):
        t = [pp.preprocess(im_pair[m], box, factor, sz, lut=lut if m == 1 else None) for m in range(2)]
        return [torch.from_numpy(x[0])[None] for x in t], t[0][2]

    tmpl, _ = prep(frames[0], init, 2.0, 128)
    online, state = list(tmpl), list(init)
    for f in range(1, 4):
        srch, rf = prep(frames[f], state, 5.0, 320)
        out, _ = oracle_forward(tsd, "shared", tmpl, online, srch)
        ref = pp.track_update(out["pred_boxes"].view(4).numpy(), state, rf, H, W, 320)
        got = trk.track(frames[f], {})["target_bbox"]
        err = max(abs(a - b) for a, b in zip(got, ref))
        print("frame %d err %.3g px (tol %.3g)" % (f, err, 1e-3 * 320 / rf))
        assert err <= 1e-3 * 320 / rf, (f, got, ref)
        state = got
        if f % 3 == 0:
            online, _ = prep(frames[f], state, 2.0, 128)
