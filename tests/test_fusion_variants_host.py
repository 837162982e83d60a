"""The deformable fusion front-ends Attention_Fusion_Bimodal / _LNSpecific_Sum / _LNSpecific_2 and the
uni-backbone model on the CPU: state_dict contract, builders, the weight tying that maps each onto the
LNSpecific plan, and the training forward's aten path.  Goldens: tests/golden/make_golden_fusion.py (the
reference's own forward)."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

LNS = "Attention_Fusion_Bimodal_LNSpecific"
CLASSES = {"bimodal": "Attention_Fusion_Bimodal", "sum": LNS + "_Sum", "add2": LNS + "_2"}
# (runtime / builder variant, fusion class, layers, state_dict fixture)
CONTRACTS = [("asym", CLASSES[k], 2, "state_dict_asym_fusion_%s.json" % k) for k in CLASSES] + [
    ("uni", LNS, 2, "state_dict_uni.json")]


def tie_to_lnspecific(sd):
    """A state dict of any accepted front-end / of the uni-backbone -> the LNSpecific-shaped one that computes
    the same function (ISSUE table): a single norm serves both modalities, adjust_in both inputs, and a conv on
    out_v + out_i is [W | W] on their concat."""
    out = {}
    for k, v in sd.items():
        if ".adjust_in." in k:
            out[k.replace("adjust_in", "adjust_v")] = v
            out[k.replace("adjust_in", "adjust_i")] = v
        elif ".adjust_sum." in k or ".adjust_out." in k:
            k2 = k.replace("adjust_sum", "adjust_cat").replace("adjust_out", "adjust_cat")
            out[k2] = torch.cat([v, v], 1) if k.endswith(".0.weight") else v
        elif (".encoder.layers." in k or k.startswith("backbone.blocks.")) and (".norm1." in k or ".norm2." in k):
            n = "norm1" if ".norm1." in k else "norm2"
            out[k.replace(n + ".", n + "_v.")] = v
            out[k.replace(n + ".", n + "_i.")] = v
        else:
            out[k] = v
    return out


def _synth(keys):
    from mmt_amd import synthetic
    return {k: torch.from_numpy(v) for k, v in synthetic.synth_state_dict(keys).items()}


# ----------------------------------------------------------------------------- H1
@pytest.mark.parametrize("variant,cls,layers,fixture", CONTRACTS)
def test_state_dict_contract(variant, cls, layers, fixture):
    from mmt_amd.model import BUILDERS, hot_path_cfg, reference_state_dict_shapes
    ref = [(k, list(s)) for k, s in json.load(open(GOLDEN + "/" + fixture))]
    assert reference_state_dict_shapes(variant, fusion_layers=layers, fusion_class=cls) == ref
    model = BUILDERS[variant](hot_path_cfg(fusion_layers=layers, fusion_class=cls), train=False)
    res = model.load_state_dict(_synth(ref), strict=True)
    assert not res.missing_keys and not res.unexpected_keys


# ----------------------------------------------------------------------------- H2
def test_default_config_builds_bimodal_six_layers():
    """The reference config's default fusion (Attention_Fusion_Bimodal, 6 layers), left as default_cfg() has it.
    Only the head type is set: CORNER_UP is the one head every shipped yaml selects and the one built here."""
    from mmt_amd.config import default_cfg
    from mmt_amd.model import Attention_Fusion_Bimodal, build_mixformer_vit_rgbt
    cfg = default_cfg()
    assert (cfg.MODEL.FUSION_CLASS, cfg.MODEL.FUSION_LAYERS) == ("Attention_Fusion_Bimodal", 6)
    cfg.MODEL.HEAD_TYPE = "CORNER_UP"
    with torch.device("meta"):
        m = build_mixformer_vit_rgbt(cfg, train=False)
    assert type(m.fusion_vi) is Attention_Fusion_Bimodal
    layers = m.fusion_vi.fusion_attention.encoder.layers
    assert len(layers) == 6 and hasattr(layers[0], "norm1") and not hasattr(layers[0], "norm1_v")


@pytest.mark.parametrize("cls", list(CLASSES.values()) + [LNS])
@pytest.mark.parametrize("variant", ["rgbt", "shared", "asym", "asym_online", "asym_ce", "uni"])
def test_every_rgbt_builder_takes_every_deformable_class(variant, cls):
    from mmt_amd import model as M
    with torch.device("meta"):
        m = M.BUILDERS[variant](M.hot_path_cfg(fusion_class=cls), train=False)
    assert type(m.fusion_vi).__name__ == cls and m.variant == variant


@pytest.mark.parametrize("cls", ["Attention_Fusion_Bimodal_2", "No_Such_Fusion", "RGBT_Fusion_1", "Attention_Fusion_512"])
def test_other_fusion_classes_still_refused(cls):
    from mmt_amd.model import build_asymmetric_shared, hot_path_cfg
    with pytest.raises(NotImplementedError, match="Attention_Fusion_Bimodal_LNSpecific_Sum"):  # lists what it takes
        build_asymmetric_shared(hot_path_cfg(fusion_class=cls), train=False)


def test_lib_overlay_exports_uni():
    from lib.models.mixformer_vit_rgbt.mixformer_unibackbone import build_mixformer_vit_rgbt_uni
    from lib.test.tracker import mixformer_vit_rgbt_unibackbone as tr
    from mmt_amd import model as M
    assert build_mixformer_vit_rgbt_uni is M.build_mixformer_vit_rgbt_uni is M.BUILDERS["uni"]
    assert tr.get_tracker_class().__name__ == "MixFormer" and tr.get_batch_tracker_class().__name__ == "BatchMixFormer"


def test_uni_pretrained_loading_rule(tmp_path):
    """mixformer_unibackbone.py:448-457: RGBT_PRETRAINED_PATH holds this model's own keys; the fixed position
    tables are skipped, the rest loads (strict=False)."""
    from mmt_amd.model import build_mixformer_vit_rgbt_uni, hot_path_cfg
    cfg = hot_path_cfg(search=64, template=32)
    torch.manual_seed(0)
    src = build_mixformer_vit_rgbt_uni(cfg, train=False)
    ck = {k: v.clone() for k, v in src.state_dict().items()}
    ck["backbone.pos_embed_s"] = torch.full_like(ck["backbone.pos_embed_s"], 7.0)
    torch.save({"net": ck}, tmp_path / "uni.pth")
    cfg.MODEL.RGBT_PRETRAINED_PATH = str(tmp_path / "uni.pth")
    torch.manual_seed(1)
    dst = build_mixformer_vit_rgbt_uni(cfg, train=True)
    for k, v in dst.state_dict().items():
        if "pos_embed" in k:
            assert not (v == 7.0).any()
        else:
            assert torch.equal(v, ck[k]), k


# ----------------------------------------------------------------------------- H3
# (golden, state_dict fixture or (variant, class, layers) to take the keys from the builder, oracle variant, B)
TYING = [("model_asym_fusion_bimodal_b1", "state_dict_asym_fusion_bimodal.json", "asym", 1),
         ("model_asym_fusion_sum_b1", "state_dict_asym_fusion_sum.json", "asym", 1),
         ("model_asym_fusion_add2_b1", "state_dict_asym_fusion_add2.json", "asym", 1),
         ("model_rgbt_fusion_bimodal6_b1", ("rgbt", CLASSES["bimodal"], 6), "rgbt", 1),
         ("model_uni_b1", "state_dict_uni.json", "shared", 1), ("model_uni_b2", "state_dict_uni.json", "shared", 2)]
BOX_BAR, MAP_BAR = 4e-6, 1.5e-5  # 4x the largest measured figure: see the docstring below


@pytest.mark.parametrize("gold,keys,ovariant,B", TYING)
def test_tying_reproduces_reference(gold, keys, ovariant, B):
    """The oracle (an LNSpecific restatement, untouched) on tie_to_lnspecific(synthetic weights) against the
    reference's own forward of each front-end.  Measured (max abs box error / score-map error relative to
    max(1, |map|max)), fp32 CPU, 8 threads: bimodal 6.0e-7 / 1.8e-6, sum 2.7e-7 / 2.7e-6, add2 2.8e-7 / 2.3e-6,
    rgbt + 6-layer bimodal 2.7e-7 / 3.7e-6, uni B=1 1.2e-7 / 2.0e-6, uni B=2 9.8e-7 / 3.7e-6: no more than the
    LNSpecific oracle-vs-golden figures (2.4e-6 / 4e-5), so the [W | W] association adds nothing measurable.  The
    bars are 4x the largest of these (boxes 4 x 9.8e-7, maps 4 x 3.7e-6), far below the 1e-4 ceiling on boxes."""
    from mmt_amd import synthetic
    from mmt_amd.model import reference_state_dict_shapes
    from oracle import forward as of
    torch.set_num_threads(8)
    if isinstance(keys, tuple):
        keys = reference_state_dict_shapes(keys[0], fusion_class=keys[1], fusion_layers=keys[2])
    else:
        keys = json.load(open(GOLDEN + "/" + keys))
    sd = _synth(keys)
    g = np.load(GOLDEN + "/%s.npz" % gold)
    wsum = sum(float(v.double().abs().sum()) for v in sd.values())
    assert abs(wsum - float(g["weights_abs_sum"][0])) <= 1e-9 * wsum  # the weights the reference ran
    t, o, s = synthetic.synth_inputs(B)
    out, coord, aux = of.forward(tie_to_lnspecific(sd), ovariant, t, o, s, return_aux=True)
    berr = np.abs(out["pred_boxes"].numpy() - g["pred_boxes"]).max()
    merr = max(np.abs(aux[nm].numpy() - g[nm]).max() / max(1.0, np.abs(g[nm]).max())
               for nm in ("score_map_tl", "score_map_br"))
    print("%s: box err %.3g, rel map err %.3g" % (gold, berr, merr))
    assert berr <= BOX_BAR, berr
    assert merr <= MAP_BAR, merr


# ----------------------------------------------------------------------------- H4
CH = 64  # channels = d_model


def _restate(p, cls, in_v, in_i):
    """fusion_utils.py:192-201 / :309-318 / :344-353 with deformable_encoder.py:149-158 or
    deformable_encoder_lnspecific.py:150-160, on the parameter dict p of the module itself (no tying)."""
    from oracle import forward as of
    b, _, h, w = in_v.shape
    adj = lambda nm, x: of._gn(p, nm + ".1", of._conv1x1(p, nm + ".0", x))  # noqa: E731
    if cls == CLASSES["add2"]:
        av, ai = adj("adjust_in", in_v), adj("adjust_in", in_i)
    else:
        av, ai = adj("adjust_v", in_v), adj("adjust_i", in_i)
    d = av.shape[1]
    pos = of.sine_pos_embed(b, d, h, w).flatten(2).transpose(1, 2)
    lvl = p["fusion_attention.level_embed"]
    src = torch.cat([av.flatten(2).transpose(1, 2), ai.flatten(2).transpose(1, 2)], 1)
    lpos = torch.cat([pos + lvl[0].view(1, 1, -1), pos + lvl[1].view(1, 1, -1)], 1)
    ref = of.reference_points(h, w, b, 2)
    li = 0
    while "fusion_attention.encoder.layers.%d.linear1.weight" % li in p:
        lp = "fusion_attention.encoder.layers.%d." % li
        src = src + of.msdeform_bimodal(p, lp + "self_attn.", src + lpos, ref, src, [(h, w), (h, w)])
        for nm, ffn in (("norm1", True), ("norm2", False)):
            if cls == CLASSES["bimodal"]:
                src = of._ln(p, lp + nm, src, 1e-5)
            else:
                s_v, s_i = torch.chunk(src, 2, 1)
                src = torch.cat([of._ln(p, lp + nm + "_v", s_v, 1e-5), of._ln(p, lp + nm + "_i", s_i, 1e-5)], 1)
            if ffn:
                src = src + of._lin(p, lp + "linear2", F.relu(of._lin(p, lp + "linear1", src)))
        li += 1
    o_v, o_i = (x.permute(0, 2, 1).reshape(b, -1, h, w) for x in torch.chunk(src, 2, 1))
    if cls == CLASSES["bimodal"]:
        return adj("adjust_cat", torch.cat([o_v, o_i], 1))
    return adj("adjust_sum" if cls == CLASSES["sum"] else "adjust_out", o_v + o_i)


def _fusion(cls, layers, seed=0):
    from mmt_amd import model as M
    torch.manual_seed(seed)
    fu = M.FUSION_CLASSES[cls](CH, CH, 2, layers)
    with torch.no_grad():
        for n, p in fu.named_parameters():  # fan-in scaled weights, norm scales near 1, small biases
            if p.dim() > 1:
                p.copy_(torch.randn_like(p) * p[0].numel() ** -0.5)
            else:
                p.copy_(0.1 * torch.randn_like(p) + (1.0 if n.endswith("weight") else 0.0))
    return fu.eval()  # dropout 0


def _twin(fu, channels=CH, d_model=CH):
    """The LNSpecific module carrying copies of fu's weights by the tying table."""
    from mmt_amd import model as M
    n = len(fu.fusion_attention.encoder.layers)
    tw = M.Attention_Fusion_Bimodal_LNSpecific(channels, d_model, 2, n)
    sd = tie_to_lnspecific({"fusion_vi." + k: v.detach().clone() for k, v in fu.state_dict().items()})
    tw.load_state_dict({k[len("fusion_vi."):]: v for k, v in sd.items()}, strict=True)
    return tw.eval()


def _tied_grads(fu, tw):
    """{parameter name of fu: sum of the twin's gradients that the tying maps onto it}."""
    tg = {k: p.grad for k, p in tw.named_parameters()}
    out = {}
    for k, p in fu.named_parameters():
        if k.startswith("adjust_in."):
            out[k] = tg[k.replace("adjust_in", "adjust_v")] + tg[k.replace("adjust_in", "adjust_i")]
        elif k.startswith("adjust_sum.") or k.startswith("adjust_out."):
            g = tg["adjust_cat." + k.split(".", 1)[1]]
            out[k] = g[:, :g.shape[1] // 2] + g[:, g.shape[1] // 2:] if k.endswith(".0.weight") else g
        elif ".norm1." in k or ".norm2." in k:
            n = "norm1" if ".norm1." in k else "norm2"
            out[k] = tg[k.replace(n + ".", n + "_v.")] + tg[k.replace(n + ".", n + "_i.")]
        else:
            out[k] = tg[k]
    return out


OUT_BAR, GRAD_BAR = 1e-5, 1e-6  # see the docstring below


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("cls", list(CLASSES.values()))
def test_fusion_forward_aten_path(cls, layers):
    """train.fusion_forward with the fp32 stand-in ops of tests/test_train.py on (2, 64, 4, 4) maps: the output
    against the plain restatement above, and every parameter's gradient (the tied ones included) against the sum
    of the LNSpecific twin's gradients that the tying maps onto it.  Measured over the six cases, fp32 CPU: output
    max abs error 1.1e-6 .. 2.5e-6 at |out|max 3.3 .. 4.1 (fp32 rounding through the GroupNorms); bar 4 x 2.5e-6.
    The gradients measured exactly equal (0): module and twin run the same operations on the same values, and
    autograd's sum of the two gradients is the same single fp32 add.  Their bar is 1e-6 of the tensor's largest
    gradient (a few fp32 ulps, 1.2e-7 each), not 4 x 0, so another BLAS summation order does not fail it."""
    from mmt_amd.train import fusion_forward
    from test_train import TorchOps
    fu = _fusion(cls, layers)
    g = torch.Generator().manual_seed(3)
    s_v, s_i = torch.randn(2, CH, 4, 4, generator=g), torch.randn(2, CH, 4, 4, generator=g)
    probe = torch.randn(2, CH, 4, 4, generator=g)
    out = fusion_forward(fu, s_v, s_i, TorchOps)
    ref = _restate({k: v.detach() for k, v in fu.state_dict().items()}, cls, s_v, s_i)
    err = (out - ref).abs().max().item()
    (out * probe).sum().backward()
    tw = _twin(fu)
    (fusion_forward(tw, s_v, s_i, TorchOps) * probe).sum().backward()
    want = _tied_grads(fu, tw)
    gerr = 0.0
    for k, p in fu.named_parameters():
        assert p.grad is not None, k
        gerr = max(gerr, ((p.grad - want[k]).abs().max() / want[k].abs().max().clamp_min(1e-3)).item())
    print("%s L=%d: out err %.3g (|out| %.3g), grad rel err %.3g" % (cls, layers, err, ref.abs().max().item(), gerr))
    assert err <= OUT_BAR, err
    assert gerr <= GRAD_BAR, gerr


def test_uni_module_forward_aten_path():
    """module_forward's "uni" route (the stacked backbone on plain blocks): boxes and the backbone norms'
    gradients equal the shared model's carrying the same norm in both modality slots (boxes: same operations,
    so equal; gradients: the tied norm's is the sum of the twin's two)."""
    from mmt_amd import model as M
    from mmt_amd.train import module_forward, synthetic_batch
    from test_train import TorchOps
    torch.set_num_threads(8)
    cfg = M.hot_path_cfg(search=64, template=32)
    torch.manual_seed(0)
    uni = M.build_mixformer_vit_rgbt_uni(cfg, train=False).eval()
    sh = M.build_mixformer_vit_rgbt_shared(cfg, train=False).eval()
    with torch.no_grad():
        for br in ("tl", "br"):
            getattr(uni.box_head, "conv5_" + br).weight.mul_(30.0)
        for k, p in uni.named_parameters():
            if "norm" in k and k.startswith("backbone."):
                p.add_(0.1 * torch.randn_like(p))
    sh.load_state_dict(tie_to_lnspecific(uni.state_dict()), strict=True)
    t, o, s, _ = synthetic_batch(2, "cpu", torch.Generator().manual_seed(1), 32, 64)
    outs = []
    for net in (uni, sh):
        out, coord = module_forward(net, t, o, s, TorchOps)
        coord.square().sum().backward()
        outs.append(coord.detach())
    assert torch.equal(outs[0], outs[1])
    tg = dict(sh.named_parameters())
    for k, p in uni.named_parameters():
        if "pos_embed" in k:
            continue
        assert p.grad is not None, k
        if k.startswith("backbone.") and ".norm" in k:
            n = "norm1" if ".norm1." in k else "norm2"
            want = tg[k.replace(n + ".", n + "_v.")].grad + tg[k.replace(n + ".", n + "_i.")].grad
            assert (p.grad - want).abs().max().item() <= 1e-5 * want.abs().max().item() + 1e-12, k
