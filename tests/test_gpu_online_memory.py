"""Online template memory in the runtime and the modules: MixFormerRGBTRuntime(online_size=K), K online
templates per sequence of which online_count[b] are filled (upstream mixformer_vit_online.py's online_size /
ONLINE_SIZES; token layout of mixformer_online.py:231-250: [template | online 0 .. online c-1 | search]).

One plan serves every fill level (the attention reads the valid template rows per sequence from device
memory), so the checks are:
  rows        at K = 3, B = 3, counts [1, 2, 3]: row b of the mixed-count run equals, bit for bit, row b of the
              run with count c_b everywhere at the same batch -- full forward, the template pass's cache rows
              [0, tl), the search pass
  exact size  the cached search pass equals bit for bit the runtime built with online_size = c, once that runtime's
              cache rows and KV1 are copied in; the full forward agrees with template + search passes and with the
              exact-size runtime within the 5e-3 tests/test_gpu_cache.py grants the cache path
  restatement fp32 boxes within the project's fp32 bound 1e-3 of a plain-PyTorch restatement in this file
              (oracle/forward.py's blocks on the token layout above, per sample with its own count)
  poison      NaN images in the absent slots change nothing
  default     online_size = 1 is today's runtime
"""
import functools
import json

import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

K, B, COUNTS = 3, 3, [1, 2, 3]
VARIANTS = ["asym_online", "shared"]
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


@functools.lru_cache(maxsize=None)
def _sd(variant):
    from mmt_amd import synthetic
    keys = json.load(open(GOLDEN + "/state_dict_%s.json" % variant))
    return {k: torch.from_numpy(v) for k, v in synthetic.synth_state_dict(keys).items()}


def _runtime(variant, dname, size=None):
    from mmt_amd.runtime import MixFormerRGBTRuntime
    kw = {} if size is None else {"online_size": size}
    return MixFormerRGBTRuntime(_sd(variant), variant, dtype=DTYPES[dname], **kw)


@functools.lru_cache(maxsize=None)
def _inputs_cpu(batch=B, slots=K):
    """t, s: [rgb, tir] (B,3,h,h); o: [rgb, tir] (B,slots,3,h,h), every slot its own image."""
    from mmt_amd import synthetic
    t, o0, s = synthetic.synth_inputs(batch)
    os_ = [o0] + [synthetic.synth_inputs(batch, seed=100 + k)[1] for k in range(1, slots)]
    o = [torch.stack([ok[m] for ok in os_], 1).contiguous() for m in range(2)]
    return t, o, s


def _cuda(xs):
    return [x.cuda() for x in xs]


def _inputs(batch=B, slots=K):
    t, o, s = _inputs_cpu(batch, slots)
    return _cuda(t), _cuda(o), _cuda(s)


def _take(o, c):
    """The first c slots, in the form a runtime of online_size c takes."""
    return [x[:, 0].contiguous() if c == 1 else x[:, :c].contiguous() for x in o]


def _score(variant):
    return variant == "asym_online"


def _fwd(rt, t, o, s, variant, **kw):
    box, sc = rt.forward(t, o, s, run_score_head=_score(variant), **kw)
    torch.cuda.synchronize()
    return box.clone(), (sc.clone() if sc is not None else None)


def _search(rt, s, variant, **kw):
    box, sc = rt.forward_search(s, run_score_head=_score(variant), **kw)
    torch.cuda.synchronize()
    return box.clone(), (sc.clone() if sc is not None else None)


def _cache_rows(rt, batch):
    ws = rt.cache_workspace(batch)
    d = rt.d
    return [q.view(d.nmod * batch, d.ntok, 3 * d.C) for q in ws["QKVL"]], ws


@pytest.mark.parametrize("dname", sorted(DTYPES))
@pytest.mark.parametrize("variant", VARIANTS)
def test_mixed_counts_equal_uniform_counts_row_by_row(variant, dname):
    rt = _runtime(variant, dname, K)
    t, o, s = _inputs()
    nt1 = rt.d.nt1
    box, sc = _fwd(rt, t, o, s, variant, online_count=COUNTS)
    rt.set_template(t, o, online_count=COUNTS)
    torch.cuda.synchronize()
    rows, ws = _cache_rows(rt, B)
    mixed_rows = [r.clone() for r in rows]
    kv1 = ws["KV1"].clone() if "KV1" in ws else None
    sbox, ssc = _search(rt, s, variant)
    assert torch.isfinite(box).all() and torch.isfinite(sbox).all()
    for b, c in enumerate(COUNTS):
        ubox, usc = _fwd(rt, t, o, s, variant, online_count=[c] * B)
        assert torch.equal(box[b], ubox[b]), (b, c, "full forward")
        rt.set_template(t, o, online_count=[c] * B)
        torch.cuda.synchronize()
        tl = (1 + c) * nt1
        for m in range(rt.d.nmod):
            for got, want in zip(mixed_rows, rows):
                assert torch.equal(got[m * B + b, :tl], want[m * B + b, :tl]), (b, c, m, "cache rows")
        usbox, ussc = _search(rt, s, variant)
        assert torch.equal(sbox[b], usbox[b]), (b, c, "search pass")
        if sc is not None:
            assert torch.equal(sc[b], usc[b]) and torch.equal(ssc[b], ussc[b]), (b, c, "scores")
            n1 = rt.d.n_kv1
            assert torch.equal(kv1[b * n1:(b + 1) * n1], ws["KV1"][b * n1:(b + 1) * n1]), (b, c, "KV1")


@pytest.mark.parametrize("c", [1, 2])
@pytest.mark.parametrize("dname", sorted(DTYPES))
@pytest.mark.parametrize("variant", VARIANTS)
def test_agrees_with_the_exact_size_runtime(variant, dname, c):
    rt, rc = _runtime(variant, dname, K), _runtime(variant, dname, None if c == 1 else c)
    assert rc.d.n_t == (1 + c) * rc.d.nt1 and rt.d.n_t == (1 + K) * rt.d.nt1
    t, o, s = _inputs()
    oc = _take(o, c)
    tl, nt = rc.d.n_t, rt.d.n_t
    # cached search pass, bit for bit, on the exact-size runtime's cache rows
    rc.set_template(t, oc)
    want_box, want_sc = _search(rc, s, variant)
    rt.set_template(t, o, online_count=[c] * B)  # sets TL (and its own rows, overwritten below)
    torch.cuda.synchronize()
    rows_k, ws_k = _cache_rows(rt, B)
    rows_c, ws_c = _cache_rows(rc, B)
    for qk, qc in zip(rows_k, rows_c):
        qk[:, :nt] = float("nan")
        qk[:, :tl] = qc[:, :tl]
    if "KV1" in ws_k:
        ws_k["KV1"].copy_(ws_c["KV1"])
    got_box, got_sc = _search(rt, s, variant)
    assert torch.equal(got_box, want_box)
    if want_sc is not None:
        assert torch.equal(got_sc, want_sc)
    # full forward against its own template + search passes and against the exact-size runtime
    full_box, full_sc = _fwd(rt, t, o, s, variant, online_count=[c] * B)
    rt.set_template(t, o, online_count=[c] * B)
    pass_box, pass_sc = _search(rt, s, variant)
    ref_box, ref_sc = _fwd(rc, t, oc, s, variant)
    errs = ((full_box - pass_box).abs().max().item(), (full_box - ref_box).abs().max().item(),
            (pass_box - want_box).abs().max().item())
    print("%s %s c=%d: full vs passes %.3g, full vs exact size %.3g, passes vs exact-size passes %.3g" % ((variant, dname, c) + errs))
    assert max(errs) <= 5e-3, errs
    if full_sc is not None:
        assert max((full_sc - pass_sc).abs().max().item(), (full_sc - ref_sc).abs().max().item()) <= 5e-3


# ---- plain-PyTorch restatement (CPU, fp32) --------------------------------------------------------------

def _restated(sd, variant, t, o, s, c, score):
    """One sample with c online templates: tokens [template | online 0 .. c-1 | search] per modality
    (mixformer_online.py:231-250: the online templates are more template tokens, x_ot.reshape(1, -1, C)), through
    oracle/forward.py's blocks with n_t = (1 + c) nt1 -- the shared MAM (template queries see template keys,
    search queries every key) or the cross-modal one (asymmetric_shared.py:55-104: search_m attends
    [template_V | template_I | search_m]) -- then the oracle's fusion, corner head and score decoder, which reads
    the first template's tokens."""
    import oracle.forward as O
    pre = "backbone."
    C, H, depth, gt, gs = O._vit_dims(sd, pre)
    nt1 = gt * gt
    n_t = (1 + c) * nt1
    x = []
    for m in range(2):
        parts = [O._patch_embed(sd, pre, t[m]) + sd[pre + "pos_embed_t"]]
        parts += [O._patch_embed(sd, pre, o[m][:, k]) + sd[pre + "pos_embed_t"] for k in range(c)]
        parts.append(O._patch_embed(sd, pre, s[m]) + sd[pre + "pos_embed_s"])
        x.append(torch.cat(parts, 1))
    x_v, x_i = x
    for i in range(depth):
        b = pre + "blocks.%d." % i
        w = (sd[b + "attn.qkv.weight"], sd[b + "attn.qkv.bias"], sd[b + "attn.proj.weight"], sd[b + "attn.proj.bias"])
        n_v, n_i = O._ln(sd, b + "norm1_v", x_v, 1e-6), O._ln(sd, b + "norm1_i", x_i, 1e-6)
        if variant == "shared":
            a_v, a_i = O.mam_attention(*w, torch.cat([n_v, n_i], 0), n_t, H).chunk(2, 0)
        else:
            a_v, a_i = O.mam_attention_asym(*w, n_v, n_i, n_t, H)
        x_v, x_i = x_v + a_v, x_i + a_i
        x_v = x_v + O._mlp(sd, b + "mlp", O._ln(sd, b + "norm2_v", x_v, 1e-6))
        x_i = x_i + O._mlp(sd, b + "mlp", O._ln(sd, b + "norm2_i", x_i, 1e-6))
    img = lambda z, a, n, g: z[:, a:a + n].transpose(1, 2).reshape(1, C, g, g).contiguous()  # noqa: E731
    fused = O.fusion_lnspecific(sd, "fusion_vi.", img(x_v, n_t, gs * gs, gs), img(x_i, n_t, gs * gs, gs))
    xyxy = O.corner_head(sd, "box_head.", fused)
    box = O.xyxy_to_cxcywh(xyxy).view(4)
    sc = None
    if score:
        templ = torch.cat([img(x_v, 0, nt1, gt), img(x_i, 0, nt1, gt)], dim=2)
        sc = O.score_decoder(sd, "score_branch.", fused, templ, xyxy.view(-1, 4), num_heads=H).view(())
    return box, sc


@pytest.mark.parametrize("variant", VARIANTS)
def test_fp32_boxes_match_the_restatement(variant):
    rt = _runtime(variant, "f32", K)
    t, o, s = _inputs_cpu()
    box, sc = _fwd(rt, _cuda(t), _cuda(o), _cuda(s), variant, online_count=COUNTS)
    sd = _sd(variant)
    with torch.no_grad():
        for b, c in enumerate(COUNTS):
            one = lambda xs: [x[b:b + 1] for x in xs]  # noqa: E731
            rbox, rsc = _restated(sd, variant, one(t), one(o), one(s), c, _score(variant))
            err = (box[b].cpu() - rbox).abs().max().item()
            print("%s sample %d count %d: box err %.3g" % (variant, b, c, err))
            assert err <= 1e-3, (b, c, err)
            if rsc is not None:
                assert abs(sc[b].item() - rsc.item()) <= 1e-3 * max(1.0, abs(rsc.item())), (b, c)


@pytest.mark.parametrize("dname", sorted(DTYPES))
@pytest.mark.parametrize("variant", VARIANTS)
def test_absent_slots_are_never_read(variant, dname):
    rt = _runtime(variant, dname, K)
    t, o, s = _inputs()
    zero, nan = [x.clone() for x in o], [x.clone() for x in o]
    for b, c in enumerate(COUNTS):
        for z, n in zip(zero, nan):
            z[b, c:] = 0
            n[b, c:] = float("nan")
    want = _fwd(rt, t, zero, s, variant, online_count=COUNTS)
    got = _fwd(rt, t, nan, s, variant, online_count=COUNTS)
    rt.set_template(t, nan, online_count=COUNTS)
    got_s = _search(rt, s, variant)
    rt.set_template(t, zero, online_count=COUNTS)
    want_s = _search(rt, s, variant)
    for g, w in ((got, want), (got_s, want_s)):
        assert torch.isfinite(g[0]).all() and torch.equal(g[0], w[0])
        if g[1] is not None:
            assert torch.isfinite(g[1]).all() and torch.equal(g[1], w[1])


@pytest.mark.parametrize("dname", sorted(DTYPES))
@pytest.mark.parametrize("variant", VARIANTS)
def test_online_size_one_is_the_default_runtime(variant, dname):
    r1, r0 = _runtime(variant, dname, 1), _runtime(variant, dname)
    t, o, s = _inputs(2, 1)
    o = _take(o, 1)
    ws = r1.workspace(2)
    assert "TL" not in ws and r1.d.n_t == r0.d.n_t and [p[2] for p in ws["plan"]] == [p[2] for p in r0.workspace(2)["plan"]]
    a, b = _fwd(r1, t, o, s, variant), _fwd(r0, t, o, s, variant)
    assert torch.equal(a[0], b[0]) and (a[1] is None or torch.equal(a[1], b[1]))
    with pytest.raises(ValueError):
        r1.forward(t, o, s, online_count=[1, 1])


def test_zero_copy_plan_and_graph_serve_every_count():
    """plan_for_inputs: one captured plan, the counts rewritten between replays."""
    rt = _runtime("asym_online", "bf16", K)
    t, o, s = _inputs()
    plan = rt.plan_for_inputs(t, o, s, run_score_head=True, online_count=[K] * B)
    g = rt.capture_plan(plan)
    ws = rt.workspace(B)
    for counts in ([1, 1, 1], COUNTS):
        rt.load_online_count(ws, counts)
        g.replay()
        torch.cuda.synchronize()
        box = ws["BOX"].clone()
        want, _ = _fwd(rt, t, o, s, "asym_online", online_count=counts)
        assert torch.equal(box, want), counts


def test_modules_take_online_count():
    from mmt_amd.model import build_asymmetric_shared_online_score, hot_path_cfg
    model = build_asymmetric_shared_online_score(hot_path_cfg(), train=False)
    model.load_state_dict(_sd("asym_online"), strict=True)
    model = model.cuda().eval().set_online_size(K)
    t, o, s = _inputs()
    rt = _runtime("asym_online", "bf16", K)
    want_box, want_sc = _fwd(rt, t, o, s, "asym_online", online_count=COUNTS)
    with torch.no_grad():
        out, _ = model(t, o, s, run_score_head=True, online_count=COUNTS)
        model.set_online(t, o, online_count=COUNTS)
        out_t, _ = model.forward_test(s, run_score_head=True)
    assert torch.equal(out["pred_boxes"].view(B, 4), want_box) and torch.equal(out["pred_scores"], want_sc)
    assert (out_t["pred_boxes"].view(B, 4) - want_box).abs().max().item() <= 5e-3


def test_packed_step_is_refused():
    rt = _runtime("shared", "bf16", K)
    with pytest.raises(NotImplementedError, match="online_size"):
        rt.slot_pack_gather(4, 2, torch.zeros(2, dtype=torch.int32, device="cuda"), ("pack", 4, 2))
