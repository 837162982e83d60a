"""ScoreTrainStep(net, rt, ops=HipOps): the TRAIN.TRAIN_SCORE stage with the score decoder, the loss, the clip and
AdamW on libmmt_hip.so, eager and as one hipGraph replay.  Model and inputs of
test_gpu_train_ops.py::test_score_train_step_matches_oracle_grads: the asym_online synthetic state dict, B = 3,
labels [1, 0, 1]; an fp32 and a bf16 runtime."""
import json

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

B = 3
DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module")
def state():
    from conftest import GOLDEN
    from mmt_amd import synthetic
    keys = json.load(open(GOLDEN + "/state_dict_asym_online.json"))
    sd = {k: torch.from_numpy(v) for k, v in synthetic.synth_state_dict(keys).items()}
    t, o, s = synthetic.synth_inputs(B)
    inputs = ([x.cuda() for x in t], [x.cuda() for x in o], [x.cuda() for x in s])
    return sd, inputs, torch.tensor([1.0, 0.0, 1.0], device="cuda")


@pytest.fixture(scope="module")
def runtimes(state):
    from mmt_amd.runtime import MixFormerRGBTRuntime
    cache = {}

    def get(dtype):
        if dtype not in cache:
            cache[dtype] = MixFormerRGBTRuntime(state[0], "asym_online", dtype=dtype)
        return cache[dtype]
    return get


def _net(sd):
    from mmt_amd.model import build_asymmetric_shared_online_score, hot_path_cfg
    net = build_asymmetric_shared_online_score(hot_path_cfg(), train=False)
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval()


def _score_state(step):
    """Every score parameter and both AdamW moments, cloned."""
    out = {}
    for n, p in step.net.named_parameters():
        if "score" in n:
            st = step.opt.state[p]
            out[n] = (p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone())
    return out


def _same_state(a, b):
    return [n for n in a if not all(torch.equal(x, y) for x, y in zip(a[n], b[n]))]


def _rel_errors(got, ref):
    """Relative L2 per gradient against max(its own norm, 1e-4 x the largest): the proj_k biases' gradients are
    mathematically zero (softmax is shift-invariant), rounding noise there is not a ratio."""
    gmax = max(v.norm().item() for v in ref.values())
    return {k: ((got[k].double() - ref[k].double()).norm() / max(ref[k].norm().item(), 1e-4 * gmax)).item()
            for k in ref}


@pytest.mark.parametrize("dtype", DTYPES, ids=["rt_fp32", "rt_bf16"])
def test_decoder_parity_frozen_trunk_and_learning(state, runtimes, dtype):
    """Logits and every score-branch gradient of the HIP step against autograd through the oracle's ScoreDecoder
    restatement on the CPU, fed the same trunk outputs.  The bar is test_gpu_train_ops.py's for the bf16-operand
    training path: relative L2 <= max(3e-2, 1.2 x e_torch), e_torch the error of the eager decoder under
    torch.autocast(bfloat16) on the same inputs against the same oracle.  Negative control: one weight gradient
    scaled by 0.9 fails the comparison.  Parameters without "score" in their name get no gradient and they, and
    the runtime's weight buffers, are bitwise unchanged after the steps; five steps after the first lower the
    loss."""
    from mmt_amd.train import HipOps, ScoreTrainStep, score_decoder_forward
    from oracle.forward import score_decoder
    sd, (t, o, s), labels = state
    net, rt = _net(sd), runtimes(dtype)
    step = ScoreTrainStep(net, rt, ops=HipOps)
    frozen = {n: p.detach().clone() for n, p in net.named_parameters() if "score" not in n}
    rt_w = [v for val in rt.w.values() for v in (val if isinstance(val, (tuple, list)) else (val,))
            if torch.is_tensor(v)]
    rt_sum = [(v.double().sum().item(), v.double().abs().sum().item()) for v in rt_w]
    stats = step.backward(t, o, s, labels)
    named = dict(net.named_parameters())
    for n, p in named.items():
        assert (p.grad is not None) == ("score" in n), n
    hip = {n: p.grad.detach().float().cpu() for n, p in named.items() if "score" in n}
    hip_logits = stats["scores"].float().cpu()
    # the same trunk outputs, as the eager step hands them to its decoder
    fused, templ, xyxy = ScoreTrainStep(net, rt).trunk(t, o, s)
    leaf = {k: v.detach().cpu().float().requires_grad_(True) for k, v in net.state_dict().items()
            if k.startswith("score_branch.")}
    ref_logits = score_decoder(leaf, "score_branch.", fused.cpu(), templ.cpu(), xyxy.cpu(),
                               num_heads=fused.shape[1] // 64).view(-1)
    ref_loss = F.binary_cross_entropy_with_logits(ref_logits, labels.cpu())
    ref_loss.backward()
    ref = {k: v.grad for k, v in leaf.items() if v.grad is not None}
    assert set(ref) == set(hip)
    # e_torch: the eager decoder under autocast(bf16), same inputs
    net.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        ac_logits = score_decoder_forward(net.score_branch, fused, templ, xyxy)
    F.binary_cross_entropy_with_logits(ac_logits.float(), labels).backward()
    ac = {n: p.grad.detach().float().cpu() for n, p in named.items() if "score" in n}
    net.zero_grad(set_to_none=True)
    e_hip, e_torch = _rel_errors(hip, ref), _rel_errors(ac, ref)
    ln = ref_logits.detach().norm().item()
    l_hip = ((hip_logits - ref_logits.detach()).norm() / ln).item()
    l_torch = ((ac_logits.detach().float().cpu() - ref_logits.detach()).norm() / ln).item()
    print("logits: hip %.3g autocast %.3g; loss hip %.6f oracle %.6f" % (l_hip, l_torch, stats["loss"].item(),
                                                                          ref_loss.item()))
    for k in sorted(ref):
        print("grad %-40s hip %.3g autocast %.3g" % (k, e_hip[k], e_torch[k]))
    assert l_hip <= max(3e-2, 1.2 * l_torch)
    for k in ref:
        assert e_hip[k] <= max(3e-2, 1.2 * e_torch[k]), (k, e_hip[k], e_torch[k])
    # negative control
    k = "score_branch.score_head.layers.2.weight"
    bad = dict(hip)
    bad[k] = hip[k] * 0.9
    assert _rel_errors(bad, ref)[k] > max(3e-2, 1.2 * e_torch[k])
    # learning, frozen parameters
    step.backward(t, o, s, labels)
    step.apply()
    losses = [step(t, o, s, labels)["loss"].item() for _ in range(5)]
    print("score losses", stats["loss"].item(), losses)
    assert losses[-1] < stats["loss"].item()
    for n, p in net.named_parameters():
        if "score" not in n:
            assert p.grad is None and torch.equal(p.detach(), frozen[n]), n
    assert rt_sum == [(v.double().sum().item(), v.double().abs().sum().item()) for v in rt_w]


@pytest.mark.parametrize("dtype", DTYPES, ids=["rt_fp32", "rt_bf16"])
def test_capture_replay_equals_eager_steps(state, runtimes, dtype):
    """Two equal-state copies: A runs warmup + 3 eager HIP steps on fixed inputs, B runs capture(warmup) (its
    warm-up steps are real steps; recording the graph executes nothing) and three replay()s.  Every score
    parameter and both AdamW moments are torch.equal.  replay() with new inputs equals an eager step on them from
    the same state; replay() before capture() and after a changed learning rate raise, capture() again picks
    the new value up."""
    from mmt_amd.train import HipOps, ScoreTrainStep
    sd, (t, o, s), labels = state
    rt = runtimes(dtype)
    net_a = _net(sd)
    net_b = _net(sd)
    a, b = ScoreTrainStep(net_a, rt, ops=HipOps), ScoreTrainStep(net_b, rt, ops=HipOps)
    warmup = 2
    with pytest.raises(RuntimeError):
        b.replay()
    for _ in range(warmup + 3):
        sa = a(t, o, s, labels)
    sa = {k: v.clone() for k, v in sa.items()}
    # static inputs of B's graph (replay copies new inputs into them)
    st, so, ss = [x.clone() for x in t], [x.clone() for x in o], [x.clone() for x in s]
    sl = labels.clone()
    b.capture(st, so, ss, sl, warmup=warmup)
    for _ in range(3):
        sb = b.replay()
    torch.cuda.synchronize()
    assert _same_state(_score_state(a), _score_state(b)) == []
    assert torch.equal(sa["loss"], sb["loss"]) and torch.equal(sa["scores"], sb["scores"])
    # new inputs
    t2, o2, s2 = [x.flip(0).contiguous() for x in t], [x.flip(0).contiguous() for x in o], \
        [x.flip(0).contiguous() for x in s]
    labels2 = torch.tensor([0.0, 1.0, 1.0], device="cuda")
    sa = a(t2, o2, s2, labels2)
    sb = b.replay(t2, o2, s2, labels2)
    torch.cuda.synchronize()
    assert _same_state(_score_state(a), _score_state(b)) == []
    assert torch.equal(sa["loss"], sb["loss"]) and torch.equal(sa["scores"], sb["scores"])
    assert torch.equal(st[0], t2[0]) and torch.equal(sl, labels2)
    # hyper-parameter guard
    b.opt.param_groups[0]["lr"] = 5e-5
    with pytest.raises(RuntimeError):
        b.replay()
    b.capture(st, so, ss, sl, warmup=1)
    b.replay()
    torch.cuda.synchronize()
    b.score_weight = 2.0
    with pytest.raises(RuntimeError):
        b.replay()


def test_decoder_on_hip_with_a_live_roi_memory():
    """The synthetic trunk above predicts a degenerate box, so its RoI tokens are zero and the gradients of layer 0
    (score_token, norm1, proj_q.0, proj_k.0 / proj_v.0 weights) vanish.  Here a small random decoder (C = 256, 4
    heads, B = 3, a 6 x 6 map, real boxes) runs score_decoder_forward(..., ops=HipOps) against the eager fp32 path
    on the same device: every gradient, the shared query row's (M = 1 GEMMs, the sum over the batch rows) included,
    under the same bar, e_torch being the eager path under autocast(bfloat16)."""
    from mmt_amd.model import ScoreDecoder
    from mmt_amd.train import HipOps, score_decoder_forward
    torch.manual_seed(0)
    C, H = 256, 4  # the smallest width the LayerNorm kernels take
    sb = ScoreDecoder(num_heads=H, hidden_dim=C, nlayer_head=3, pool_size=4).cuda()
    with torch.no_grad():
        sb.score_token.normal_()
        for m in sb.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.2)
    feat = torch.randn(B, C, 6, 6, device="cuda")
    templ = torch.randn(B, C, 2 * 3, 3, device="cuda")
    box = torch.tensor([[0.1, 0.2, 0.7, 0.9], [0.3, 0.1, 0.95, 0.6], [0.05, 0.05, 0.5, 0.45]], device="cuda")
    labels = torch.tensor([1.0, 0.0, 1.0], device="cuda")

    def run(ops=None, autocast=False):
        sb.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            logits = score_decoder_forward(sb, feat, templ, box) if ops is None else \
                score_decoder_forward(sb, feat, templ, box, ops=ops)
        F.binary_cross_entropy_with_logits(logits.float(), labels).backward()
        return logits.detach().float().cpu(), {n: p.grad.detach().float().cpu() for n, p in sb.named_parameters()}

    l_ref, g_ref = run()
    l_ac, g_ac = run(autocast=True)
    l_hip, g_hip = run(ops=HipOps)
    assert set(g_hip) == set(g_ref)
    e_hip, e_torch = _rel_errors(g_hip, g_ref), _rel_errors(g_ac, g_ref)
    for k in sorted(g_ref):
        print("small decoder grad %-28s hip %.3g autocast %.3g (norm %.3g)" % (k, e_hip[k], e_torch[k],
                                                                               g_ref[k].norm().item()))
    for k in ("score_token", "norm1.weight", "proj_q.0.weight", "proj_k.0.weight", "proj_v.0.weight"):
        assert g_ref[k].norm().item() > 0, k  # layer 0 is live here
    assert (l_hip - l_ref).norm().item() / l_ref.norm().item() <= max(3e-2, 1.2 * (l_ac - l_ref).norm().item()
                                                                      / l_ref.norm().item())
    for k in g_ref:
        assert e_hip[k] <= max(3e-2, 1.2 * e_torch[k]), (k, e_hip[k], e_torch[k])
