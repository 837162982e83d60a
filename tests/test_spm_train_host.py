"""Score-head training on HIP, the parts that need no GPU: the new entry points exist and validate their
arguments on the host, the public signatures, and the wiring of score_decoder_forward's `ops` branch against
the eager decoder with a plain-torch stand-in ops."""
import ctypes
import inspect

import torch
import torch.nn.functional as F

from test_capi import declared_symbols

NEW = ("mmt_spm_attention_train_fwd", "mmt_spm_attention_bwd", "mmt_spm_dq_sum", "mmt_bce_logits",
       "mmt_bce_logits_bwd")
EBADARG = -10000
FAKE = 1 << 20  # 16-B aligned, never dereferenced: every case below fails validation before a launch


def test_new_symbols_declared_bound_and_exported():
    from mmt_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    syms = declared_symbols()
    for s in NEW:
        assert s in syms, s
        assert s in _lib.EXPORTED, s
        assert hasattr(lib, s), s


def test_new_entry_points_reject_bad_arguments_on_the_host():
    from mmt_amd._lib import LIB

    def fwd(q=FAKE, kv=FAKE, out=FAKE, prob=FAKE, B=2, Lk=16, C=128, H=2, qs=128):
        return LIB.mmt_spm_attention_train_fwd(q, qs, kv, out, prob, B, Lk, C, H, 0.125, None)

    def bwd(q=FAKE, kv=FAKE, prob=FAKE, dout=FAKE, dq=FAKE, dkv=FAKE, B=2, Lk=16, C=128, H=2, qs=128):
        return LIB.mmt_spm_attention_bwd(q, qs, kv, prob, dout, dq, dkv, B, Lk, C, H, 0.125, None)

    for fn, ptrs in ((fwd, ("q", "kv", "out", "prob")), (bwd, ("q", "kv", "prob", "dout", "dq", "dkv"))):
        for name in ptrs:
            assert fn(**{name: None}) == EBADARG, (fn.__name__, name)
        assert fn(C=100) == EBADARG        # C != 64 H
        assert fn(C=128, H=3) == EBADARG
        assert fn(Lk=0) == EBADARG
        assert fn(Lk=2049) == EBADARG      # above the forward kernel's SPM_MAXK
        assert fn(B=0) == EBADARG
        assert fn(qs=64) == EBADARG        # q_stride is 0 (shared row) or C
    assert LIB.mmt_spm_dq_sum(None, FAKE, 2, 128, None) == EBADARG
    assert LIB.mmt_spm_dq_sum(FAKE, None, 2, 128, None) == EBADARG
    assert LIB.mmt_spm_dq_sum(FAKE, FAKE, 0, 128, None) == EBADARG
    for args in ((None, FAKE, 1.0, FAKE, 3), (FAKE, None, 1.0, FAKE, 3), (FAKE, FAKE, 1.0, None, 3),
                 (FAKE, FAKE, 1.0, FAKE, 0), (FAKE, FAKE, 1.0, FAKE, 65537)):
        assert LIB.mmt_bce_logits(*args, None) == EBADARG, args
    for args in ((None, FAKE, FAKE, 1.0, FAKE, 3), (FAKE, None, FAKE, 1.0, FAKE, 3), (FAKE, FAKE, None, 1.0, FAKE, 3),
                 (FAKE, FAKE, FAKE, 1.0, None, 3), (FAKE, FAKE, FAKE, 1.0, FAKE, 0),
                 (FAKE, FAKE, FAKE, 1.0, FAKE, 65537)):
        assert LIB.mmt_bce_logits_bwd(*args, None) == EBADARG, args


def test_signatures():
    from mmt_amd.train import HipOps, ScoreTrainStep, score_decoder_forward
    p = inspect.signature(ScoreTrainStep.__init__).parameters
    assert "ops" in p and p["ops"].default is None
    p = inspect.signature(score_decoder_forward).parameters
    assert list(p)[:4] == ["sb", "search_feat", "template_feat", "box_xyxy"]
    assert p["ops"].default is None
    for name in ("spm_attention", "bce_logits", "linear_cat"):
        assert hasattr(HipOps, name), name
    assert hasattr(ScoreTrainStep, "capture") and hasattr(ScoreTrainStep, "replay")


class StandInOps:
    """Plain torch, fp32: what HipOps computes, without its bf16 rounding."""

    dtype = torch.float32

    @staticmethod
    def linear(x, weight, bias, out_f32=False):
        return F.linear(x, weight, bias)

    @staticmethod
    def layer_norm(x, w0, b0, eps, w1=None, b1=None, rows0=None, out_f32=False):
        assert w1 is None
        return F.layer_norm(x, (x.shape[-1],), w0, b0, eps)

    @staticmethod
    def spm_attention(q, kv, heads, scale):
        B, Lk, C2 = kv.shape
        C = C2 // 2
        k, v = kv[..., :C].reshape(B, Lk, heads, 64), kv[..., C:].reshape(B, Lk, heads, 64)
        qh = q.expand(B, C).reshape(B, heads, 64)
        a = torch.softmax(torch.einsum("bhd,bkhd->bhk", qh, k) * scale, -1)
        return torch.einsum("bhk,bkhd->bhd", a, v).reshape(B, C)

    @staticmethod
    def bce_logits(logits, labels, weight=1.0):
        return F.binary_cross_entropy_with_logits(logits, labels.float().view(-1)) * weight


def test_ops_branch_matches_eager_decoder_on_cpu(monkeypatch):
    """C = 128, 2 heads, B = 3, a 6 x 6 search map: score_decoder_forward(..., ops=stand-in) gives the default
    path's logits and gradients to fp32 rounding (the shared-query sum over the batch rows, the k | v split, no
    residual around norm2, the zero-padded last Linear).  The RoI features come from the oracle's CPU restatement
    of PrRoIPool for both paths."""
    import mmt_amd.functional as fn
    from mmt_amd.model import ScoreDecoder
    from mmt_amd.train import score_decoder_forward
    from oracle.prroi import prroi_pool2d as prroi_cpu

    def prroi(features, rois, ph, pw, scale):
        return torch.from_numpy(prroi_cpu(features.detach().numpy(), rois.detach().numpy(), ph, pw, scale))

    monkeypatch.setattr(fn, "prroi_pool2d", prroi)
    torch.manual_seed(0)
    C, H, B = 128, 2, 3
    sb = ScoreDecoder(num_heads=H, hidden_dim=C, nlayer_head=3, pool_size=4)
    with torch.no_grad():
        sb.score_token.normal_()
        for m in sb.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.2)
    feat = torch.randn(B, C, 6, 6)
    templ = torch.randn(B, C, 2 * 3, 3)
    box = torch.tensor([[0.1, 0.2, 0.7, 0.9], [0.3, 0.1, 0.95, 0.6], [0.05, 0.05, 0.5, 0.45]])
    labels = torch.tensor([1.0, 0.0, 1.0])

    def run(ops):
        sb.zero_grad(set_to_none=True)
        logits = score_decoder_forward(sb, feat, templ, box) if ops is None else \
            score_decoder_forward(sb, feat, templ, box, ops=ops)
        F.binary_cross_entropy_with_logits(logits, labels).backward()
        return logits.detach().clone(), {n: p.grad.clone() for n, p in sb.named_parameters()}

    l0, g0 = run(None)
    l1, g1 = run(StandInOps)
    assert l0.shape == l1.shape == (B,)
    assert (l0 - l1).abs().max().item() <= 1e-5 * max(1.0, l0.abs().max().item())
    assert set(g0) == set(g1)
    gmax = max(g.norm().item() for g in g0.values())
    assert gmax > 0
    for n in g0:
        assert g0[n].shape == g1[n].shape, n
        rel = (g0[n] - g1[n]).norm().item() / max(g0[n].norm().item(), 1e-4 * gmax)
        assert rel <= 1e-4, (n, rel)
    # negative control: the comparison sees a dropped batch row of the shared query's gradient
    bad = g1["score_token"] * (B - 1) / B
    assert (g0["score_token"] - bad).norm().item() / g0["score_token"].norm().item() > 1e-2
