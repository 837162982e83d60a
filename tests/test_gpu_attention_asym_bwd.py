"""The cross-modal (asym = 1) MAM attention backward against probes that account for every query of every key
(tests/attn_asym_bwd_probes.py), at attn_probes' tile-edge shapes with 2 BM = 4 sequences.

Each test runs the training forward (bf16, lse) at asym = 1 and then mmt_mam_attention_bwd into a dqkv that was
filled with NaN.  Bars, from the arithmetic (test_attn_asym_bwd_host.py asserts the margins):
  census   dV within 2^-7 |ref| (P = 1 / n rounded once to bf16, the sum rounded once); every single attending
           (sequence, query) weighs >= 5.4x that, and the weights differ between sequences, so a query group that is
           dropped, doubled, cut short or read from the wrong sequence cannot hide.  dK exactly 0 (q' = 0).  dQ within
           2^-7 scale sum_k A_qk |k_k| elementwise.  No NaN left: every row of every sequence is written in all three
           column blocks.
  random   per-row relative error (attn_probes.row_rel_err) against fp64 within 4x the worst row of the CPU
           emulation of the documented arithmetic: emulation dQ 8.23e-3, dK 1.083e-2, dV 8.13e-3 -> bars 3.29e-2,
           4.33e-2, 3.25e-2 (attn_asym_bwd_probes.ASYM_BWD_ROW_BAR)."""
import pytest
import torch

import attn_asym_bwd_probes as A
import attn_probes as P
from attn_probes import BM, HEADS, SHAPES

pytestmark = pytest.mark.gpu

S, H, C = A.S, HEADS, 64 * HEADS
IMPLS = [0, 8, 21]


def _lib():
    from mmt_amd import _lib
    return _lib


def _first(bad, got, ref, what):
    i = tuple(bad.nonzero()[0].tolist())
    return "%s: %d elements over the bar, first at %s: got %.9g, reference %.9g" % (
        what, int(bad.sum()), i, got[i].item(), ref[i].item())


def _bwd_params(qd, out, dd, lse, delta, dqkv, n_t, nseq, Bm):
    L = _lib()
    b = L.AttnBwdParams()
    b.qkv, b.out, b.dout, b.lse, b.delta, b.dqkv = qd.data_ptr(), out.data_ptr(), dd.data_ptr(), lse.data_ptr(), \
        delta.data_ptr(), dqkv.data_ptr()
    b.S, b.Bm, b.ntok, b.n_t, b.C, b.H, b.asym, b.scale = nseq, Bm, qd.shape[1], n_t, C, H, 1, P.SCALE
    return b


def _fwd(qd, n_t, impl):
    """The training forward (lse) at asym = 1 on qd [S][ntok][3C] bf16 (device)."""
    L = _lib()
    ntok = qd.shape[1]
    out = torch.empty(S, ntok, C, device="cuda", dtype=torch.bfloat16)
    lse = torch.full((S, H, ntok), float("nan"), device="cuda")
    p = L.AttnParams()
    p.qkv, p.out, p.S, p.Bm, p.ntok, p.n_t, p.C, p.H, p.asym = qd.data_ptr(), out.data_ptr(), S, BM, ntok, n_t, C, H, 1
    p.scale, p.impl, p.lse = P.SCALE, impl, lse.data_ptr()
    L.check(L.LIB.mmt_mam_attention(p, L.MMT_BF16, torch.cuda.current_stream().cuda_stream), "attn")
    return out, lse


def _fwd_bwd(qkv, dout, n_t, impl, calls=1):
    """Forward and `calls` backward calls on the S sequences; returns the dqkv of each call (device, bf16)."""
    L = _lib()
    qd, dd = qkv.bfloat16().cuda(), dout.bfloat16().cuda()
    out, lse = _fwd(qd, n_t, impl)
    res = []
    for _ in range(calls):
        delta = torch.empty(S, H, qd.shape[1], device="cuda")
        dqkv = torch.full(qd.shape, float("nan"), device="cuda", dtype=torch.bfloat16)
        b = _bwd_params(qd, out, dd, lse, delta, dqkv, n_t, S, BM)
        L.check(L.LIB.mmt_mam_attention_bwd(b, L.MMT_BF16, torch.cuda.current_stream().cuda_stream), "attn bwd")
        torch.cuda.synchronize()
        res.append(dqkv)
    return res


@pytest.mark.parametrize("n_t,n_s", SHAPES)
@pytest.mark.parametrize("impl", IMPLS)
def test_backward_census(impl, n_t, n_s):
    """dV counts the attending (sequence, query) pairs of every key, dK is exactly zero, dQ stays inside its
    elementwise rounding bound, and no element of dqkv is left unwritten."""
    qkv, dout, ref, bound = A.census_case(n_t, n_s)
    got = _fwd_bwd(qkv, dout, n_t, impl)[0].double().cpu()
    assert not got.isnan().any(), _first(got.isnan(), got, ref, "unwritten")
    gq, gk, gv = got.split(C, -1)
    rq, _, rv = ref.split(C, -1)
    bad = ~((gv - rv).abs() <= 2.0 ** -7 * rv.abs())
    assert not bad.any(), _first(bad, gv, rv, "dV")
    assert bool((gk == 0).all()), _first(gk != 0, gk, torch.zeros_like(gk), "dK")
    bad = ~((gq - rq).abs() <= bound)
    assert not bad.any(), _first(bad, gq, rq, "dQ")


@pytest.mark.parametrize("n_t,n_s", P.BWD_RANDOM_SHAPES)
@pytest.mark.parametrize("impl", IMPLS)
def test_backward_random_rows(impl, n_t, n_s):
    """N(0, 1) inputs, the error taken per token row relative to that row's largest reference gradient."""
    qkv, dout, ref, _ = A.random_ref(n_t, n_s)
    got = _fwd_bwd(qkv, dout, n_t, impl)[0].double().cpu()
    err = P.row_rel_err(got, ref, C).tolist()
    print("per-row rel err dQ %.3g dK %.3g dV %.3g" % tuple(err))
    for nm, e, bar in zip("qkv", err, A.ASYM_BWD_ROW_BAR):
        assert e <= bar, (nm, e, bar)


@pytest.mark.parametrize("n_t,n_s", [(49, 64), (64, 193)])
def test_backward_is_deterministic(n_t, n_s):
    qkv, dout, _, _ = A.random_ref(n_t, n_s)
    a, b = _fwd_bwd(qkv, dout, n_t, 0, calls=2)
    assert torch.equal(a, b)


def test_backward_arguments():
    """asym = 1 needs S == 2 Bm: anything else is rejected before a launch (the buffers are valid either way)."""
    L = _lib()
    n_t, n_s = 32, 48
    qkv, dout = A.random_case(n_t, n_s)
    qd, dd = qkv.bfloat16().cuda(), dout.bfloat16().cuda()
    out, lse = _fwd(qd, n_t, 0)
    delta = torch.empty(S, H, n_t + n_s, device="cuda")
    dqkv = torch.full(qd.shape, float("nan"), device="cuda", dtype=torch.bfloat16)
    st = torch.cuda.current_stream().cuda_stream
    for nseq, Bm in ((S, 1), (S - 1, 1), (S, 0)):
        assert L.LIB.mmt_mam_attention_bwd(_bwd_params(qd, out, dd, lse, delta, dqkv, n_t, nseq, Bm), L.MMT_BF16, st) < 0
    torch.cuda.synchronize()
    assert bool(dqkv.isnan().all())  # nothing was launched
    assert L.LIB.mmt_mam_attention_bwd(_bwd_params(qd, out, dd, lse, delta, dqkv, n_t, S, BM), L.MMT_BF16, st) == 0
    torch.cuda.synchronize()
    assert not dqkv.isnan().any()


def test_op_native_and_composed():
    """HipOps.mam_attention_asym (the native op pair) and the composed form it replaces, under autograd with the
    same dout: both forwards within the project's bf16 bar of fp64, both dqkv within the random-row bars."""
    from mmt_amd import train
    from mmt_amd.train import HipOps, asym_attention_from_mam
    n_t, n_s = 64, 193
    qkv, dout, ref, _ = A.random_ref(n_t, n_s)
    out_ref, _ = P.mam_ref(qkv, n_t, BM, H, 1)
    assert train.ASYM_NATIVE
    forms = {"native": lambda x: HipOps.mam_attention_asym(x, BM, n_t, H),
             "composed": lambda x: asym_attention_from_mam(HipOps.mam_attention, x, BM, n_t, H)}
    for name, fn in forms.items():
        x = qkv.bfloat16().cuda().requires_grad_()
        out = fn(x)
        out.backward(dout.bfloat16().cuda())
        ferr = (out.detach().double().cpu() - out_ref).abs().max().item()
        err = P.row_rel_err(x.grad.double().cpu(), ref, C).tolist()
        print("%s: forward max err %.3g, per-row rel err dQ %.3g dK %.3g dV %.3g" % ((name, ferr) + tuple(err)))
        assert ferr <= 1.5e-2, (name, ferr)
        for nm, e, bar in zip("qkv", err, A.ASYM_BWD_ROW_BAR):
            assert e <= bar, (name, nm, e, bar)


def test_opcheck_mam_attention_asym():
    import mmt_amd.ops  # noqa: F401
    g = torch.Generator().manual_seed(2)
    qkv = torch.randn(4, 100, 3 * 128, generator=g).bfloat16().cuda()
    torch.library.opcheck(torch.ops.mmt.mam_attention_asym_forward.default, (qkv.clone().requires_grad_(True), 2, 36, 2))
    out, lse = torch.ops.mmt.mam_attention_asym_forward(qkv, 2, 36, 2)
    dout = torch.randn(4, 100, 128, generator=g).bfloat16().cuda()
    torch.library.opcheck(torch.ops.mmt.mam_attention_asym_backward.default, (qkv, out, dout, lse, 2, 36, 2))
