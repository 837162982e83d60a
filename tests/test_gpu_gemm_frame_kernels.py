"""The lean frame kernels of the LDS-DMA GEMM (gemm_glds.hip, gemm_glds_frame_kernel) against the general kernel.

The batch-1 frame's ViT GEMMs run on entry points of their own: qkv / fc1 (LayerNorm fold on handed-in statistics,
16-bit C, optional GELU) on the 128x128 tile and proj / fc2 (fp32 C = acc + bias + R, its 16-bit copy, the next
LayerNorm's row statistics) on the 64x64 tile with two k-groups.  impl 1 / 3 force those tile shapes and take the lean
kernel when the parameter set is one it covers; impl 10 runs the general kernel at the same tile shape.  Both must give
the same bits, and both must meet the fp32 reference at the tolerances tests/test_gpu_ops.py holds these epilogues to
(LayerNorm fold: 1e-2 of the reference magnitude; residual producer: 1e-3 of it + 1e-4, C2 the rounded C, statistics
rtol 1e-5 / atol 1e-3).

Shapes are the smallest that reach every path: two groups; M = 136 = one 128-row tile + an 8-row tail (wave rows
with all, one and no 16-row fragment below M) and M = 72 = 64 + 8 for the 64-row tile; N = 192 = a full column tile
+ a 64-column tail; K = 128 / 192 / 320 = 2 / 3 / 5 K-steps around the 4-slot ring (an odd count leaves the second
k-group of the 64x64 tile one step short), K = 256 = two steps per k-group."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
G, N = 2, 192
_cache = {}


def _lib():
    from mmt_amd import _lib
    return _lib


def _launch(p, dt, name, path=None):
    """Launches p; `path`: fields of mmt_gemm_select's answer for p that must read as given (an LDS-DMA kernel)."""
    L = _lib()
    code = L.MMT_BF16 if dt == torch.bfloat16 else L.MMT_F16
    if path is not None:
        c = L.gemm_select(p, code)
        assert c is not None and c.family == L.GEMM_LDS_DMA, (name, path)
        got = {k: getattr(c, k) for k in path}
        assert got == path, (name, got, path)
    L.check(L.LIB.mmt_gemm(p, code, torch.cuda.current_stream().cuda_stream), name)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


def _fold_case(dname, M, K):
    """Inputs and fp32 references (without / with GELU) of Linear(LayerNorm(x)), made once per shape."""
    key = ("fold", dname, M, K)
    if key not in _cache:
        dt = DT[dname]
        g = torch.Generator().manual_seed(1000 * M + K)
        x = (torch.randn(G, M, K, generator=g) * 2 + 0.7).to(dt)
        W = torch.randn(N, K, generator=g) / math.sqrt(K)
        b = torch.randn(N, generator=g)
        gam = 1 + 0.3 * torch.randn(G, K, generator=g)
        bet = 0.2 * torch.randn(G, K, generator=g)
        Wp = (W[None] * gam[:, None, :]).to(dt)
        colsum = Wp.float().sum(-1).contiguous()
        bp = (b[None] + torch.einsum("nk,gk->gn", W, bet)).contiguous()
        v = x.float().reshape(G, M, K // 64, 64)
        stats = torch.stack([v.sum(-1), (v * v).sum(-1)], -1).reshape(G, M, 2 * (K // 64)).contiguous()
        pre = torch.stack([F.layer_norm(x[q].float(), (K,), gam[q], bet[q], 1e-6) @ W.t() + b for q in range(G)])
        dev = [t.cuda() for t in (x, Wp, colsum, bp, stats)]
        _cache[key] = (dev, {0: pre, 1: F.gelu(pre)})
    return _cache[key]


# impl 1 / 3 take the lean kernel of the ViT form (FORM 0); impl 10 the general kernel at the same tile, unsplit
LEAN = {1: dict(lean=1, form=0, cfg=1, bm=128, bn=128, nsk=1), 3: dict(lean=1, form=0, cfg=3, bm=64, bn=64, nsk=1)}
GENERAL = {k: dict(v, lean=0) for k, v in LEAN.items()}


def _run_fold(dname, M, K, act, impl, cmap=None, path=None):
    (x, Wp, colsum, bp, stats), _ = _fold_case(dname, M, K)
    L = _lib()
    rows = M if cmap is None else (M // cmap[0]) * cmap[1]
    out = torch.full((G, rows, N), float("nan"), device="cuda", dtype=DT[dname])
    p = L.GemmParams()
    for q in range(G):
        p.a[q], p.w[q], p.c[q], p.bias[q] = x[q].data_ptr(), Wp[q].data_ptr(), out[q].data_ptr(), bp[q].data_ptr()
        p.ln_colsum[q], p.ln_stats_in[q] = colsum[q].data_ptr(), stats[q].data_ptr()
    p.lda, p.ldc, p.a_seg_rows, p.a_segs_a = K, N, M, 1
    p.M, p.N, p.K, p.act, p.groups, p.impl, p.ln_fold, p.ln_eps = M, N, K, act, G, impl, 2, 1e-6
    if cmap is not None:
        p.c_seg_rows, p.c_seg_pitch = cmap
    _launch(p, DT[dname], "fold", path)
    torch.cuda.synchronize()
    return out


def _res_case(dname, M, K):
    key = ("res", dname, M, K)
    if key not in _cache:
        dt = DT[dname]
        g = torch.Generator().manual_seed(1000 * M + K + 1)
        x = torch.randn(G, M, K, generator=g).to(dt)
        W = (torch.randn(G, N, K, generator=g) / math.sqrt(K)).to(dt)
        b = torch.randn(G, N, generator=g)
        R = torch.randn(G, M, N, generator=g) * 3 + 0.5
        ref = torch.einsum("gmk,gnk->gmn", x.float(), W.float()) + b[:, None, :] + R
        _cache[key] = ([t.cuda() for t in (x, W, b, R)], ref)
    return _cache[key]


def _run_res(dname, M, K, impl, sk=None, path=None):
    (x, W, b, R), _ = _res_case(dname, M, K)
    L = _lib()
    c1 = torch.full((G, M, N), float("nan"), device="cuda")
    c2 = torch.full((G, M, N), float("nan"), device="cuda", dtype=DT[dname])
    st = torch.full((G, M, 2 * (N // 64)), float("nan"), device="cuda")
    p = L.GemmParams()
    for q in range(G):
        p.a[q], p.w[q], p.c[q], p.c2[q] = x[q].data_ptr(), W[q].data_ptr(), c1[q].data_ptr(), c2[q].data_ptr()
        p.bias[q], p.r[q], p.ln_stats_out[q] = b[q].data_ptr(), R[q].data_ptr(), st[q].data_ptr()
    p.lda, p.ldc, p.ldr, p.a_seg_rows, p.a_segs_a = K, N, N, M, 1
    p.M, p.N, p.K, p.c_f32, p.groups, p.impl, p.c2_copy = M, N, K, 1, G, impl, 1
    if sk is not None:
        n, ws, cnt = sk
        p.splitk, p.sk_ws, p.sk_ws_floats, p.sk_cnt, p.sk_cnt_n = n, ws.data_ptr(), ws.numel(), cnt.data_ptr(), cnt.numel()
    _launch(p, DT[dname], "res", path)
    torch.cuda.synchronize()
    return c1, c2, st


def _check_res(dname, M, K, outs, tag):
    _, ref = _res_case(dname, M, K)
    c1, c2, st = [t.cpu() for t in outs]
    err, lim = (c1 - ref).abs().max().item(), 1e-3 * ref.abs().max().item() + 1e-4
    print("%s: C err %.3g (limit %.3g)" % (tag, err, lim))
    assert err <= lim, (tag, err, lim)
    assert torch.equal(c2, c1.to(DT[dname])), tag
    v = c2.float().reshape(G, M, N // 64, 64)
    ref_st = torch.stack([v.sum(-1), (v * v).sum(-1)], -1).reshape(G, M, -1)
    print("%s: statistics err %.3g" % (tag, (st - ref_st).abs().max().item()))
    assert torch.allclose(st, ref_st, rtol=1e-5, atol=1e-3), (tag, (st - ref_st).abs().max())


@pytest.mark.parametrize("dname", ["bf16", "fp16"])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("K", [128, 192, 320])
@pytest.mark.parametrize("M", [136, 72])
def test_fold_kernel_bitwise_and_reference(dname, act, K, M):
    """qkv / fc1 form on the 128x128 tile: lean (impl 1) == general (impl 10) bit for bit; both near fp32."""
    lean = _run_fold(dname, M, K, act, 1, path=LEAN[1])
    gen = _run_fold(dname, M, K, act, 10, path=GENERAL[1])
    assert torch.equal(_bits(lean), _bits(gen))
    ref = _fold_case(dname, M, K)[1][act]
    err, lim = (lean.float().cpu() - ref).abs().max().item(), 1e-2 * ref.abs().max().item()
    print("fold %s M %d K %d act %d: err %.3g (limit %.3g)" % (dname, M, K, act, err, lim))
    assert err <= lim, (err, lim)


@pytest.mark.parametrize("dname", ["bf16", "fp16"])
@pytest.mark.parametrize("K", [128, 192, 256, 320])
@pytest.mark.parametrize("M", [72, 136])
def test_residual_kernel_bitwise_and_reference(dname, K, M):
    """proj / fc2 form on the 64x64 two-k-group tile: C, C2 and the statistics, lean (impl 3) == general (impl 10)."""
    lean = _run_res(dname, M, K, 3, path=LEAN[3])
    gen = _run_res(dname, M, K, 10, path=GENERAL[3])
    for a, b in zip(lean, gen):
        assert torch.equal(_bits(a), _bits(b))
    _check_res(dname, M, K, lean, "residual %s M %d K %d" % (dname, M, K))


def test_auto_choice_matches_general_kernel():
    """impl 0 (the frame plan's setting) against impl 10 on parameter sets whose auto tile is the lean kernel's."""
    M, K = 72, 256  # the cost model takes 64x64 for so few tiles
    for a, b in zip(_run_res("bf16", M, K, 0, path=LEAN[3]), _run_res("bf16", M, K, 10, path=GENERAL[3])):
        assert torch.equal(_bits(a), _bits(b))


def test_repeat_launch_same_bits():
    for impl in (1, 10):
        a, b = _run_fold("bf16", 136, 320, 1, impl), _run_fold("bf16", 136, 320, 1, impl)
        assert torch.equal(_bits(a), _bits(b))
    for impl in (3, 10):
        for a, b in zip(_run_res("bf16", 136, 320, impl), _run_res("bf16", 136, 320, impl)):
            assert torch.equal(_bits(a), _bits(b))


def test_fallback_row_map():
    """An output row map (the template K/V cache passes' qkv) is not a lean parameter set: the general kernel runs
    under impl 0 as under impl 10 (a lean kernel would ignore the map), and the rows land where the map puts them."""
    M, K, seg, pitch = 136, 192, 68, 80
    a = _run_fold("bf16", M, K, 0, 0, cmap=(seg, pitch), path=dict(lean=0))
    b = _run_fold("bf16", M, K, 0, 10, cmap=(seg, pitch), path=dict(lean=0))
    assert torch.equal(_bits(a), _bits(b))
    ref = _fold_case("bf16", M, K)[1][0]
    got = a.float().cpu().reshape(G, M // seg, pitch, N)
    assert torch.isnan(got[:, :, seg:]).all()  # the rows between segments stay untouched
    got = got[:, :, :seg].reshape(G, M, N)
    assert (got - ref).abs().max().item() <= 1e-2 * ref.abs().max().item()
    # on the lean kernel's tile shape (impl 1: the map keeps it on the general kernel) the mapped rows hold the bits of
    # the plain launch (impl 10: the general kernel at 128x128 too)
    got1 = _run_fold("bf16", M, K, 0, 1, cmap=(seg, pitch), path=dict(lean=0, cfg=1)).float().cpu().reshape(G, M // seg, pitch, N)
    assert torch.isnan(got1[:, :, seg:]).all()
    assert torch.equal(got1[:, :, :seg].reshape(G, M, N), _run_fold("bf16", M, K, 0, 10).float().cpu())


def test_fallback_split_k():
    """A forced K split keeps the general kernel and its hand-off (impl 0 as impl 10), tickets left at zero."""
    M, K = 136, 320
    ws = torch.empty(1 << 20, device="cuda")
    cnt = torch.zeros(1 << 12, device="cuda", dtype=torch.int32)
    a = _run_res("bf16", M, K, 0, sk=(2, ws, cnt), path=dict(lean=0, nsk=2))
    b = _run_res("bf16", M, K, 10, sk=(2, ws, cnt), path=dict(lean=0, nsk=2))
    for u, v in zip(a, b):
        assert torch.equal(_bits(u), _bits(v))
    _check_res("bf16", M, K, a, "split-K")
    assert int(cnt.abs().sum()) == 0


def test_fallback_k_tail():
    """K = 2 x 64 + 24 (three 8-element chunks past the last full step): the general kernel's zero-filled tail."""
    M, K = 136, 152
    a, b = _run_res("bf16", M, K, 0, path=dict(lean=0)), _run_res("bf16", M, K, 10, path=dict(lean=0))
    for u, v in zip(a, b):
        assert torch.equal(_bits(u), _bits(v))
    _check_res("bf16", M, K, a, "K tail")


def test_fallback_conv():
    """Conv mode (implicit im2col) with the compact bias + ReLU epilogue: same bits under impl 0 and impl 10."""
    L = _lib()
    B, h, cin, cout = 2, 12, 64, 64
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, cin, h, h, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)
    b = torch.randn(cout, generator=g)
    xin = x.permute(0, 2, 3, 1).contiguous().bfloat16().cuda()
    wk = w.permute(0, 2, 3, 1).reshape(cout, 9 * cin).contiguous().bfloat16().cuda()
    bd = b.cuda()
    outs = []
    for impl in (0, 10):
        out = torch.full((B * h * h, cout), float("nan"), device="cuda", dtype=torch.bfloat16)
        p = L.GemmParams()
        p.a[0], p.w[0], p.c[0], p.bias[0] = xin.data_ptr(), wk.data_ptr(), out.data_ptr(), bd.data_ptr()
        p.lda, p.ldc = cin, cout
        p.M, p.N, p.K, p.act, p.groups, p.impl = B * h * h, cout, 9 * cin, 2, 1, impl
        p.conv_h, p.conv_up, p.conv_cin, p.conv_k3 = h, 1, cin, 1
        _launch(p, torch.bfloat16, "conv", dict(lean=0, conv=1))
        torch.cuda.synchronize()
        outs.append(out)
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    ref = F.relu(F.conv2d(x.bfloat16().float(), w.bfloat16().float(), b, padding=1))
    got = outs[0].float().cpu().reshape(B, h, h, cout).permute(0, 3, 1, 2)
    assert (got - ref).abs().max().item() <= 2e-2 * ref.abs().max().item()
