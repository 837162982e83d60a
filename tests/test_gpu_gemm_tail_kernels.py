"""The lean entry points of the frame's other GEMM-mode launches (gemm_glds.hip, the LEAN_PLAIN forms of
gemm_glds_frame_kernel and gemm_glds_frame_multi_kernel) against the general kernels.

Forms: fp32 C = acc + bias (+ R) with A from one pointer or two, 16-bit C = acc + bias, all on the 64x64 tile with two
k-groups (impl 3); 16-bit C = relu(acc + bias) on the 128x64 tile (impl 2).  The forced tile shape takes the lean
kernel when the parameter set is one it covers; impl 10 runs the general kernel at the same tile shape.  Both must give
the same bits, leave everything past M rows / N columns untouched, and meet the fp32 reference at the tolerances
tests/test_gpu_ops.py holds these epilogues to (fp32 producers: 1e-3 of the reference magnitude + 1e-4; 16-bit C: 1e-2
of it).

Shapes are the smallest that reach every path: one and two groups; M = 72 = 64 + 8 for the 64-row tile, M = 136 = 128
+ 8 for the 128-row tile; N = 72 = one full 64-column tile + an 8-column tail; K = 128 / 192 / 320 = 2 / 3 / 5 K-steps
around the 4-slot ring (an odd count leaves the second k-group one step short) and K = 256.  The outputs have 8 rows
past M and 8 columns past N (ldc = N + 8), NaN like the rest before the launch."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
N, PAD = 72, 8
KS = [128, 192, 256, 320]
_cache = {}


def _lib():
    from mmt_amd import _lib
    return _lib


def _code(dt):
    L = _lib()
    return L.MMT_BF16 if dt == torch.bfloat16 else L.MMT_F16


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


def _case(dname, G, M, K):
    """Inputs of one shape, made once: A (and a second generator's A1 for the two-pointer cases), W, bias, R."""
    key = (dname, G, M, K)
    if key not in _cache:
        dt = DT[dname]
        g = torch.Generator().manual_seed(100000 * G + 1000 * M + K)
        g1 = torch.Generator().manual_seed(7 + 100000 * G + 1000 * M + K)
        x = torch.randn(G, M, K, generator=g).to(dt)
        x1 = (torch.rand(G, M, K, generator=g1) * 4 - 1).to(dt)  # the second half's source: another distribution
        W = (torch.randn(G, N, K, generator=g) / math.sqrt(K)).to(dt)
        b = torch.randn(G, N, generator=g)
        R = torch.randn(G, M + PAD, N, generator=g) * 3 + 0.5
        _cache[key] = {k: v.cuda() for k, v in dict(x=x, x1=x1, W=W, b=b, R=R).items()}
    return _cache[key]


def _ref(dname, G, M, K, *, f32, act=0, bias=True, r=False, r_p0=None, k_split=0):
    """fp32 reference on the CPU, made once per parameter set."""
    key = ("ref", dname, G, M, K, f32, act, bias, r, r_p0, k_split)
    if key not in _cache:
        t = {k: v.float().cpu() for k, v in _case(dname, G, M, K).items()}
        A = t["x"] if not k_split else torch.cat([t["x"][..., :k_split], t["x1"][..., :K - k_split]], -1)
        v = torch.einsum("gmk,gnk->gmn", A, t["W"])
        if bias:
            v = v + t["b"][:, None, :]
        if act == 2:
            v = v.relu()
        if r:
            rows = torch.arange(M) % (r_p0 if r_p0 else M + PAD)
            v = v + t["R"][:, rows]
        _cache[key] = v
    return _cache[key]


def _params(dname, G, M, K, impl, out, *, f32, act=0, bias=True, r=False, r_mode=0, r_p0=0, k_split=0, cmap=None, sk=None):
    L = _lib()
    t = _case(dname, G, M, K)
    p = L.GemmParams()
    for q in range(G):
        p.a[q], p.w[q], p.c[q] = t["x"][q].data_ptr(), t["W"][q].data_ptr(), out[q].data_ptr()
        if bias:
            p.bias[q] = t["b"][q].data_ptr()
        if r:
            p.r[q] = t["R"][q].data_ptr()
        if k_split:
            p.a1[q] = t["x1"][q].data_ptr()
    p.lda, p.ldc, p.ldr, p.a_seg_rows, p.a_segs_a = K, N + PAD, N, M, 1
    p.M, p.N, p.K, p.act, p.c_f32, p.groups, p.impl, p.k_split = M, N, K, act, int(f32), G, impl, k_split
    p.r_mode, p.r_p0, p.r_p1 = r_mode, r_p0, 1
    if cmap is not None:
        p.c_seg_rows, p.c_seg_pitch = cmap
    if sk is not None:
        n, ws, cnt = sk
        p.splitk, p.sk_ws, p.sk_ws_floats, p.sk_cnt, p.sk_cnt_n = n, ws.data_ptr(), ws.numel(), cnt.data_ptr(), cnt.numel()
    return p


TILE = {1: (128, 128), 2: (128, 64), 3: (64, 64)}
PL, LR, A2 = 1, 2, 4  # the lean FORM bits: plain, R added, A from two pointers


def _path(p, dname, want, n=1):
    """What mmt_gemm_select says the launch of p (n > 1: of the array p through mmt_gemm_multi) runs: the fields of
    `want` must read as given (an LDS-DMA kernel in every case of this file)."""
    L = _lib()
    c = L.gemm_select(p, _code(DT[dname]), n)
    assert c is not None and c.family == L.GEMM_LDS_DMA, want
    got = {k: getattr(c, k) for k in want}
    assert got == want, (got, want)


def _out(dname, G, rows, f32):
    return torch.full((G, rows + PAD, N + PAD), float("nan"), device="cuda", dtype=torch.float32 if f32 else DT[dname])


def _run(dname, G, M, K, impl, *, f32, rows=None, path=None, **kw):
    L = _lib()
    out = _out(dname, G, M if rows is None else rows, f32)
    p = _params(dname, G, M, K, impl, out, f32=f32, **kw)
    if path is not None:
        _path(p, dname, path)
    L.check(L.LIB.mmt_gemm(p, _code(DT[dname]), torch.cuda.current_stream().cuda_stream), "tail gemm")
    torch.cuda.synchronize()
    return out


def _check(out, ref, f32, tag, rows=None):
    """Sentinels untouched, the M x N block within the form's tolerance of the fp32 reference."""
    M = ref.shape[1] if rows is None else rows
    got = out.float().cpu()
    assert torch.isnan(got[:, M:]).all() and torch.isnan(got[:, :, N:]).all(), tag
    if rows is None:
        err = (got[:, :M, :N] - ref).abs().max().item()
        lim = 1e-3 * ref.abs().max().item() + 1e-4 if f32 else 1e-2 * ref.abs().max().item()
        print("%s: err %.3g (limit %.3g)" % (tag, err, lim))
        assert err <= lim, (tag, err, lim)


def _pair(dname, G, M, K, impl, *, f32, **kw):
    """The lean path (forced tile shape) and impl 10: same bits, sentinels, reference.  The selection says that the
    first is the lean kernel of the expected form and the second the general kernel at the same tile, unsplit."""
    form = PL | (LR if kw.get("r") else 0) | (A2 if kw.get("k_split") else 0)
    tile = dict(cfg=impl, bm=TILE[impl][0], bn=TILE[impl][1], nsk=1)
    lean = _run(dname, G, M, K, impl, f32=f32, path=dict(tile, lean=1, form=form), **kw)
    gen = _run(dname, G, M, K, 10, f32=f32, path=dict(tile, lean=0, form=0), **kw)
    assert torch.equal(_bits(lean), _bits(gen))
    rk = {k: kw[k] for k in ("act", "bias", "r", "k_split") if k in kw}
    if kw.get("r_mode") == 1:
        rk["r_p0"] = kw["r_p0"]
    ref = _ref(dname, G, M, K, f32=f32, **rk)
    _check(lean, ref, f32, "%s G %d M %d K %d %s" % (dname, G, M, K, kw))
    return lean


@pytest.mark.parametrize("dname", ["bf16", "fp16"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("r", [False, True])
def test_f32_form_bitwise_and_reference(dname, K, G, r):
    """fp32 C = acc + bias (+ R): fusion_adjust / enc_outproj, with R enc_linear2; 64x64 tile."""
    _pair(dname, G, 72, K, 3, f32=True, r=r)


@pytest.mark.parametrize("dname", ["bf16", "fp16"])
@pytest.mark.parametrize("K,k_split", [(128, 64), (192, 64), (192, 128)])
@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("r", [False, True])
def test_f32_two_pointer_form_bitwise_and_reference(dname, K, k_split, G, r):
    """The same with A from two pointers (fusion_adjust_cat, the offsets Linear): the boundary on (128 of 192: k-group
    0 takes steps 0 and 2) and off (64) the k-group boundary; the halves come from different generators."""
    _pair(dname, G, 72, K, 3, f32=True, r=r, k_split=k_split)


@pytest.mark.parametrize("dname", ["bf16", "fp16"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("G", [1, 2])
def test_c16_form_bitwise_and_reference(dname, K, G):
    """16-bit C = acc + bias (the value Linear), 64x64 tile."""
    _pair(dname, G, 72, K, 3, f32=False)


@pytest.mark.parametrize("dname", ["bf16", "fp16"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("G", [1, 2])
def test_c16_relu_form_bitwise_and_reference(dname, K, G):
    """16-bit C = relu(acc + bias) (enc_linear1), 128x64 tile with two k-groups."""
    _pair(dname, G, 136, K, 2, f32=False, act=2)


def test_auto_choice_matches_general_kernel():
    """impl 0 (the frame plan's setting) on shapes whose auto tile is the lean kernel's (64x64 for so few tiles)."""
    for kw in (dict(f32=True, r=True), dict(f32=True, k_split=128), dict(f32=False)):
        a = _run("bf16", 2, 72, 256, 0, path=dict(lean=1, cfg=3), **kw)
        b = _run("bf16", 2, 72, 256, 10, path=dict(lean=0, cfg=3, nsk=1), **kw)
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("r_p0", [72, 80])
def test_edge_identity_row_map_inside(r_p0):
    """r_mode 1 with r_p0 = M and M + 8 is the identity map: the bits of r_mode 0, lean as impl 10."""
    mapped = _pair("bf16", 2, 72, 192, 3, f32=True, r=True, r_mode=1, r_p0=r_p0)
    plain = _run("bf16", 2, 72, 192, 3, f32=True, r=True)
    assert torch.equal(_bits(mapped), _bits(plain))


def test_edge_row_map_wraps_outside():
    """r_p0 = M / 2: rows wrap, the general kernel runs and matches a reference that wraps."""
    out = _run("bf16", 2, 72, 192, 3, f32=True, r=True, r_mode=1, r_p0=36, path=dict(lean=0, cfg=3, epi=0))
    _check(out, _ref("bf16", 2, 72, 192, f32=True, r=True, r_p0=36), True, "r_p0 36")
    assert not torch.equal(_bits(out), _bits(_run("bf16", 2, 72, 192, 3, f32=True, r=True)))


def test_edge_k_split():
    """k_split = 64 is a lean parameter set, 72 (inside a K-step) is not; both meet their references."""
    _pair("bf16", 2, 72, 192, 3, f32=True, k_split=64)
    out = _run("bf16", 2, 72, 192, 3, f32=True, k_split=72, path=dict(lean=0, cfg=3))
    _check(out, _ref("bf16", 2, 72, 192, f32=True, k_split=72), True, "k_split 72")


def test_edge_bias():
    """With the bias lean, without it the general kernel."""
    _pair("bf16", 2, 72, 192, 3, f32=True, bias=True)
    out = _run("bf16", 2, 72, 192, 3, f32=True, bias=False, path=dict(lean=0, cfg=3))
    _check(out, _ref("bf16", 2, 72, 192, f32=True, bias=False), True, "no bias")
    out = _run("bf16", 2, 72, 192, 3, f32=False, bias=False, path=dict(lean=0, cfg=3))
    _check(out, _ref("bf16", 2, 72, 192, f32=False, bias=False), False, "no bias, 16-bit C")


def test_edge_output_row_map():
    """An output row map keeps the general kernel (a lean kernel would ignore it): two segments of 36 rows at pitch
    40, the rows between and after them untouched."""
    _pair("bf16", 2, 72, 192, 3, f32=True)
    seg, pitch = 36, 40
    out = _run("bf16", 2, 72, 192, 3, f32=True, rows=2 * pitch, cmap=(seg, pitch), path=dict(lean=0, cfg=3, epi=0))
    _check(out, None, True, "row map", rows=2 * pitch)
    got = out.float().cpu()[:, :2 * pitch, :N].reshape(2, 2, pitch, N)
    assert torch.isnan(got[:, :, seg:]).all()
    ref = _ref("bf16", 2, 72, 192, f32=True)
    err = (got[:, :, :seg].reshape(2, 72, N) - ref).abs().max().item()
    assert err <= 1e-3 * ref.abs().max().item() + 1e-4, err


def test_edge_forced_split_k():
    """A forced K split keeps the general kernel and its hand-off; unsplit is lean.  Tickets left at zero."""
    _pair("bf16", 2, 72, 320, 3, f32=True, r=True)
    ws = torch.empty(1 << 20, device="cuda")
    cnt = torch.zeros(1 << 12, device="cuda", dtype=torch.int32)
    out = _run("bf16", 2, 72, 320, 3, f32=True, r=True, sk=(2, ws, cnt), path=dict(lean=0, cfg=3, nsk=2))
    _check(out, _ref("bf16", 2, 72, 320, f32=True, r=True), True, "split-K")
    assert int(cnt.abs().sum()) == 0


@pytest.mark.parametrize("bias1", [False, True])
@pytest.mark.parametrize("dname", ["bf16", "fp16"])
def test_multi_bitwise(dname, bias1):
    """The fusion encoder's pair in one launch: a 16-bit plain problem (M 136) beside an fp32 two-pointer one with
    row-mapped R (r_mode 1, r_p0 = M = 72; without a bias as in the frame, and with one).  mmt_gemm_multi at impl 0
    (the lean multi kernel), at impl 10 (the general one) and two mmt_gemm calls at the 64x64 tile: the same bits."""
    L = _lib()
    st = torch.cuda.current_stream().cuda_stream
    kw1 = dict(f32=True, r=True, r_mode=1, r_p0=72, k_split=128, bias=bias1)
    res = []
    for impl in (0, 10, 3):
        o0, o1 = _out(dname, 1, 136, False), _out(dname, 1, 72, True)
        p0 = _params(dname, 1, 136, 128, impl, o0, f32=False)
        p1 = _params(dname, 1, 72, 256, impl, o1, **kw1)
        if impl == 3:
            L.check(L.LIB.mmt_gemm(p0, _code(DT[dname]), st), "value")
            L.check(L.LIB.mmt_gemm(p1, _code(DT[dname]), st), "offsets")
        else:
            arr = (L.GemmParams * 2)(p0, p1)
            # the lean multi kernel (its second problem's form takes the bias or its absence) / the general one
            _path(arr, dname, dict(joint=2, cfg=3, lean=int(impl == 0), form=(PL | LR | A2 | 8) * (impl == 0)), n=2)
            L.check(L.LIB.mmt_gemm_multi(arr, 2, _code(DT[dname]), st), "multi")
        torch.cuda.synchronize()
        res.append((o0, o1))
    for o0, o1 in res[1:]:
        assert torch.equal(_bits(o0), _bits(res[0][0])) and torch.equal(_bits(o1), _bits(res[0][1]))
    _check(res[0][0], _ref(dname, 1, 136, 128, f32=False), False, "multi value %s" % dname)
    _check(res[0][1], _ref(dname, 1, 72, 256, f32=True, r=True, r_p0=72, k_split=128, bias=bias1), True,
           "multi offsets %s" % dname)
