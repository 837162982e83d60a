"""Attention kernels against probes that account for every key (tests/attn_probes.py), at shapes on the
kernels' tile edges (16-key steps of the last key tile, 64-key tiles, 64 / 128-query blocks, a key block that
straddles n_t, more key tiles than ring slots, and the degenerate (1, 1)).

Bars, from the arithmetic (test_attn_probes_host.py asserts the margins that make them discriminating):
  census    |out - ref| <= ulp |ref| (ulp 2^-8 bf16, 2^-11 fp16, 2^-20 f32: P is exactly 1, the fp32 sums are
            exact integers, one rounding to the storage type); |lse - log2 n| <= 1e-4.  One key dropped,
            counted twice or leaked moves a channel by >= 8 bf16 ulps and lse by >= 2.4e-3.
  selector  |out - v[target]| <= 2 ulp |v[target]| + 2^-11 max|v| (the softmax is one-hot to 2^-12).
  backward census  dV within 2^-7 |ref| (P = 1/n rounded once to bf16, the output rounded once); dK
            exactly 0 (q' = 0); dQ within 2^-7 scale sum_k A_qk |k_k| elementwise (mam_bwd_ref).
  t2s column sums  census 1e-6 relative; selector 2^-11 count + 2^-11; random inputs 1e-4 of the largest
            column (an order above the fp32 bound of 64-term dot products).
Random inputs at the same shapes keep the project's bars (1.5e-2 bf16 / fp16, 2e-5 fp32; the backward per
token row, see test_backward_random_rows)."""
import pytest
import torch

import attn_probes as P
from attn_probes import BM, HEADS, SHAPES, DT, ULP, LOG2E

pytestmark = pytest.mark.gpu

S, H, C = 2 * BM, HEADS, 64 * HEADS
GUARD = 7.0
FWD = [("f32", 0)] + [("bf16", i) for i in (0, 4, 8, 17, 21, 22)] + [("fp16", i) for i in (0, 4, 8)]
BF16_IMPLS = [0, 4, 8, 17, 21, 22]
LSE_IMPLS = [0, 4, 8, 17, 21]
STRADDLING = [(49, 64), (63, 65)]  # a 64-key block holds template and search keys


def _lib():
    from mmt_amd import _lib
    return _lib


def _code(dname):
    L = _lib()
    return {"f32": L.MMT_F32, "bf16": L.MMT_BF16, "fp16": L.MMT_F16}[dname]


def _attn(qd, n_t, n_s, dname, impl, asym, scale=P.SCALE, lse=False, q_part=0, tok_pitch=0, out_pitch=0, out_q0=0):
    """One mmt_mam_attention call on qd [S][pitch][3C] (device); out is pre-filled with GUARD."""
    L = _lib()
    nseq, ntok = qd.shape[0], n_t + n_s
    out = torch.full((nseq, out_pitch or tok_pitch or ntok, C), GUARD, device="cuda", dtype=DT[dname])
    lse_t = torch.full((nseq, H, ntok), float("nan"), device="cuda") if lse else None
    p = L.AttnParams()
    p.qkv, p.out, p.S, p.Bm, p.ntok, p.n_t, p.C, p.H, p.asym = qd.data_ptr(), out.data_ptr(), nseq, nseq // 2, ntok, n_t, C, H, asym
    p.scale, p.impl, p.lse = scale, impl, lse_t.data_ptr() if lse else None
    p.q_part, p.tok_pitch, p.out_pitch, p.out_q0 = q_part, tok_pitch, out_pitch, out_q0
    L.check(L.LIB.mmt_mam_attention(p, _code(dname), torch.cuda.current_stream().cuda_stream), "attn")
    torch.cuda.synchronize()
    return out, lse_t


def _first(bad, got, ref, what):
    i = tuple(bad.nonzero()[0].tolist())
    return "%s: %d elements over the bar, first at %s: got %.9g, reference %.9g" % (
        what, int(bad.sum()), i, got[i].item(), ref[i].item())


def _assert_census(out, ref, dname, what="census"):
    got = out.double().cpu()
    bad = (got - ref).abs() > ULP[dname] * ref.abs()
    assert not bad.any(), _first(bad, got, ref, what)


# ---- forward ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_t,n_s", SHAPES)
@pytest.mark.parametrize("asym", [0, 1])
@pytest.mark.parametrize("dname,impl", FWD)
def test_census(dname, impl, asym, n_t, n_s):
    """n * out[j] counts the keys that were summed: exactly the allowed ones, each once."""
    qkv, ref, _ = P.census_case(n_t, n_s, asym, dname)
    out, _ = _attn(qkv.to(DT[dname]).cuda(), n_t, n_s, dname, impl, asym)
    _assert_census(out, ref, dname)


@pytest.mark.parametrize("n_t,n_s", SHAPES)
@pytest.mark.parametrize("asym", [0, 1])
@pytest.mark.parametrize("impl", LSE_IMPLS)
def test_census_lse(impl, asym, n_t, n_s):
    """The training forward's log2-sum-exp2 (bf16) is log2 of the key count, and its out is the census."""
    qkv, ref, lse_ref = P.census_case(n_t, n_s, asym, "bf16")
    out, lse = _attn(qkv.bfloat16().cuda(), n_t, n_s, "bf16", impl, asym, lse=True)
    got = lse.double().cpu()
    bad = ~((got - lse_ref).abs() <= 1e-4)
    assert not bad.any(), _first(bad, got, lse_ref, "lse")
    _assert_census(out, ref, "bf16")


def _assert_selector(out, want, qkv, dname):
    got, want = out.double().cpu(), want.double()
    bar = 2 * ULP[dname] * want.abs() + 2.0 ** -11 * qkv[..., 2 * C:].abs().max().item()
    bad = ~((got - want).abs() <= bar)
    assert not bad.any(), _first(bad, got, want, "selector")


@pytest.mark.parametrize("n_t,n_s", SHAPES)
@pytest.mark.parametrize("asym", [0, 1])
@pytest.mark.parametrize("dname,impl", FWD)
def test_selector(dname, impl, asym, n_t, n_s):
    """Every query returns the v row of the one key it aims at: segment ends, the other modality's
    template, both sides of every 16 / 64-key boundary (a wrong row, head or sequence is an O(1) error)."""
    qkv, want, _ = P.selector_case(n_t, n_s, asym, dname)
    out, _ = _attn(qkv.to(DT[dname]).cuda(), n_t, n_s, dname, impl, asym)
    _assert_selector(out, want, qkv, dname)


@pytest.mark.parametrize("n_t,n_s", SHAPES)
@pytest.mark.parametrize("asym", [0, 1])
@pytest.mark.parametrize("impl", BF16_IMPLS)
def test_selector_prescaled_q(impl, asym, n_t, n_s):
    """The runtime's convention: q arrives times scale * log2(e) (rounded to bf16), scale = 1 / log2(e)."""
    qkv, want, _ = P.selector_case(n_t, n_s, asym, "bf16")
    qs = qkv.clone()
    qs[..., :C] *= P.SCALE * LOG2E
    out, _ = _attn(qs.bfloat16().cuda(), n_t, n_s, "bf16", impl, asym, scale=1.0 / LOG2E)
    _assert_selector(out, want, qkv, "bf16")


@pytest.mark.parametrize("n_t,n_s", SHAPES)
@pytest.mark.parametrize("asym", [0, 1])
@pytest.mark.parametrize("impl", BF16_IMPLS)
def test_selector_out_of_range_scores(impl, asym, n_t, n_s):
    """q = 16 k[target]: the target's log2-score is 185, past the fp32 range of exp2 without a reference
    point, so the range-checked kernels (17 / 21 / 22) take their exact two-pass fallback at every tile-edge
    shape (its own key loop and row clamps); the running-maximum kernels must not care.  Same bar."""
    qkv, want, _ = P.selector_case(n_t, n_s, asym, "bf16")
    qs = qkv.clone()
    qs[..., :C] *= 4
    out, _ = _attn(qs.bfloat16().cuda(), n_t, n_s, "bf16", impl, asym)
    _assert_selector(out, want, qkv, "bf16")


@pytest.mark.parametrize("n_t,n_s", STRADDLING)
@pytest.mark.parametrize("asym", [0, 1])
@pytest.mark.parametrize("impl", BF16_IMPLS)
def test_census_layout_variants(impl, asym, n_t, n_s):
    """Query parts (in place and with compact out_pitch / out_q0) and tok_pitch > ntok with large finite
    values in the rows past ntok (stale pruned tokens): the census still counts exactly the allowed keys,
    and no row outside the part / past ntok is written."""
    qkv, ref, _ = P.census_case(n_t, n_s, asym, "bf16")
    ntok = n_t + n_s
    qd = qkv.bfloat16().cuda()
    for part, rows, q0 in ((1, n_t, 0), (2, n_s, n_t)):
        out, _ = _attn(qd, n_t, n_s, "bf16", impl, asym, q_part=part)
        _assert_census(out[:, q0:q0 + rows], ref[:, q0:q0 + rows], "bf16", "q_part %d" % part)
        rest = torch.cat([out[:, :q0], out[:, q0 + rows:]], 1)
        assert bool((rest == GUARD).all()), part
        out, _ = _attn(qd, n_t, n_s, "bf16", impl, asym, q_part=part, out_pitch=rows + 3, out_q0=q0)
        _assert_census(out[:, :rows], ref[:, q0:q0 + rows], "bf16", "compact q_part %d" % part)
        assert bool((out[:, rows:] == GUARD).all()), part
    pitch = ntok + 5
    qp = torch.full((S, pitch, 3 * C), 1e4)
    qp[:, :ntok] = qkv
    for part, qa, qb in ((0, 0, ntok), (1, 0, n_t), (2, n_t, ntok)):
        out, _ = _attn(qp.bfloat16().cuda(), n_t, n_s, "bf16", impl, asym, q_part=part, tok_pitch=pitch)
        _assert_census(out[:, qa:qb], ref[:, qa:qb], "bf16", "tok_pitch, q_part %d" % part)
        rest = torch.cat([out[:, :qa], out[:, qb:]], 1)
        assert bool((rest == GUARD).all()), part


@pytest.mark.parametrize("n_t,n_s", SHAPES)
@pytest.mark.parametrize("asym", [0, 1])
@pytest.mark.parametrize("dname,impl", FWD)
def test_random_inputs(dname, impl, asym, n_t, n_s):
    """The score arithmetic on N(0, 1) inputs at the tile-edge shapes (test_gpu_ops.test_mam_attention's
    reference and bars)."""
    from test_gpu_ops import _attn_ref
    ntok, dt = n_t + n_s, DT[dname]
    qkv = torch.randn(S, ntok, 3 * C, generator=torch.Generator().manual_seed(5000 + 7 * n_t + n_s + asym))
    out, _ = _attn(qkv.to(dt).cuda(), n_t, n_s, dname, impl, asym)
    ref = _attn_ref(qkv.to(dt).float(), S, BM, ntok, n_t, C, H, asym)
    err = (out.float().cpu() - ref).abs().max().item()
    assert err <= (1.5e-2 if dt != torch.float32 else 2e-5), err


# ---- backward ---------------------------------------------------------------------------------------

def _fwd_bwd(qkv, dout, n_t, n_s, impl):
    """bf16 training forward (lse) and backward on BM sequences; returns dqkv on the CPU (fp64)."""
    L = _lib()
    ntok = n_t + n_s
    qd, dd = qkv.bfloat16().cuda(), dout.bfloat16().cuda()
    out, lse = _attn(qd, n_t, n_s, "bf16", impl, 0, lse=True)
    delta = torch.empty(BM, H, ntok, device="cuda")
    dqkv = torch.full((BM, ntok, 3 * C), float("nan"), device="cuda", dtype=torch.bfloat16)
    b = L.AttnBwdParams()
    b.qkv, b.out, b.dout, b.lse, b.delta, b.dqkv = qd.data_ptr(), out.data_ptr(), dd.data_ptr(), lse.data_ptr(), \
        delta.data_ptr(), dqkv.data_ptr()
    b.S, b.Bm, b.ntok, b.n_t, b.C, b.H, b.asym, b.scale = BM, BM // 2, ntok, n_t, C, H, 0, P.SCALE
    L.check(L.LIB.mmt_mam_attention_bwd(b, L.MMT_BF16, torch.cuda.current_stream().cuda_stream), "attn bwd")
    torch.cuda.synchronize()
    return dqkv.double().cpu()


_BWD_REF = {}


def _bwd_ref(kind, n_t, n_s):
    """fp64 backward reference of the census / random case, computed once and shared (read-only)."""
    key = (kind, n_t, n_s)
    if key not in _BWD_REF:
        if kind == "census":
            qkv, dout = P.census_qkv(n_t, n_s)[:BM].bfloat16().float(), P.bwd_census_dout(n_t, n_s)
        else:
            qkv, dout = P.bwd_random_case(n_t, n_s)
        _BWD_REF[key] = (qkv, dout) + P.mam_bwd_ref(qkv, dout, n_t, BM, H)
    return _BWD_REF[key]


@pytest.mark.parametrize("n_t,n_s", SHAPES)
@pytest.mark.parametrize("impl", [0, 8, 21])
def test_backward_census(impl, n_t, n_s):
    """dV counts the attending queries of every key (each query's share is >= 8x the bar), dK is exactly
    zero, dQ stays inside its elementwise rounding bound."""
    qkv, dout, ref, bound = _bwd_ref("census", n_t, n_s)
    got = _fwd_bwd(qkv, dout, n_t, n_s, impl)
    gq, gk, gv = got.split(C, -1)
    rq, _, rv = ref.split(C, -1)
    bad = ~((gv - rv).abs() <= 2.0 ** -7 * rv.abs())
    assert not bad.any(), _first(bad, gv, rv, "dV")
    assert bool((gk == 0).all()), _first(gk != 0, gk, torch.zeros_like(gk), "dK")
    bad = ~((gq - rq).abs() <= bound)
    assert not bad.any(), _first(bad, gq, rq, "dQ")


@pytest.mark.parametrize("n_t,n_s", P.BWD_RANDOM_SHAPES)
@pytest.mark.parametrize("impl", [0, 8, 21])
def test_backward_random_rows(impl, n_t, n_s):
    """test_gpu_train_ops.test_attention_backward's comparison on N(0, 1) inputs with the error taken per
    token row, relative to that row's largest reference gradient.  The bars are 4x the worst row of a CPU
    emulation of the documented arithmetic (q' = bf16(q scale log2 e), P and dS rounded to bf16, fp32
    sums, bf16 outputs; attn_probes.mam_bwd_emul) against fp64 over the same cases: emulation dQ 7.66e-3,
    dK 1.124e-2, dV 7.90e-3 -> bars 3.06e-2, 4.50e-2, 3.16e-2 (attn_probes.BWD_ROW_BAR)."""
    qkv, dout, ref, _ = _bwd_ref("random", n_t, n_s)
    got = _fwd_bwd(qkv, dout, n_t, n_s, impl)
    err = P.row_rel_err(got, ref, C).tolist()
    print("per-row rel err dQ %.3g dK %.3g dV %.3g" % tuple(err))
    for nm, e, bar in zip("qkv", err, P.BWD_ROW_BAR):
        assert e <= bar, (nm, e, bar)


# ---- template -> search column sums (candidate elimination) ------------------------------------------

def _t2s(qkv, dname, n_t, n_s, mask):
    """mmt_ce_t2s_attention[_masked] on qkv [S][pitch][3C]; the partial rows of each (b, h) summed on the host."""
    L = _lib()
    qd = qkv.to(DT[dname]).cuda()
    nparts = 2 * n_t // (16 if dname == "bf16" else 8)
    part = torch.full((BM, H, nparts, 2 * n_s), float("nan"), device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    args = (BM, qkv.shape[1], n_t, n_s, C, H, P.SCALE, _code(dname), st)
    if mask is None:
        L.check(L.LIB.mmt_ce_t2s_attention(qd.data_ptr(), part.data_ptr(), *args), "t2s")
    else:
        md = mask.cuda()
        L.check(L.LIB.mmt_ce_t2s_attention_masked(qd.data_ptr(), part.data_ptr(), md.data_ptr(), *args), "t2s masked")
    torch.cuda.synchronize()
    return part.double().cpu().sum(2)


def _t2s_masks(n_t):
    ones = torch.ones(BM, 2 * n_t, dtype=torch.uint8)
    four = torch.zeros_like(ones)
    for b in range(BM):
        four[b, [1 + b, n_t - 1, n_t + 2, 2 * n_t - 1 - b]] = 1
    block = ones.clone()  # one whole 16-query block masked out (the early exit) and half of another
    block[:, :24 if 2 * n_t >= 32 else 8] = 0
    return {"none": None, "ones": ones, "four": four, "block": block}


@pytest.mark.parametrize("n_s", [1, 7, 8, 9, 33, 138, 576])
@pytest.mark.parametrize("n_t", [8, 64])
@pytest.mark.parametrize("dname", ["bf16", "f32"])
def test_t2s_column_sums(dname, n_t, n_s):
    """mmt_ce_t2s_attention / _masked called directly (576 is the bf16 kernel's limit, uneven key blocks per
    wave at 33), every mask kind, tok_pitch > n_t + n_s with large finite rows beyond."""
    pitch = n_t + n_s + 3
    g = torch.Generator().manual_seed(6000 + 7 * n_t + n_s)
    census = torch.randn(S, pitch, 3 * C, generator=g)
    census[..., :C] = 0
    selector, tgt = P.t2s_selector_qkv(BM, n_t, n_s, H, pitch)
    rnd = torch.randn(S, pitch, 3 * C, generator=g)
    for x in (census, selector, rnd):
        x[:, n_t + n_s:] = 1e4
    packed = rnd[:, :n_t + n_s].contiguous()  # and tok_pitch == n_t + n_s
    for name, mask in _t2s_masks(n_t).items():
        m = torch.ones(BM, 2 * n_t, dtype=torch.float64) if mask is None else mask.double()
        got = _t2s(census, dname, n_t, n_s, mask)
        want = (m.sum(1) / (2 * n_s))[:, None, None].expand(BM, H, 2 * n_s)
        bad = ~((got - want).abs() <= 1e-6 * want)
        assert not bad.any(), _first(bad, got, want, "t2s census, mask " + name)
        got = _t2s(selector, dname, n_t, n_s, mask)
        want = torch.zeros(BM, H, 2 * n_s, dtype=torch.float64)
        for b in range(BM):
            for h in range(H):
                want[b, h].index_add_(0, tgt[b, h], m[b])
        bad = ~((got - want).abs() <= 2.0 ** -11 * want + 2.0 ** -11)
        assert not bad.any(), _first(bad, got, want, "t2s selector, mask " + name)
        for x in (rnd, packed):
            got = _t2s(x, dname, n_t, n_s, mask)
            want = P.t2s_ref(x.to(DT[dname]), BM, n_t, n_s, H, P.SCALE, mask)
            bad = ~((got - want).abs() <= 1e-4 * want.abs().max())
            assert not bad.any(), _first(bad, got, want, "t2s random, mask " + name)


def test_t2s_rejects_unsupported_shapes():
    """MMT_EBADARG with real device buffers too: 2 n_t % 16 != 0; bf16 with 2 n_s > 1152; nothing is written."""
    L = _lib()
    st = torch.cuda.current_stream().cuda_stream
    qd = torch.zeros(S, 64 + 577, 3 * C, device="cuda", dtype=torch.bfloat16)
    part = torch.full((BM * H * 8 * 2 * 577,), GUARD, device="cuda")
    assert L.LIB.mmt_ce_t2s_attention(qd.data_ptr(), part.data_ptr(), BM, 64 + 577, 64, 577, C, H, P.SCALE, L.MMT_BF16, st) == -10000
    for dt in (L.MMT_BF16, L.MMT_F32):
        assert L.LIB.mmt_ce_t2s_attention(qd.data_ptr(), part.data_ptr(), BM, 12 + 64, 12, 64, C, H, P.SCALE, dt, st) == -10000
    torch.cuda.synchronize()
    assert bool((part == GUARD).all())
