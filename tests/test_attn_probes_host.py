"""The attention probes of tests/attn_probes.py, checked on the CPU: the shape list covers the kernels' tile
edges, the fp64 references agree with the project's references, and every probe is discriminating by the
margin its GPU bar needs (one key removed or added moves the census by >= 8 bf16 ulps; a reference with
one key removed violates the GPU bar at each of the ten tail classes; the selector's softmax is one-hot
to 2^-12; one query removed moves the backward census' dV by >= 8x its bar)."""
import math

import pytest
import torch

import attn_probes as P
from attn_probes import BM, HEADS, SHAPES

ULP_BF16 = 2.0 ** -8
S, H, C = 2 * BM, HEADS, HEADS * 64


def test_shapes_cover_the_tile_edges():
    tails = {lk % 64 for n_t, n_s in SHAPES for lk in P.key_counts(n_t, n_s)}
    assert set(P.TAIL_CLASSES) <= tails, sorted(set(P.TAIL_CLASSES) - tails)
    counts = [n for shape in SHAPES for n in shape]
    for m in (64, 128):  # query blocks of 64 (latency / fp32 / backward) and 128 (throughput kernels)
        assert any(n % m == 1 for n in counts) and any(n % m == 63 for n in counts), m
        assert any(n % m == m - 1 for n in counts) and any(n % m == 0 for n in counts), m
        assert any(n == m + 1 or (n > m and n % m == 1) for n in counts), m  # one past a full block
    # a 64-key block that holds template and search keys (the backward's dK / dV workgroups)
    assert any(n_t % 64 and (n_t // 64) * 64 + 64 <= n_t + n_s for n_t, n_s in SHAPES)
    # more key tiles than the 8 ring slots of the latency kernel
    assert any((n_t + n_s + 63) // 64 > 8 for n_t, n_s in SHAPES)
    assert (1, 1) in SHAPES
    # what candidate elimination produces: n_t a multiple of 8 with an arbitrary n_s
    assert any(n_t % 8 == 0 and n_t < 64 and n_s % 16 for n_t, n_s in SHAPES)


@pytest.mark.parametrize("asym", [0, 1])
def test_mam_ref_matches_the_project_reference(asym):
    from test_gpu_ops import _attn_ref
    n_t, n_s = 17, 45
    qkv = torch.randn(S, n_t + n_s, 3 * C, generator=torch.Generator().manual_seed(1))
    out, lse = P.mam_ref(qkv, n_t, BM, H, asym)
    ref = _attn_ref(qkv.double(), S, BM, n_t + n_s, n_t, C, H, asym)
    assert (out - ref).abs().max().item() <= 1e-6
    # lse against the definition, one query
    q, k, _ = P.split_heads(qkv, H)
    seq, row = P.key_index(3, 1, n_t, n_s, BM, asym)
    sc = (k[seq, 1, row] @ q[3, 1, n_t + 5]) * P.SCALE * P.LOG2E
    assert abs(torch.log2(torch.exp2(sc).sum()).item() - lse[3, 1, n_t + 5].item()) <= 1e-9


def test_mam_bwd_ref_matches_autograd():
    from test_gpu_train_ops import _attn_ref
    n_t, n_s = 17, 45
    qkv, dout = P.bwd_random_case(n_t, n_s)
    q, k, v = (t.clone().requires_grad_(True) for t in P.split_heads(qkv, H))
    o = _attn_ref(q, k, v, n_t)
    o.backward(dout.double().view(BM, n_t + n_s, H, 64).permute(0, 2, 1, 3))
    want = torch.cat([P.merge_heads(t.grad) for t in (q, k, v)], -1)
    got, bound = P.mam_bwd_ref(qkv, dout, n_t, BM, H)
    assert (got - want).abs().max().item() <= 1e-10
    assert (bound >= 0).all()


def _class_values(v, s, cls, n_t, n_s, asym):
    seq, row = P.key_index(s, cls, n_t, n_s, BM, asym)
    fseq, frow = P.forbidden_index(s, cls, n_t, n_s, BM, asym)
    return v[seq, row], v[fseq, frow]  # [n][H][64], [m][H][64]


@pytest.mark.parametrize("asym", [0, 1])
@pytest.mark.parametrize("n_t,n_s", SHAPES)
def test_census_sees_every_single_key(n_t, n_s, asym):
    """q = 0, so out of every query of a class is the mean of its keys' v rows (checked against mam_ref)
    and lse = log2 n.  One allowed key less, or one forbidden key more (a search key for a template
    query; another sequence's search key or the wrong sequence's template key), moves some channel by
    at least 8 bf16 ulps relative -- the GPU bar is one ulp."""
    qkv, out, lse = P.census_case(n_t, n_s, asym, "bf16")
    vq = qkv[..., 2 * C:]  # the census values are exact in every storage type (k is random and unused: q = 0)
    assert torch.equal(vq.bfloat16().float(), vq) and torch.equal(vq.half().float(), vq)
    assert qkv[..., :C].abs().max().item() == 0.0
    v = P.split_heads(qkv, H)[2].permute(0, 2, 1, 3)  # [S][ntok][H][64]
    worst = math.inf
    for s in range(S):
        for cls, (qa, qb) in enumerate(((0, n_t), (n_t, n_t + n_s))):
            allowed, forbidden = _class_values(v, s, cls, n_t, n_s, asym)
            n = allowed.shape[0]
            assert n == P.key_counts(n_t, n_s)[0 if cls == 0 else 1 + asym]
            T = allowed.sum(0)
            base = T / n
            for qi in (qa, qb - 1):
                assert (out[s, qi].view(H, 64) - base).abs().max().item() <= 1e-12
                assert (lse[s, :, qi] - math.log2(n)).abs().max().item() <= 1e-12
            assert torch.equal(T, T.round())  # n * out is an integer census
            cases = [(T + forbidden) / (n + 1)]
            if n > 1:
                cases.append((T - allowed) / (n - 1))
            assert forbidden.shape[0] > 0
            for new in cases:
                d = (new - base).abs()
                rel = torch.where(base > 0, d / base.clamp_min(1e-300), torch.where(d > 0, math.inf, 0.0))
                worst = min(worst, rel.amax(-1).min().item())
    print("census %s asym %d: smallest single-key effect %.3g (bf16 ulp %.3g)" % ((n_t, n_s), asym, worst, ULP_BF16))
    assert worst >= 8 * ULP_BF16, worst


@pytest.mark.parametrize("tail", P.TAIL_CLASSES)
def test_reference_with_one_key_removed_violates_the_census_bar(tail):
    """Sensitivity, on the reference alone: at a key count of every tail class, the fp64 reference that
    leaves out the last key of the list breaks |out - ref| <= ulp |ref| (bf16) and |lse - log2 n| <= 1e-4."""
    n_t, n_s, kind = next((a, b, i) for a, b in SHAPES if (a, b) != (1, 1)
                          for i, lk in enumerate(P.key_counts(a, b)) if lk % 64 == tail)
    cls, asym = (0, 0) if kind == 0 else (1, kind - 1)
    qkv, out, lse = P.census_case(n_t, n_s, asym, "bf16")
    bad, bad_lse = P.mam_ref(qkv, n_t, BM, H, asym,
                             edit=lambda s, c, seq, row: (seq[:-1], row[:-1]) if c == cls else (seq, row))
    qa, qb = ((0, n_t), (n_t, n_t + n_s))[cls]
    for s in range(S):
        for qi in range(qa, qb):
            assert ((bad[s, qi] - out[s, qi]).abs() > ULP_BF16 * out[s, qi].abs()).any()
            assert ((bad_lse[s, :, qi] - lse[s, :, qi]).abs() > 1e-4).all()


@pytest.mark.parametrize("asym", [0, 1])
@pytest.mark.parametrize("n_t,n_s", SHAPES)
def test_selector_is_one_hot_and_aims_at_every_edge(n_t, n_s, asym):
    qkv, want, pos = P.selector_case(n_t, n_s, asym, "bf16")
    for dn in ("bf16", "fp16"):
        assert torch.equal(qkv[..., :2 * C].to(P.DT[dn]).float(), qkv[..., :2 * C])  # q, k exact
    out, _ = P.mam_ref(qkv, n_t, BM, H, asym)
    wmin, smax = 1.0, -math.inf
    for s, cls, qa, qb, seq, row, sc in P.mam_classes(qkv, n_t, BM, H, asym, P.SCALE):
        w = torch.softmax(sc, -1).gather(-1, pos[s, :, qa:qb, None])
        wmin, smax = min(wmin, w.min().item()), max(smax, sc.max().item() * P.LOG2E)
        assert int(pos[s, :, qa:qb].max()) < len(row)
    print("selector %s asym %d: 1 - smallest target weight %.3g, largest log2-score %.1f" % ((n_t, n_s), asym, 1 - wmin, smax))
    assert wmin >= 1 - 2.0 ** -12
    assert smax <= 64  # the range-checked kernels stay on their fast path
    assert (out - want.double()).abs().max().item() <= 2.0 ** -11 * want.abs().max().item()
    for cls, (qa, qb) in enumerate(((0, n_t), (n_t, n_t + n_s))):
        segs = P.key_segments(cls, n_t, n_s, asym)
        hit = set(pos[:, :, qa:qb].reshape(-1).tolist())
        slots = S * H * (qb - qa)
        must = P.must_positions(segs)
        # segment ends (incl. the other modality's template) and both sides of every 16 / 64-key boundary
        assert set(must[:slots]) <= hit
        assert len(must) <= slots, "shape has too few queries to aim at every edge"
        if slots >= sum(segs):
            assert hit == set(range(sum(segs)))  # every allowed key is some query's target
    for s in range(S):  # every template query of every (s, h): each template key exactly once
        for h in range(H):
            assert sorted(pos[s, h, :n_t].tolist()) == list(range(n_t))


@pytest.mark.parametrize("n_t,n_s", SHAPES)
def test_backward_census_sees_every_single_query(n_t, n_s):
    """dV[k] = sum over the queries that attend k of dout_q / n_q; taking any one of them out changes its
    channel by at least 8x the GPU bar (2^-7 relative); dK = 0; dout is exact in bf16."""
    qkv = P.census_qkv(n_t, n_s)[:BM]
    dout = P.bwd_census_dout(n_t, n_s)
    assert torch.equal(dout.bfloat16().float(), dout)
    ref, _ = P.mam_bwd_ref(qkv, dout, n_t, BM, H)
    assert ref[..., C:2 * C].abs().max().item() == 0.0
    dv = ref[..., 2 * C:].view(BM, n_t + n_s, H, 64)
    q = torch.arange(n_t + n_s)
    share = P.bwd_census_weight(q, n_t, n_s).double() / torch.where(q < n_t, n_t, n_t + n_s)  # dout_q / n_q
    worst = math.inf
    for key, attending in ((0, q), (n_t + n_s - 1, q[n_t:])):  # a template key, a search key
        tot = dv[0, key, 0, attending % 64]
        again = torch.zeros(64, dtype=torch.float64).index_add_(0, attending % 64, share[attending])
        assert (again - dv[0, key, 0]).abs().max().item() <= 1e-12
        worst = min(worst, (share[attending] / tot).min().item())
    print("backward census %s: smallest single-query share %.3g (bar %.3g)" % ((n_t, n_s), worst, 2.0 ** -7))
    assert worst >= 8 * 2.0 ** -7, worst


def test_backward_row_bars_are_four_times_the_emulation():
    """BWD_ROW_BAR = 4 x the worst row of the documented arithmetic (mam_bwd_emul) against fp64 over the
    random cases the GPU test uses."""
    worst = torch.zeros(3, dtype=torch.float64)
    assert set(SHAPES) - set(P.BWD_RANDOM_SHAPES) == {(1, 1)}
    for n_t, n_s in P.BWD_RANDOM_SHAPES:
        qkv, dout = P.bwd_random_case(n_t, n_s)
        ref, _ = P.mam_bwd_ref(qkv, dout, n_t, BM, H)
        worst = torch.maximum(worst, P.row_rel_err(P.mam_bwd_emul(qkv, dout, n_t, H), ref, C))
    print("emulated per-row errors dQ dK dV:", ["%.4g" % x for x in worst.tolist()])
    for w, e, b in zip(worst.tolist(), P.BWD_ROW_EMUL, P.BWD_ROW_BAR):
        assert abs(w - e) <= 0.05 * e, (w, e)
        assert b == 4 * e


@pytest.mark.parametrize("n_t", [8, 64])
@pytest.mark.parametrize("n_s", [1, 7, 8, 9, 33, 138, 576])
def test_t2s_selector_is_one_hot(n_t, n_s):
    qkv, tgt = P.t2s_selector_qkv(BM, n_t, n_s, H, n_t + n_s + 3)
    assert torch.equal(qkv[..., :2 * C].bfloat16().float(), qkv[..., :2 * C])
    cols = P.t2s_ref(qkv, BM, n_t, n_s, H, P.SCALE)
    counts = torch.zeros_like(cols)
    for b in range(BM):
        for h in range(H):
            counts[b, h].index_add_(0, tgt[b, h], torch.ones(2 * n_t, dtype=torch.float64))
    assert (cols - counts).abs().max().item() <= 2.0 ** -12
    if 2 * n_t * BM * H >= 2 * n_s:
        assert (counts.sum((0, 1)) > 0).all()


def test_t2s_rejects_unsupported_shapes():
    """MMT_EBADARG on the host, nothing launched: 2 n_t not a multiple of 16; bf16 with 2 n_s > 1152."""
    from mmt_amd import _lib
    fake = 1 << 20  # 16-B aligned, never dereferenced

    def t2s(n_t, n_s, dt, mask=None):
        return _lib.LIB.mmt_ce_t2s_attention_masked(fake, fake, mask, 2, n_t + n_s, n_t, n_s, 128, 2, 0.125, dt, None)
    for dt in (_lib.MMT_BF16, _lib.MMT_F32):
        assert t2s(4, 64, dt) == -10000 and t2s(12, 64, dt) == -10000 and t2s(63, 64, dt) == -10000
        assert _lib.LIB.mmt_ce_t2s_attention(fake, fake, 2, 8 + 64, 4, 64, 128, 2, 0.125, dt, None) == -10000
    assert t2s(64, 577, _lib.MMT_BF16) == -10000
    assert t2s(64, 577, _lib.MMT_BF16, fake) == -10000
    assert t2s(64, 1025, _lib.MMT_F32) == -10000
    assert _lib.LIB.mmt_ce_t2s_attention_masked(fake, fake, None, 2, 64 + 100 - 1, 64, 100, 128, 2, 0.125,
                                                _lib.MMT_BF16, None) == -10000  # tok_pitch < n_t + n_s
