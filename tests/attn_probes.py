"""Probe inputs and fp64 references of the attention tests (no tests here).

References (plain fp64 torch on the CPU, key sets spelled out as index lists in the kernels' key order):
  mam_ref       MAM attention, joint (asym 0) or cross-modal (asym 1) key sets: out and the log2-sum-exp2
  mam_bwd_ref   its backward (asym 0) with the elementwise rounding bound of dQ
  mam_bwd_emul  the backward kernels' documented arithmetic (bf16 q', P, dS; fp32 sums; bf16 outputs)
  t2s_ref       column sums of the template->search softmax (mmt_ce_t2s_attention[_masked])

Probes -- inputs on which every single key (and, in the backward, every single query) shows in the result
at a bar that follows from the arithmetic, so an off-by-one key range, a wrong tail mask or one leaked
forbidden key cannot hide below a tolerance sized for random inputs:
  census    q = 0: every allowed key weighs exactly 1/n; v[s, h, r, j] = a(s, h, r) * [j == r % 64] with a
            small integer a, so n * out[j] counts the keys that were summed and lse = log2 n.  P is
            exactly 1, the sums are exact integers in fp32, the result is rounded once.
  selector  k = random +-1 rows, q_i = 4 * k[target(i)]: the softmax is one-hot on the target up to
            2^-12, so out_i = v[target(i)]; a wrong row, head or sequence is an O(1) error.
  backward census: the census qkv with dout[s, q, h, j] = w(q) * [j == q % 64]: dV counts the attending
            queries of every key, dK is exactly 0 (q' = 0).

SHAPES are (n_t, n_s) pairs that sit on the kernels' tile edges (16-key steps of the last key tile, 64-key
tiles, 64 / 128-query workgroups), not workloads; test_attn_probes_host.py asserts what they cover and
the margins that make the probes discriminating.
"""
import functools
import math

import torch

LOG2E = 1.4426950408889634
D = 64
BM, HEADS = 2, 2  # S = 4 sequences (b and b + Bm differ), 2 heads
SCALE = 0.125

SHAPES = [(49, 64), (63, 65), (17, 129), (64, 193), (32, 48), (33, 31), (128, 15), (16, 561), (8, 127), (1, 1)]
TAIL_CLASSES = (0, 1, 15, 16, 17, 32, 33, 48, 49, 63)
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
ULP = {"f32": 2.0 ** -20, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}  # one rounding to the storage type


def key_counts(n_t, n_s):
    """Lk of the template queries, the joint search queries and the cross-modal search queries."""
    return n_t, n_t + n_s, 2 * n_t + n_s


def key_segments(cls, n_t, n_s, asym):
    """Lengths of the key segments of query class cls (0 template, 1 search) in key order."""
    if cls == 0:
        return [n_t]
    return [n_t, n_t, n_s] if asym else [n_t, n_s]


def key_index(s, cls, n_t, n_s, Bm, asym):
    """(seq, row): the keys that queries of class cls of sequence s attend, in the kernels' key order."""
    ntok = n_t + n_s
    if cls == 0:
        return torch.full((n_t,), s), torch.arange(n_t)
    if not asym:
        return torch.full((ntok,), s), torch.arange(ntok)
    b = s % Bm
    seq = torch.cat([torch.full((n_t,), b), torch.full((n_t,), b + Bm), torch.full((n_s,), s)])
    return seq, torch.cat([torch.arange(n_t), torch.arange(n_t), torch.arange(n_t, ntok)])


def forbidden_index(s, cls, n_t, n_s, Bm, asym):
    """(seq, row) of every key of the same head that class cls of sequence s must NOT attend."""
    S, ntok = 2 * Bm, n_t + n_s
    seq, row = key_index(s, cls, n_t, n_s, Bm, asym)
    allowed = torch.zeros(S, ntok, dtype=torch.bool)
    allowed[seq, row] = True
    f = (~allowed).nonzero()
    return f[:, 0], f[:, 1]


def split_heads(x, H):
    """[S][ntok][3C] -> q, k, v [S][H][ntok][64] (fp64)."""
    S, ntok = x.shape[:2]
    return x.double().view(S, ntok, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)


def merge_heads(x):
    """[S][H][ntok][64] -> [S][ntok][C]."""
    S, H, ntok, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(S, ntok, H * D)


def mam_classes(qkv, n_t, Bm, H, asym, scale, edit=None):
    """Yields (s, cls, qa, qb, seq, row, sc): queries [qa, qb) of sequence s, their key index lists
    and the natural-log scores sc [H][qb - qa][n].  edit(s, cls, seq, row) -> (seq, row) changes a key
    set (the host test's one-key-removed / one-key-added references)."""
    q, k, _ = split_heads(qkv, H)
    S, ntok = qkv.shape[:2]
    for s in range(S):
        for cls, (qa, qb) in enumerate(((0, n_t), (n_t, ntok))):
            seq, row = key_index(s, cls, n_t, ntok - n_t, Bm, asym)
            if edit is not None:
                seq, row = edit(s, cls, seq, row)
            kk = k[seq, :, row].permute(1, 0, 2)  # [H][n][64]
            yield s, cls, qa, qb, seq, row, q[s, :, qa:qb] @ kk.transpose(-1, -2) * scale


def mam_ref(qkv, n_t, Bm, H, asym, scale=SCALE, edit=None):
    """out [S][ntok][C] and lse [S][H][ntok] = log2 sum_k exp2(q.k * scale * log2 e), fp64."""
    _, _, v = split_heads(qkv, H)
    S, ntok = qkv.shape[:2]
    out = torch.zeros(S, H, ntok, D, dtype=torch.float64)
    lse = torch.zeros(S, H, ntok, dtype=torch.float64)
    for s, cls, qa, qb, seq, row, sc in mam_classes(qkv, n_t, Bm, H, asym, scale, edit):
        out[s, :, qa:qb] = torch.softmax(sc, -1) @ v[seq, :, row].permute(1, 0, 2)
        lse[s, :, qa:qb] = torch.logsumexp(sc, -1) * LOG2E
    return merge_heads(out), lse


def mam_bwd_ref(qkv, dout, n_t, Bm, H, scale=SCALE):
    """dqkv [S][ntok][3C] of the joint (asym 0) MAM attention in fp64, and the elementwise bound of the
    bf16 kernels' dQ error: 2^-7 * scale * sum_k A_qk |k_k| with A_qk = P_qk (|dP_qk| + sum_j |dO_qj O_qj|)
    (three bf16 roundings of at most 2^-9 each against the sum of absolute terms)."""
    _, k, v = split_heads(qkv, H)
    S, ntok = qkv.shape[:2]
    do = dout.double().view(S, ntok, H, D).permute(0, 2, 1, 3)
    q = split_heads(qkv, H)[0]
    dq, dk, dv, bound = (torch.zeros(S, H, ntok, D, dtype=torch.float64) for _ in range(4))
    for s, cls, qa, qb, seq, row, sc in mam_classes(qkv, n_t, Bm, H, 0, scale):
        P = torch.softmax(sc, -1)
        kk, vv, dO = k[s][:, row], v[s][:, row], do[s, :, qa:qb]
        dP = dO @ vv.transpose(-1, -2)
        O = P @ vv
        dS = P * (dP - (dO * O).sum(-1, keepdim=True))
        dq[s, :, qa:qb] = scale * dS @ kk
        dk[s, :, :len(row)] += scale * dS.transpose(-1, -2) @ q[s, :, qa:qb]
        dv[s, :, :len(row)] += P.transpose(-1, -2) @ dO
        A = P * (dP.abs() + (dO * O).abs().sum(-1, keepdim=True))
        bound[s, :, qa:qb] = 2.0 ** -7 * scale * A @ kk.abs()
    return torch.cat([merge_heads(dq), merge_heads(dk), merge_heads(dv)], -1), merge_heads(bound)


def _bf(x):
    return x.bfloat16().float()


def mam_bwd_emul(qkv, dout, n_t, H, scale=SCALE):
    """The arithmetic attention_bwd.hip documents, on the CPU (joint key sets, bf16 inputs): q' = bf16(q *
    scale * log2 e); the forward's P rounded to bf16 for the row sums and O, lse = log2 of those sums, O
    stored in bf16; P = exp2(q'.k - lse); delta from the bf16 dO and O; dS and (for dV) P rounded to
    bf16; fp32 sums; dQ = bf16(scale * dS k), dK = bf16(dS^T q' / log2 e), dV = bf16(P^T dO)."""
    x = qkv.bfloat16().float()
    S, ntok = x.shape[:2]
    q, k, v = x.view(S, ntok, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)
    do = dout.bfloat16().float().view(S, ntok, H, D).permute(0, 2, 1, 3)
    qs = _bf(q * (scale * LOG2E))
    dq, dk, dv = (torch.zeros(S, H, ntok, D) for _ in range(3))
    for qa, qb, n in ((0, n_t, n_t), (n_t, ntok, ntok)):
        s2 = qs[:, :, qa:qb] @ k[:, :, :n].transpose(-1, -2)
        m = s2.max(-1, keepdim=True)[0]
        pf = _bf(torch.exp2(s2 - m))
        l = pf.sum(-1, keepdim=True)
        O = _bf(pf @ v[:, :, :n] / l)
        P = torch.exp2(s2 - (m + torch.log2(l)))
        dO = do[:, :, qa:qb]
        dS = _bf(P * (dO @ v[:, :, :n].transpose(-1, -2) - (dO * O).sum(-1, keepdim=True)))
        dq[:, :, qa:qb] = dS @ k[:, :, :n] * scale
        dk[:, :, :n] += dS.transpose(-1, -2) @ qs[:, :, qa:qb] / LOG2E
        dv[:, :, :n] += _bf(P).transpose(-1, -2) @ dO
    return _bf(torch.cat([merge_heads(dq), merge_heads(dk), merge_heads(dv)], -1))


def row_rel_err(got, ref, C):
    """Per gradient (q, k, v): the largest error of a token row relative to that row's largest reference
    gradient, maximised over the rows -> [3] (a boundary row cannot hide behind the global maximum)."""
    g = got.double().reshape(-1, 3, C)
    r = ref.double().reshape(-1, 3, C)
    err, den = (g - r).abs().amax(-1), r.abs().amax(-1)
    zero = torch.where(err > 0, math.inf, 0.0).double()  # a row whose reference is 0 must be 0
    return torch.where(den > 0, err / den.clamp_min(1e-300), zero).amax(0)


# ---- census probe -----------------------------------------------------------------------------------

def census_value(s, h, r, H=HEADS):
    """a(s, h, r): 20..50, exact in bf16 and fp16.  Flat enough that one key among the ~10 that share a
    channel at 593 keys still moves that channel by > 8 bf16 ulps; steps with the 64-row block and with
    (sequence, head), distinct for every (sequence, head) at one row."""
    return 20 + r // 64 + 3 * (s * H + h)


def census_qkv(n_t, n_s, Bm=BM, H=HEADS, seed=0):
    """[S][ntok][3C] fp32: q = 0, k random, v the census values (exact in every storage type)."""
    S, ntok, C = 2 * Bm, n_t + n_s, H * D
    g = torch.Generator().manual_seed(1000 + 7 * n_t + n_s + seed)
    x = torch.zeros(S, ntok, 3, H, D)
    x[:, :, 1] = torch.randn(S, ntok, H, D, generator=g)
    r = torch.arange(ntok)
    for s in range(S):
        for h in range(H):
            e = torch.zeros(ntok, D)
            e[r, r % 64] = census_value(s, h, r, H).float()
            x[s, :, 2, h] = e
    return x.view(S, ntok, 3 * C)


def bwd_census_weight(q, n_t, n_s):
    """w(q) of the backward census' dout: (32 + q // 64), search queries times the power of two nearest
    ntok / n_t, so that a template query's 1/n_t and a search query's 1/ntok shares of a template key's
    dV are comparable (each of the ~10 queries of a channel stays above 8x the bar); exact in bf16."""
    g = 2.0 ** round(math.log2((n_t + n_s) / n_t))
    return (32 + q // 64) * torch.where(q < n_t, 1.0, g)


def bwd_census_dout(n_t, n_s, S=BM, H=HEADS):
    """[S][ntok][C]: dout[s, q, h, j] = w(q) * [j == q % 64]."""
    ntok = n_t + n_s
    q = torch.arange(ntok)
    e = torch.zeros(ntok, D)
    e[q, q % 64] = bwd_census_weight(q, n_t, n_s).float()
    return e[None, :, None, :].expand(S, ntok, H, D).reshape(S, ntok, H * D)


# ---- selector probe ---------------------------------------------------------------------------------

def must_positions(segs):
    """Key positions every selector must aim at: the first and last key of each segment and both sides
    of every 16-key (hence every 64-key) boundary of the key list."""
    L, must, o = sum(segs), set(), 0
    for n in segs:
        must.update((o, o + n - 1))
        o += n
    for b in range(16, L, 16):
        must.update((b - 1, b))
    return sorted(must)


def probe_order(segs):
    """All key positions, the must_positions first, then the rest in a fixed shuffled order (so that a
    window of the order samples every segment)."""
    L = sum(segs)
    must = must_positions(segs)
    rest = torch.ones(L, dtype=torch.bool)
    rest[must] = False
    rest = rest.nonzero()[:, 0]
    rest = rest[torch.randperm(len(rest), generator=torch.Generator().manual_seed(L))]
    return torch.cat([torch.tensor(must, dtype=torch.long), rest])


def selector_targets(n_t, n_s, asym, Bm=BM, H=HEADS):
    """pos [S][H][ntok]: position in its key list of the key that query i of (s, h) selects.  Template
    queries: a rotation of the order (n_t queries, n_t keys: every key once).  Search queries: (s, h)
    takes the window [(s H + h) n_s, +n_s) of the order, so the union over (s, h) covers S H n_s
    positions, must_positions first."""
    S, ntok = 2 * Bm, n_t + n_s
    pos = torch.zeros(S, H, ntok, dtype=torch.long)
    ot, os_ = probe_order(key_segments(0, n_t, n_s, asym)), probe_order(key_segments(1, n_t, n_s, asym))
    for s in range(S):
        for h in range(H):
            g = s * H + h
            pos[s, h, :n_t] = ot[(7 * g + torch.arange(n_t)) % len(ot)]
            pos[s, h, n_t:] = os_[(g * n_s + torch.arange(n_s)) % len(os_)]
    return pos


def selector_qkv(n_t, n_s, asym, dname, Bm=BM, H=HEADS):
    """(qkv [S][ntok][3C] fp32 holding values exact in dtype `dname`, want [S][ntok][C] = v[target], pos)."""
    S, ntok, C = 2 * Bm, n_t + n_s, H * D
    g = torch.Generator().manual_seed(2000 + 7 * n_t + n_s + asym)
    k = torch.randint(0, 2, (S, ntok, H, D), generator=g).float() * 2 - 1
    v = torch.randn(S, ntok, H, D, generator=g).to(DT[dname]).float()
    pos = selector_targets(n_t, n_s, asym, Bm, H)
    q, want = torch.zeros(S, ntok, H, D), torch.zeros(S, ntok, H, D)
    for s in range(S):
        for cls, (qa, qb) in enumerate(((0, n_t), (n_t, ntok))):
            seq, row = key_index(s, cls, n_t, n_s, Bm, asym)
            for h in range(H):
                p = pos[s, h, qa:qb]
                q[s, qa:qb, h] = 4 * k[seq[p], row[p], h]
                want[s, qa:qb, h] = v[seq[p], row[p], h]
    return torch.stack([q, k, v], 2).view(S, ntok, 3 * C), want.view(S, ntok, C), pos


@functools.lru_cache(maxsize=None)
def census_case(n_t, n_s, asym, dname):
    """(qkv fp32, fp64 out, fp64 lse) of the census at one shape, computed once and shared (read-only)."""
    qkv = census_qkv(n_t, n_s)
    out, lse = mam_ref(qkv.to(DT[dname]), n_t, BM, HEADS, asym)
    return qkv, out, lse


@functools.lru_cache(maxsize=None)
def selector_case(n_t, n_s, asym, dname):
    return selector_qkv(n_t, n_s, asym, dname)


# ---- template -> search column sums (candidate elimination) ------------------------------------------

def t2s_ref(qkv, Bm, n_t, n_s, H, scale, mask=None):
    """[Bm][H][2 n_s] fp64: per frame and head, the softmax over the keys [k_s_V | k_s_I] of the queries
    [q_mt_V ; q_mt_I] (rows of qkv [S][pitch][3C]), the rows with a nonzero mask [Bm][2 n_t] summed."""
    q, k, _ = split_heads(qkv, H)
    cols = torch.zeros(Bm, H, 2 * n_s, dtype=torch.float64)
    for b in range(Bm):
        qq = torch.cat([q[b, :, :n_t], q[b + Bm, :, :n_t]], 1)
        kk = torch.cat([k[b, :, n_t:n_t + n_s], k[b + Bm, :, n_t:n_t + n_s]], 1)
        P = torch.softmax(qq @ kk.transpose(-1, -2) * scale, -1)
        if mask is not None:
            P = P * (mask[b] != 0).double()[None, :, None]
        cols[b] = P.sum(1)
    return cols


def t2s_selector_qkv(Bm, n_t, n_s, H, pitch, seed=0):
    """(qkv [S][pitch][3C] fp32 with +-1 keys and q = 4 * k[target], tgt [Bm][H][2 n_t] key columns)."""
    S, C = 2 * Bm, H * D
    g = torch.Generator().manual_seed(3000 + 7 * n_t + n_s + seed)
    x = torch.zeros(S, pitch, 3, H, D)
    x[:, :, 1] = torch.randint(0, 2, (S, pitch, H, D), generator=g).float() * 2 - 1
    x[:, :, 2] = torch.randn(S, pitch, H, D, generator=g)
    order = probe_order([n_s, n_s])
    tgt = torch.zeros(Bm, H, 2 * n_t, dtype=torch.long)
    for b in range(Bm):
        for h in range(H):
            tgt[b, h] = order[((b * H + h) * 2 * n_t + torch.arange(2 * n_t)) % (2 * n_s)]
            kk = torch.cat([x[b, n_t:n_t + n_s, 1, h], x[b + Bm, n_t:n_t + n_s, 1, h]])
            x[b, :n_t, 0, h] = 4 * kk[tgt[b, h, :n_t]]
            x[b + Bm, :n_t, 0, h] = 4 * kk[tgt[b, h, n_t:]]
    return x.view(S, pitch, 3 * C), tgt


# ---- random inputs of the backward's per-row comparison ----------------------------------------------

# Per-row bars of the random-input backward comparison (row_rel_err of dQ, dK, dV): 4x the worst row of
# mam_bwd_emul against mam_bwd_ref over bwd_random_case at every shape of SHAPES (measured values in
# BWD_ROW_EMUL; test_attn_probes_host.py recomputes them).  (1, 1) is left out of this comparison alone: its
# template query has a single key, so its reference dQ row is exactly 0 (dS = P (dP - delta) cancels) and a
# relative row error is undefined there; the backward census covers that shape with absolute bounds.
BWD_RANDOM_SHAPES = [shape for shape in SHAPES if shape != (1, 1)]
BWD_ROW_EMUL = (0.00766, 0.01124, 0.00790)
BWD_ROW_BAR = tuple(4 * x for x in BWD_ROW_EMUL)


@functools.lru_cache(maxsize=None)
def bwd_random_case(n_t, n_s, S=BM, H=HEADS):
    """(qkv, dout) N(0, 1) rounded to bf16 (as fp32), one fixed seed per shape."""
    g = torch.Generator().manual_seed(4000 + 7 * n_t + n_s)
    ntok, C = n_t + n_s, H * D
    return _bf(torch.randn(S, ntok, 3 * C, generator=g)), _bf(torch.randn(S, ntok, C, generator=g))
