"""Probe inputs and fp64 references of the cross-modal (asym = 1) MAM attention backward (no tests here).

The geometry is attn_probes' (BM = 2, HEADS = 2, SHAPES, key_index(..., asym=1)): S = 2 BM sequences, RGB first;
template queries of sequence s attend the template keys of s, search queries attend
[template of s % BM | template of s % BM + BM | own search].  Hence a template key of sequence (m, b) is attended by
three query groups -- its own template queries, the search queries of sequence b and those of b + BM -- and a search
key by the search queries of its own sequence only.

  mam_asym_bwd_ref    dqkv in fp64 by explicit formulas over the key lists, and the elementwise bound of dQ
                      (attn_probes.mam_bwd_ref's formula: 2^-7 scale sum_k A_qk |k_k|)
  mam_asym_bwd_emul   the arithmetic attention_bwd.hip documents (bf16 q', P, dS; fp32 sums; bf16 outputs)
  attend_weights      W[query, key] = 1 / n_q where the query attends the key: with the census qkv (q = 0, so P is
                      uniform and fixed by the forward's lse) dV = W^T dout exactly; the host test edits W to build
                      the wrong references
  census_dout         the backward census' dout, which depends on the sequence so that a query group read from the
                      wrong sequence shows

ASYM_BWD_ROW_EMUL / ASYM_BWD_ROW_BAR: the per-row bars of the random-input comparison, derived below.
"""
import functools
import math

import torch

import attn_probes as P
from attn_probes import BM, D, HEADS, LOG2E, SCALE

S = 2 * BM


def search_gain(n_t, n_s):
    """g: the power of two nearest (2 n_t + n_s) / n_t, the ratio of a search query's key count to a template
    query's, so that both kinds of query give a template key's dV comparable shares."""
    return 2.0 ** round(math.log2((2 * n_t + n_s) / n_t))


def census_weight(s, q, n_t, n_s):
    """w_s(q) = (32 + q // 64 + 4 s) g(q), g = 1 for template queries and search_gain for search queries: at most
    53 * 32, a 6-bit integer times a power of two, exact in bf16; distinct for every sequence at one query."""
    return (32 + q // 64 + 4 * s) * torch.where(q < n_t, 1.0, search_gain(n_t, n_s))


def census_dout(n_t, n_s, H=HEADS):
    """[S][ntok][C] fp32: dout[s, q, h, j] = w_s(q) * [j == q % 64]."""
    ntok = n_t + n_s
    q = torch.arange(ntok)
    e = torch.zeros(S, ntok, D)
    for s in range(S):
        e[s, q, q % 64] = census_weight(s, q, n_t, n_s).float()
    return e[:, :, None, :].expand(S, ntok, H, D).reshape(S, ntok, H * D)


def attend_weights(n_t, n_s, Bm=BM):
    """W [S ntok (query)][S ntok (key)] fp64: 1 / n_q where query (s, q) attends key (seq, row), else 0, from
    key_index(..., asym=1); n_q = n_t for template and 2 n_t + n_s for search queries."""
    ntok = n_t + n_s
    W = torch.zeros(2 * Bm * ntok, 2 * Bm * ntok, dtype=torch.float64)
    for s in range(2 * Bm):
        for cls, (qa, qb) in enumerate(((0, n_t), (n_t, ntok))):
            seq, row = P.key_index(s, cls, n_t, n_s, Bm, 1)
            W[s * ntok + qa:s * ntok + qb, seq * ntok + row] = 1.0 / len(row)
    return W


def census_dv(W, dout):
    """dV [S][ntok][C] fp64 of the census (P = W) for dout [S][ntok][C]: every head has the same P."""
    return (W.t() @ dout.double().reshape(-1, dout.shape[-1])).view(dout.shape)


def mam_asym_bwd_ref(qkv, dout, n_t, Bm=BM, H=HEADS, scale=SCALE):
    """dqkv [S][ntok][3C] of the cross-modal MAM attention in fp64 and the elementwise bound of the bf16 kernels'
    dQ error (see attn_probes.mam_bwd_ref).  dK / dV of a key are summed over every query list that holds it."""
    q, k, v = P.split_heads(qkv, H)
    nseq, ntok = qkv.shape[:2]
    do = dout.double().view(nseq, ntok, H, D).permute(0, 2, 1, 3)
    dq, bound = (torch.zeros(nseq, H, ntok, D, dtype=torch.float64) for _ in range(2))
    dk, dv = (torch.zeros(nseq * ntok, H, D, dtype=torch.float64) for _ in range(2))
    for s, cls, qa, qb, seq, row, sc in P.mam_classes(qkv, n_t, Bm, H, 1, scale):
        Pm = torch.softmax(sc, -1)
        kk, vv, dO = k[seq, :, row].permute(1, 0, 2), v[seq, :, row].permute(1, 0, 2), do[s, :, qa:qb]
        dP = dO @ vv.transpose(-1, -2)
        O = Pm @ vv
        dS = Pm * (dP - (dO * O).sum(-1, keepdim=True))
        dq[s, :, qa:qb] = scale * dS @ kk
        dk.index_add_(0, seq * ntok + row, (scale * dS.transpose(-1, -2) @ q[s, :, qa:qb]).permute(1, 0, 2))
        dv.index_add_(0, seq * ntok + row, (Pm.transpose(-1, -2) @ dO).permute(1, 0, 2))
        A = Pm * (dP.abs() + (dO * O).abs().sum(-1, keepdim=True))
        bound[s, :, qa:qb] = 2.0 ** -7 * scale * A @ kk.abs()
    C = H * D
    return torch.cat([P.merge_heads(dq), dk.view(nseq, ntok, C), dv.view(nseq, ntok, C)], -1), P.merge_heads(bound)


def _bf(x):
    return x.bfloat16().float()


def mam_asym_bwd_emul(qkv, dout, n_t, Bm=BM, H=HEADS, scale=SCALE):
    """attn_probes.mam_bwd_emul for the cross-modal key lists: q' = bf16(q scale log2 e); the forward's P rounded
    to bf16 for the row sums and O, lse = log2 of those sums, O stored in bf16; P = exp2(q'.k - lse); delta from
    the bf16 dO and O; dS and (for dV) P rounded to bf16; fp32 sums over every query list of a key; dQ =
    bf16(scale dS k), dK = bf16(dS^T q' / log2 e), dV = bf16(P^T dO): each rounded to bf16 once."""
    x = qkv.bfloat16().float()
    nseq, ntok = x.shape[:2]
    n_s = ntok - n_t
    q, k, v = x.view(nseq, ntok, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)
    do = dout.bfloat16().float().view(nseq, ntok, H, D).permute(0, 2, 1, 3)
    qs = _bf(q * (scale * LOG2E))
    dq = torch.zeros(nseq, H, ntok, D)
    dk, dv = (torch.zeros(nseq * ntok, H, D) for _ in range(2))
    for s in range(nseq):
        for cls, (qa, qb) in enumerate(((0, n_t), (n_t, ntok))):
            seq, row = P.key_index(s, cls, n_t, n_s, Bm, 1)
            kk, vv = k[seq, :, row].permute(1, 0, 2), v[seq, :, row].permute(1, 0, 2)
            s2 = qs[s, :, qa:qb] @ kk.transpose(-1, -2)
            m = s2.max(-1, keepdim=True)[0]
            pf = _bf(torch.exp2(s2 - m))
            l = pf.sum(-1, keepdim=True)
            O = _bf(pf @ vv / l)
            Pm = torch.exp2(s2 - (m + torch.log2(l)))
            dO = do[s, :, qa:qb]
            dS = _bf(Pm * (dO @ vv.transpose(-1, -2) - (dO * O).sum(-1, keepdim=True)))
            dq[s, :, qa:qb] = dS @ kk * scale
            dk.index_add_(0, seq * ntok + row, (dS.transpose(-1, -2) @ qs[s, :, qa:qb] / LOG2E).permute(1, 0, 2))
            dv.index_add_(0, seq * ntok + row, (_bf(Pm).transpose(-1, -2) @ dO).permute(1, 0, 2))
    C = H * D
    return _bf(torch.cat([P.merge_heads(dq), dk.view(nseq, ntok, C), dv.view(nseq, ntok, C)], -1))


# Per-row bars of the random-input comparison (attn_probes.row_rel_err of dQ, dK, dV), by the project's rule for
# BWD_ROW_BAR: 4x the worst row of mam_asym_bwd_emul against mam_asym_bwd_ref over random_case at every shape of
# BWD_RANDOM_SHAPES.  ASYM_BWD_ROW_EMUL holds those worst rows as the CPU emulation gives them
# (test_attn_asym_bwd_host.py recomputes them); nothing here comes from the kernels.
ASYM_BWD_ROW_EMUL = (0.00823, 0.01083, 0.00813)
ASYM_BWD_ROW_BAR = tuple(4 * x for x in ASYM_BWD_ROW_EMUL)


def random_case(n_t, n_s):
    """(qkv, dout) as attn_probes.bwd_random_case draws them, for 2 BM sequences."""
    return P.bwd_random_case(n_t, n_s, S)


@functools.lru_cache(maxsize=None)
def census_case(n_t, n_s):
    """(qkv, dout, fp64 dqkv, dQ bound) of the backward census at one shape, computed once and shared (read-only)."""
    qkv, dout = P.census_qkv(n_t, n_s).bfloat16().float(), census_dout(n_t, n_s)
    return (qkv, dout) + mam_asym_bwd_ref(qkv, dout, n_t)


@functools.lru_cache(maxsize=None)
def random_ref(n_t, n_s):
    """(qkv, dout, fp64 dqkv, dQ bound) of the random case at one shape, computed once and shared (read-only)."""
    qkv, dout = random_case(n_t, n_s)
    return (qkv, dout) + mam_asym_bwd_ref(qkv, dout, n_t)
