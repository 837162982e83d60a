"""mmt_mam_attention_tl (valid template rows per sequence, read from device memory) and mmt_patch_im2col_mem
(patch staging for 1 + K templates), on the smallest shapes that cross every edge: C = 128, H = 2, S = 4,
Bm = 2, n_s = 70 (the last key tile and the last query block are short), n_t in {128, 192, 144} (144: no
multiple of the 64-key tile, the ViT-L case), mixed lengths.

  compacted copy  the key walk with a length is that of a launch with n_t' = tl, so every written row equals,
                  bit for bit, mmt_mam_attention at the same forced impl on a copy that holds rows [0, tl) and
                  [n_t, ntok) back to back (per sequence; cross-modal search rows per pair of equal lengths)
  census          unequal lengths within a pair: tests/attn_probes.py's census (q = 0, v counts the keys), with
                  the reference's key lists cut to the lengths; bar as test_gpu_attention_probes.py (one
                  rounding to the storage type)
  poison          NaN in the rows [tl, n_t) of qkv never reaches a written row; skipped rows and sequences with
                  a length outside 1..n_t keep the sentinel
  contract        NULL lengths are mmt_mam_attention bit for bit; lse / impl 17 / impl 29 are MMT_EBADARG;
                  the staging at K = 1 is mmt_patch_im2col bit for bit, at K = 3 every pixel of every image
                  lands at its place (exact integer images)
"""
import functools

import pytest
import torch

import attn_probes as P
from attn_probes import DT, ULP

pytestmark = pytest.mark.gpu

S, BM, H, C, NS = 4, 2, 2, 128, 70
GUARD = 7.0
EBADARG = -10000  # MMT_EBADARG
KERNELS = [("f32", 0)] + [("bf16", i) for i in (4, 21, 22)] + [("fp16", i) for i in (4, 8)]
# n_t -> lengths of the four sequences: pair (1, 3) equal, pair (0, 2) unequal; full, aligned and unaligned values
LENS = {128: [64, 128, 16, 128], 192: [64, 128, 192, 128], 144: [16, 144, 80, 144]}
# lengths outside 1..n_t (sequences 0 and 2): those sequences, and with asym = 1 the pair's search rows, are skipped
DEAD = {128: [0, 128, 129, 64], 192: [-1, 64, 193, 192], 144: [0, 144, 145, 80]}
assert P.BM == BM and P.HEADS == H


def _lib():
    from mmt_amd import _lib
    return _lib


def _code(dname):
    L = _lib()
    return {"f32": L.MMT_F32, "bf16": L.MMT_BF16, "fp16": L.MMT_F16}[dname]


def _params(qd, out, n_t, asym, impl, q_part=0, bm=None, lse=None):
    L = _lib()
    p = L.AttnParams()
    nseq = qd.shape[0]
    p.qkv, p.out, p.S, p.Bm, p.ntok, p.n_t, p.C, p.H, p.asym = (
        qd.data_ptr(), out.data_ptr(), nseq, bm or max(1, nseq // 2), qd.shape[1], n_t, C, H, asym)
    p.scale, p.impl, p.lse, p.q_part = P.SCALE, impl, lse, q_part
    return p


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _attn(qd, n_t, dname, impl, asym, q_part=0, bm=None):
    """mmt_mam_attention on qd [nseq][ntok][3C]; out pre-filled with GUARD."""
    L = _lib()
    out = torch.full((qd.shape[0], qd.shape[1], C), GUARD, device="cuda", dtype=DT[dname])
    L.check(L.LIB.mmt_mam_attention(_params(qd, out, n_t, asym, impl, q_part, bm), _code(dname), _stream()), "attn")
    torch.cuda.synchronize()
    return out


def _attn_tl(qd, n_t, lens, dname, impl, asym, q_part=0):
    L = _lib()
    out = torch.full((qd.shape[0], qd.shape[1], C), GUARD, device="cuda", dtype=DT[dname])
    tl = torch.tensor(lens, dtype=torch.int32, device="cuda") if lens is not None else None
    rc = L.LIB.mmt_mam_attention_tl(_params(qd, out, n_t, asym, impl, q_part), tl.data_ptr() if tl is not None else None,
                                    _code(dname), _stream())
    L.check(rc, "attn_tl")
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _random_qkv(n_t, dname):
    g = torch.Generator().manual_seed(9100 + n_t)
    return torch.randn(S, n_t + NS, 3 * C, generator=g).to(DT[dname])


def _compact(q, seqs, tl, n_t):
    return torch.stack([torch.cat([q[s, :tl], q[s, n_t:]]) for s in seqs]).contiguous()


@pytest.mark.parametrize("n_t", sorted(LENS))
@pytest.mark.parametrize("asym", [0, 1])
@pytest.mark.parametrize("dname,impl", KERNELS)
def test_compacted_copy(dname, impl, asym, n_t):
    lens = LENS[n_t]
    qd = _random_qkv(n_t, dname).cuda()
    for q_part in (0, 1, 2):
        out = _attn_tl(qd, n_t, lens, dname, impl, asym, q_part)
        for s, tl in enumerate(lens):
            if q_part != 2:  # template rows: the sequence alone
                ref = _attn(_compact(qd, [s], tl, n_t), tl, dname, impl, 0, q_part=1)
                assert torch.equal(out[s, :tl], ref[0, :tl]), (q_part, s, "template rows")
            else:
                assert bool((out[s, :tl] == GUARD).all()), (q_part, s)
            assert bool((out[s, tl:n_t] == GUARD).all()), (q_part, s, "rows [tl, n_t) written")
            if q_part == 1:
                assert bool((out[s, n_t:] == GUARD).all()), (q_part, s)
            elif not asym:
                ref = _attn(_compact(qd, [s], tl, n_t), tl, dname, impl, 0, q_part=2)
                assert torch.equal(out[s, n_t:], ref[0, tl:]), (q_part, s, "search rows")
        if asym and q_part != 1:
            pairs = [(b, b + BM) for b in range(BM) if lens[b] == lens[b + BM]]
            assert pairs
            for sv, si in pairs:
                tl = lens[sv]
                ref = _attn(_compact(qd, [sv, si], tl, n_t), tl, dname, impl, 1, q_part=2, bm=1)
                assert torch.equal(out[sv, n_t:], ref[0, tl:]) and torch.equal(out[si, n_t:], ref[1, tl:]), (q_part, sv)


def _live(lens, n_t, asym):
    """(template rows live, search rows live) per sequence."""
    ok = [1 <= t <= n_t for t in lens]
    return ok, [ok[s] and (not asym or (ok[s % BM] and ok[s % BM + BM])) for s in range(S)]


@functools.lru_cache(maxsize=None)
def _census_ref(n_t, asym, dname, lens):
    """Census reference with every key list cut to the lengths (fp64), computed once per case."""
    qkv = P.census_qkv(n_t, NS)

    def edit(s, cls, seq, row):
        keep = (row >= n_t) | (row < torch.tensor(lens)[seq].clamp(0, n_t))
        return seq[keep], row[keep]

    ref, _ = P.mam_ref(qkv.to(DT[dname]), n_t, BM, H, asym, edit=edit)
    return qkv, ref


@pytest.mark.parametrize("table", ["mixed", "dead"])
@pytest.mark.parametrize("n_t", sorted(LENS))
@pytest.mark.parametrize("asym", [0, 1])
@pytest.mark.parametrize("dname,impl", KERNELS)
def test_census_unequal_lengths(dname, impl, asym, n_t, table):
    """n * out[j] counts the keys that were summed: per segment exactly the rows below that segment's own
    length (sV's, sI's, the sequence's own) and the search rows, each once."""
    lens = (LENS if table == "mixed" else DEAD)[n_t]
    qkv, ref = _census_ref(n_t, asym, dname, tuple(lens))
    out = _attn_tl(qkv.to(DT[dname]).cuda(), n_t, lens, dname, impl, asym).double().cpu()
    t_live, s_live = _live(lens, n_t, asym)
    for s, tl in enumerate(lens):
        for live, (a, b) in ((t_live[s], (0, max(0, min(tl, n_t)))), (s_live[s], (n_t, n_t + NS))):
            if live:
                bad = (out[s, a:b] - ref[s, a:b]).abs() > ULP[dname] * ref[s, a:b].abs()
                assert not bad.any(), (s, a, b, int(bad.sum()), tuple(bad.nonzero()[0].tolist()))
            else:
                assert bool((out[s, a:b] == GUARD).all()), (s, a, b, "dead rows written")
        a = max(0, min(tl, n_t)) if t_live[s] else 0
        assert bool((out[s, a:n_t] == GUARD).all()), (s, "rows [tl, n_t) written")


@pytest.mark.parametrize("table", ["mixed", "dead"])
@pytest.mark.parametrize("n_t", sorted(LENS))
@pytest.mark.parametrize("asym", [0, 1])
@pytest.mark.parametrize("dname,impl", KERNELS)
def test_poisoned_rows(dname, impl, asym, n_t, table):
    lens = (LENS if table == "mixed" else DEAD)[n_t]
    clean = _random_qkv(n_t, dname).clone()
    poison = clean.clone()
    for s, tl in enumerate(lens):
        a = max(0, min(tl, n_t))
        clean[s, a:n_t] = 0
        poison[s, a:n_t] = float("nan")
    for q_part in (0, 1, 2):
        out = _attn_tl(poison.cuda(), n_t, lens, dname, impl, asym, q_part)
        assert not bool(torch.isnan(out).any()), q_part
        assert torch.equal(out, _attn_tl(clean.cuda(), n_t, lens, dname, impl, asym, q_part)), q_part
        t_live, s_live = _live(lens, n_t, asym)
        for s, tl in enumerate(lens):
            a = tl if t_live[s] and q_part != 2 else 0
            assert bool((out[s, a:n_t] == GUARD).all()), (q_part, s)
            if not s_live[s] or q_part == 1:
                assert bool((out[s, n_t:] == GUARD).all()), (q_part, s)
            else:
                assert not bool((out[s, n_t:] == GUARD).all(-1).any()), (q_part, s, "live search row not written")
            if a:
                assert not bool((out[s, :a] == GUARD).all(-1).any()), (q_part, s, "live template row not written")


@pytest.mark.parametrize("asym", [0, 1])
@pytest.mark.parametrize("dname,impl", KERNELS + [("bf16", 0), ("bf16", 8), ("bf16", 17), ("fp16", 0)])
def test_null_lengths_are_the_old_entry_point(dname, impl, asym):
    qd = _random_qkv(144, dname).cuda()
    for q_part in (0, 1, 2):
        assert torch.equal(_attn_tl(qd, 144, None, dname, impl, asym, q_part), _attn(qd, 144, dname, impl, asym, q_part))


def test_rejected_arguments():
    L = _lib()
    n_t = 128
    qd = _random_qkv(n_t, "bf16").cuda()
    out = torch.full((S, n_t + NS, C), GUARD, device="cuda", dtype=torch.bfloat16)
    tl = torch.tensor(LENS[n_t], dtype=torch.int32, device="cuda")
    lse = torch.zeros(S, H, n_t + NS, device="cuda")
    call = lambda p, dt=L.MMT_BF16: L.LIB.mmt_mam_attention_tl(p, tl.data_ptr(), dt, _stream())  # noqa: E731
    assert call(_params(qd, out, n_t, 0, 21)) == 0
    assert call(_params(qd, out, n_t, 0, 21, lse=lse.data_ptr())) == EBADARG
    assert call(_params(qd, out, n_t, 0, 0, lse=lse.data_ptr())) == EBADARG
    for impl in (17, 29, 23, 5):
        assert call(_params(qd, out, n_t, 0, impl)) == EBADARG, impl
    assert call(_params(qd, out, n_t, 0, 21), L.MMT_F16) == EBADARG  # fp16 has no range-checked kernel
    assert L.LIB.mmt_mam_attention_tl(None, tl.data_ptr(), L.MMT_BF16, _stream()) == EBADARG
    torch.cuda.synchronize()
    out.fill_(GUARD)
    torch.cuda.synchronize()
    assert call(_params(qd, out, n_t, 0, 17)) == EBADARG
    torch.cuda.synchronize()
    assert bool((out == GUARD).all()), "a rejected call launched"


# ---- patch staging ----------------------------------------------------------------------------------

def _rows(img, patch):
    """[3][hw][hw] -> [(hw/patch)^2][3 patch^2], rows = (c, ky, kx) of each patch in raster order."""
    g = img.shape[-1] // patch
    return img.unfold(1, patch, patch).unfold(2, patch, patch).permute(1, 2, 0, 3, 4).reshape(g * g, 3 * patch * patch)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _stage_mem(t, o, s, K, ht, hs, patch, dname, nmod, bm):
    L = _lib()
    ntok = (1 + K) * (ht // patch) ** 2 + (hs // patch) ** 2
    out = torch.full((nmod * bm, ntok, 3 * patch * patch), GUARD, device="cuda", dtype=DT[dname])
    t1, o1, s1 = (x[1] if nmod == 2 else None for x in (t, o, s))
    L.check(L.LIB.mmt_patch_im2col_mem(t[0].data_ptr(), _ptr(t1), o[0].data_ptr(), _ptr(o1), s[0].data_ptr(), _ptr(s1),
                                       out.data_ptr(), bm, K, ht, hs, patch, _code(dname), _stream()), "im2col_mem")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("nmod", [1, 2])
@pytest.mark.parametrize("dname", ["f32", "bf16", "fp16"])
def test_staging_one_online_template_is_patch_im2col(dname, nmod):
    L = _lib()
    bm, ht, hs, patch = 3, 32, 48, 16
    g = torch.Generator().manual_seed(77)
    t, o, s = ([torch.randn(bm, 3, hw, hw, generator=g).cuda() for _ in range(nmod)] for hw in (ht, ht, hs))
    got = _stage_mem(t, [x.view(bm, 1, 3, ht, ht) for x in o], s, 1, ht, hs, patch, dname, nmod, bm)
    ref = torch.full_like(got, GUARD)
    t1, o1, s1 = (x[1] if nmod == 2 else None for x in (t, o, s))
    L.check(L.LIB.mmt_patch_im2col(t[0].data_ptr(), _ptr(t1), o[0].data_ptr(), _ptr(o1), s[0].data_ptr(), _ptr(s1),
                                   ref.data_ptr(), bm, ht, hs, patch, _code(dname), _stream()), "im2col")
    torch.cuda.synchronize()
    assert torch.equal(got, ref)


@pytest.mark.parametrize("dname,mod", [("f32", 1 << 24), ("bf16", 256), ("fp16", 2048)])
def test_staging_three_online_templates_every_pixel(dname, mod):
    """Every pixel of every image carries its own integer (modulo the storage type's exact range; fp32: none
    repeats), so a row from a wrong image, slot, batch element, channel or offset shows."""
    bm, K, ht, hs, patch = 2, 3, 32, 48, 16
    nt, ns = (ht // patch) ** 2, (hs // patch) ** 2
    base = [0]

    def images(*shape):
        n = int(torch.tensor(shape).prod())
        x = (torch.arange(base[0], base[0] + n) % mod).float().view(*shape)
        base[0] += n
        return x

    t = [images(bm, 3, ht, ht) for _ in range(2)]
    o = [images(bm, K, 3, ht, ht) for _ in range(2)]
    s = [images(bm, 3, hs, hs) for _ in range(2)]
    assert base[0] < (1 << 24)
    got = _stage_mem([x.cuda() for x in t], [x.cuda() for x in o], [x.cuda() for x in s], K, ht, hs, patch, dname, 2, bm)
    got = got.float().cpu()
    assert got.shape[1] == (1 + K) * nt + ns
    for m in range(2):
        for b in range(bm):
            row = got[m * bm + b]
            assert torch.equal(row[:nt], _rows(t[m][b], patch)), (m, b, "template")
            for k in range(K):
                assert torch.equal(row[(1 + k) * nt:(2 + k) * nt], _rows(o[m][b, k], patch)), (m, b, k)
            assert torch.equal(row[(1 + K) * nt:], _rows(s[m][b], patch)), (m, b, "search")


def test_staging_rejected_arguments():
    L = _lib()
    x = torch.zeros(1, 3, 32, 32, device="cuda")
    out = torch.zeros(1, 12, 768, device="cuda")
    call = lambda **kw: L.LIB.mmt_patch_im2col_mem(  # noqa: E731
        kw.get("t", x.data_ptr()), None, x.data_ptr(), None, x.data_ptr(), None, out.data_ptr(), kw.get("bm", 1),
        kw.get("K", 1), kw.get("ht", 32), 32, kw.get("patch", 16), kw.get("dt", L.MMT_F32), _stream())
    assert call() == 0
    for bad in (dict(K=0), dict(bm=0), dict(ht=40), dict(patch=6), dict(patch=0), dict(t=None), dict(dt=99)):
        assert call(**bad) == EBADARG, bad
    torch.cuda.synchronize()
