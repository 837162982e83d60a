"""Kernel level of the template-cached candidate elimination and of its fp16 form.

* mmt_ce_rows_gather_cast (the packed typed row gather) against torch.gather on the CPU: the fp32 rows
  bit-identical, the typed copy bit-identical to `.to(dtype)` of them, zero rows exactly where the index
  is -1 or out of range (the source is NaN behind its last row: an index that were dereferenced would
  show), guard rows around both destinations untouched; and one call on mmt_ce_index_invert of a golden
  forward's final gidx equals mmt_ce_recover.
* mmt_ce_t2s_attention_masked + mmt_ce_select in fp16, with the bf16 and fp32 kernels as controls, on
  operands rounded to the type, against a float64 computation on the same rounded operands:
  max|err| / max|ref| <= 1e-5 (the bound tests/test_gpu_ce.py holds the fp32 path to; the MFMA forms add
  exact 16-bit products in fp32, so it is theirs too), and the kept order equals torch.sort's wherever
  adjacent means differ by more than 1e-4 relative.  Rows of the qkv stream past n_t + k are NaN.
  (The mask with the first 16 queries off needs more than 16 queries: it runs for n_t = 128 only.)
* The attention at the cached pass's geometry after a pruning stage (q_part 2, tok_pitch > ntok, compact
  out rows) equals, bit for bit, the search rows of the full launch on the same rows packed; the cache
  rows past n_t + keep are NaN."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": (torch.bfloat16, 1), "f16": (torch.float16, 3), "f32": (torch.float32, 0)}


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------ packed gather
def _guarded(rows, C, dtype, sentinel):
    """rows + 2 rows of `sentinel`; returns (buffer, pointer to row 1)."""
    buf = torch.full((rows + 2, C), sentinel, dtype=dtype, device="cuda")
    return buf, buf.data_ptr() + C * buf.element_size()


def _gather_case(src_rows, dst_rows, S, seed):
    """Index rows of a case: a pruning order (distinct rows) or, with more destination than source rows, the
    inverse of a kept set (-1 where pruned); plus a few entries out of range on either side."""
    g = torch.Generator().manual_seed(seed)
    if dst_rows <= src_rows:
        idx = torch.stack([torch.randperm(src_rows, generator=g)[:dst_rows] for _ in range(S)]).int()
    else:
        idx = torch.full((S, dst_rows), -1, dtype=torch.int32)
        for s in range(S):
            pos = torch.randperm(dst_rows, generator=g)[:src_rows]
            idx[s, pos] = torch.arange(src_rows, dtype=torch.int32)
    idx[0, 1], idx[S - 1, 2], idx[S - 1, dst_rows - 1], idx[1, 0] = src_rows, src_rows + 3, src_rows, -5
    return idx


@pytest.mark.parametrize("dname", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("src_rows,dst_rows,pitch", [(9, 7, 0), (400, 280, 400), (196, 138, 400), (138, 400, 0)])
@pytest.mark.parametrize("C", [4, 768, 1024])
def test_rows_gather_cast_matches_torch_gather(C, src_rows, dst_rows, pitch, dname):
    from mmt_amd._lib import LIB, check
    S = 4
    dt, code = DTYPES[dname]
    g = torch.Generator().manual_seed(C + src_rows)
    x = torch.randn(S, src_rows, C, generator=g) * 3.0
    tail = torch.full((8, C), float("nan"))  # behind the last sequence's last row
    xd = torch.cat([x.view(-1, C), tail]).cuda()
    idx = _gather_case(src_rows, dst_rows, S, C + dst_rows)
    ip = pitch or dst_rows
    idx_p = torch.full((S, ip), 0, dtype=torch.int32)  # entries past dst_rows: never read (valid rows, nonzero data)
    idx_p[:, :dst_rows] = idx
    idx_d = idx_p.cuda()
    live = (idx >= 0) & (idx < src_rows)
    ref = torch.gather(x, 1, idx.clamp(0, src_rows - 1).long()[:, :, None].expand(-1, -1, C))
    ref = torch.where(live[:, :, None], ref, torch.zeros(()))
    ref_t = ref.to(dt)
    for with_f32, with_t in ((True, True), (False, True), (True, False)):
        fb, fp = _guarded(S * dst_rows, C, torch.float32, -77.0)
        tb, tp = _guarded(S * dst_rows, C, dt, -77.0)
        check(LIB.mmt_ce_rows_gather_cast(xd.data_ptr(), src_rows, fp if with_f32 else None, tp if with_t else None,
                                          dst_rows, idx_d.data_ptr(), pitch, S, C, code, _stream()), "rows_gather_cast")
        torch.cuda.synchronize()
        for buf, on, want in ((fb, with_f32, ref), (tb, with_t, ref_t)):
            got = buf.cpu()
            assert bool((got[0] == -77.0).all()) and bool((got[-1] == -77.0).all())  # guard rows
            body = got[1:-1].view(S, dst_rows, C)
            if not on:
                assert bool((body == -77.0).all())
                continue
            iv = {4: torch.int32, 2: torch.int16}[body.element_size()]
            assert torch.equal(body.view(iv), want.view(iv))  # bit for bit (and finite: no NaN row was read)
            assert bool((body[~live] == 0).all()) and bool(live.any())


@pytest.mark.parametrize("dname", ["bf16", "f16", "f32"])
def test_rows_gather_cast_recovery_equals_ce_recover(dname):
    """The final gidx of the golden forward (B = 2): one gather through its inverse == mmt_ce_recover."""
    from mmt_amd._lib import LIB, check
    gold = np.load(GOLDEN + "/model_asym_ce_b2.npz")
    kv, ki = gold["ce2_keep_v"], gold["ce2_keep_i"]
    B, keep = kv.shape
    S, n_t, ns, C = 2 * B, 128, 400, 768
    pitch = n_t + ns
    dt, code = DTYPES[dname]
    gidx = torch.full((S, ns), -1, dtype=torch.int32)
    gidx[:, :keep] = torch.from_numpy(np.concatenate([kv, ki]).astype(np.int32))
    gd = gidx.cuda()
    x = (torch.randn(S, pitch, C, generator=torch.Generator().manual_seed(4)) * 2.0).cuda()
    out = torch.full((S, pitch, C), 5.0, dtype=dt, device="cuda")
    check(LIB.mmt_ce_recover(x.data_ptr(), gd.data_ptr(), keep, out.data_ptr(), S, pitch, n_t, ns, C, code, _stream()),
          "ce_recover")
    packed = x[:, n_t:n_t + keep].contiguous()
    inv = torch.full((S, ns), -9, dtype=torch.int32, device="cuda")
    got = torch.full((S, ns, C), 5.0, dtype=dt, device="cuda")
    check(LIB.mmt_ce_index_invert(gd.data_ptr(), ns, inv.data_ptr(), ns, S, _stream()), "ce_index_invert")
    check(LIB.mmt_ce_rows_gather_cast(packed.data_ptr(), keep, None, got.data_ptr(), ns, inv.data_ptr(), 0, S, C, code,
                                      _stream()), "rows_gather_cast")
    torch.cuda.synchronize()
    assert int((inv >= 0).sum()) == S * keep
    assert torch.equal(got, out[:, n_t:])
    assert int((got.float().abs().sum(2) == 0).sum()) == S * (ns - keep)


# ------------------------------------------------------------------ t2s probe
def _t2s_cases():
    out = []
    for dname in ("f16", "bf16", "f32"):
        for n_t in (8, 128):
            for k in (8, 9, 138, 576):
                for mask in ("none", "first16off", "four"):
                    if mask == "first16off" and 2 * n_t <= 16:
                        continue  # would leave no query
                    out.append((dname, n_t, k, mask))
    return out


@pytest.mark.parametrize("dname,n_t,k,mask", _t2s_cases())
def test_t2s_attention_mean_and_order(dname, n_t, k, mask):
    from mmt_amd._lib import LIB, check
    H, C, Bm = 2, 128, 2
    S, pitch, scale = 2 * Bm, n_t + k + 5, 0.125
    dt, code = DTYPES[dname]
    g = torch.Generator().manual_seed(1000 * n_t + k)
    qkv = (torch.randn(S, pitch, 3 * C, generator=g) * 0.5).to(dt)
    qkv[:, n_t + k:] = float("nan")  # rows past the stage's tokens: never read
    nq_all = 2 * n_t
    m = torch.ones(Bm, nq_all, dtype=torch.uint8)
    if mask == "first16off":
        m[:, :16] = 0
    elif mask == "four":
        m[:] = 0
        for b in range(Bm):
            m[b, torch.randperm(nq_all, generator=g)[:4]] = 1
    nq = int(m[0].sum())
    # float64 reference on the rounded operands: queries [q_mt_V ; q_mt_I], keys [k_s_V | k_s_I]
    x = qkv.double().view(2, Bm, pitch, 3, H, 64)
    q = torch.cat([x[0, :, :n_t, 0], x[1, :, :n_t, 0]], 1).permute(0, 2, 1, 3)               # [Bm][H][2 n_t][64]
    kk = torch.cat([x[0, :, n_t:n_t + k, 1], x[1, :, n_t:n_t + k, 1]], 1).permute(0, 2, 1, 3)  # [Bm][H][2 k][64]
    att = torch.softmax(q @ kk.transpose(-1, -2) * scale, -1)
    ref = (att * m.double()[:, None, :, None]).sum((1, 2)) / (H * nq)                         # [Bm][2 k]
    qb = 8 if dname == "f32" else 16
    nparts = H * (nq_all // qb)
    part = torch.full((Bm * nparts * 2 * k,), float("nan"), device="cuda")
    qd, md = qkv.cuda(), m.cuda()
    check(LIB.mmt_ce_t2s_attention_masked(qd.data_ptr(), part.data_ptr(), None if mask == "none" else md.data_ptr(), Bm,
                                          pitch, n_t, k, C, H, scale, code, _stream()), "ce_t2s")
    keep = math.ceil(0.7 * k)
    gout = torch.full((S, k), -7, dtype=torch.int32, device="cuda")
    order = torch.full_like(gout, -7)
    mean = torch.full((Bm, 2 * k), float("nan"), device="cuda")
    check(LIB.mmt_ce_select(part.data_ptr(), nparts, Bm, k, keep, k, None, gout.data_ptr(), order.data_ptr(),
                            mean.data_ptr(), 1.0 / (H * nq), _stream()), "ce_select")
    torch.cuda.synchronize()
    err = ((mean.cpu().double() - ref).abs().max() / ref.abs().max()).item()
    print("t2s %s n_t=%d k=%d mask=%s: max|err|/max|ref| %.3g" % (dname, n_t, k, mask, err))
    assert err <= 1e-5, err
    checked = 0
    for s in range(S):
        mo, b = s // Bm, s % Bm
        v, ri = torch.sort(ref[b, mo * k:(mo + 1) * k], descending=True)
        gap = (v[:-1] - v[1:]) > 1e-4 * v[:-1]  # gap[r]: between ranks r and r + 1
        clear = torch.ones(k, dtype=torch.bool)
        clear[:-1] &= gap
        clear[1:] &= gap
        clear = clear[:keep]
        got = order[s, :keep].cpu().long()
        assert torch.equal(got[clear], ri[:keep][clear]), (s, int(clear.sum()))
        assert torch.equal(gout[s, :keep].cpu().long(), got)  # identity start
        checked += int(clear.sum())
    assert checked > 0


# ------------------------------------------------------------------ attention at the cached CE geometry
@pytest.mark.parametrize("dname,impl", [("bf16", i) for i in (0, 4, 8, 17, 21, 22)] + [("f16", i) for i in (0, 4, 8)])
def test_attention_cached_ce_geometry_bit_exact(dname, impl):
    from mmt_amd._lib import LIB, AttnParams, check
    S, pitch, n_t, H, keep = 2, 528, 128, 12, 138
    ntok, C = n_t + keep, 64 * H
    dt, code = DTYPES[dname]
    qkv = (torch.randn(S, pitch, 3 * C, generator=torch.Generator().manual_seed(5)) * 0.5).to(dt)
    packed = qkv[:, :ntok].contiguous().cuda()
    qkv[:, ntok:] = float("nan")  # what an earlier frame left in the cache: stale
    qkv = qkv.cuda()

    def run(src, out, **kw):
        p = AttnParams()
        p.qkv, p.out, p.S, p.Bm, p.ntok, p.n_t, p.C, p.H, p.asym = src.data_ptr(), out.data_ptr(), S, 1, ntok, n_t, C, H, 1
        p.scale, p.impl = 0.125, impl
        for name, val in kw.items():
            setattr(p, name, val)
        check(LIB.mmt_mam_attention(ctypes.byref(p), code, _stream()), "attn")
        torch.cuda.synchronize()
        return out
    full = run(packed, torch.full((S, ntok, C), 7.0, device="cuda", dtype=dt))
    out = torch.full((S * keep + 3, C), 7.0, device="cuda", dtype=dt)  # 3 guard rows behind the last sequence
    run(qkv, out, q_part=2, tok_pitch=pitch, out_pitch=keep, out_q0=n_t)
    assert torch.equal(out[:S * keep].view(S, keep, C), full[:, n_t:])
    assert bool(torch.isfinite(out.float()).all()) and bool((out[S * keep:] == 7.0).all())
