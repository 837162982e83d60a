"""The cross-rank batch norm's HIP phases (mmt_batchnorm_sync_stats / _apply / _bwd_sums / _bwd_dx) through ctypes
on one GPU: virtual ranks (the gathered buffer concatenated and the backward sums added on the device where the
collectives would run) against nn.BatchNorm2d in fp64 on the concatenated batch, and one forced rank against the
local mmt_batchnorm_relu / _bwd bitwise."""
import math

import pytest
import torch

from syncbn_ref import full_batch_reference

pytestmark = pytest.mark.gpu

MOM, EPS = 0.1, 1e-5


def _lib():
    from mmt_amd import _lib as L
    return L


def _st():
    return torch.cuda.current_stream().cuda_stream


def _pad(t, pitch, g):
    """[..][C] -> [..][pitch] bf16 on the GPU; the padding channels carry junk (the kernels must ignore it)."""
    C = t.shape[-1]
    if pitch != C:
        t = torch.cat([t, torch.randn(*t.shape[:-1], pitch - C, generator=g)], -1)
    return t.bfloat16().cuda().contiguous()


def _case(batches, H, C):
    """Per-rank bf16-rounded maps with mean 4r - 3 and std 1 + r, bf16 dy, non-trivial affine and running statistics."""
    g = torch.Generator().manual_seed(sum(batches) * H + C)
    pitch = (C + 7) // 8 * 8
    xs = [(torch.randn(b, H, H, C, generator=g) * (1 + r) + (4 * r - 3)).bfloat16().float() for r, b in enumerate(batches)]
    dys = [torch.randn(b, H, H, C, generator=g).bfloat16().float() for b in batches]
    par = {"weight": torch.rand(C, generator=g) + 0.5, "bias": torch.randn(C, generator=g) * 0.3,
           "running_mean": torch.randn(C, generator=g) * 0.1, "running_var": torch.rand(C, generator=g) + 0.5}
    xp, dyp = [_pad(x, pitch, g) for x in xs], [_pad(d, pitch, g) for d in dys]
    return xs, dys, par, xp, dyp, pitch


def _stats(x, C):
    L = _lib()
    pitch = x.shape[-1]
    M = x.numel() // pitch
    st = torch.empty(3, C, device="cuda", dtype=torch.float64)
    nws = int(L.LIB.mmt_batchnorm_ws_floats(M, C))
    ws = torch.empty(nws, device="cuda")
    L.check(L.LIB.mmt_batchnorm_sync_stats(x.data_ptr(), M, C, pitch, st.data_ptr(), ws.data_ptr(), nws, _st()), "stats")
    return st


def _apply(x, C, gathered, W, par):
    L = _lib()
    pitch = x.shape[-1]
    M = x.numel() // pitch
    y = torch.empty_like(x)
    save = torch.empty(4, C, device="cuda")
    n_total = torch.zeros(1, device="cuda", dtype=torch.float64)
    w, b = par["weight"].cuda(), par["bias"].cuda()
    rm, rv = par["running_mean"].cuda(), par["running_var"].cuda()  # this rank's own clone
    L.check(L.LIB.mmt_batchnorm_sync_apply(x.data_ptr(), y.data_ptr(), M, C, pitch, gathered.data_ptr(), W, w.data_ptr(),
                                           b.data_ptr(), rm.data_ptr(), rv.data_ptr(), MOM, EPS, 1, save.data_ptr(),
                                           n_total.data_ptr(), _st()), "apply")
    return y, save, rm, rv, n_total


def _bwd_sums(x, dy, C, save):
    L = _lib()
    pitch = x.shape[-1]
    M = x.numel() // pitch
    dgb = torch.empty(2, C, device="cuda")
    sums = torch.empty(2, C, device="cuda", dtype=torch.float64)
    nws = int(L.LIB.mmt_batchnorm_ws_floats(M, C))
    ws = torch.empty(nws, device="cuda")
    L.check(L.LIB.mmt_batchnorm_sync_bwd_sums(x.data_ptr(), dy.data_ptr(), M, C, pitch, save.data_ptr(), 1, dgb.data_ptr(),
                                              sums.data_ptr(), ws.data_ptr(), nws, _st()), "bwd_sums")
    return dgb, sums


def _bwd_dx(x, dy, C, par, save, sums, n_total):
    L = _lib()
    pitch = x.shape[-1]
    M = x.numel() // pitch
    dx = torch.empty_like(x)
    w = par["weight"].cuda()
    ws = torch.empty(3 * C, device="cuda")
    L.check(L.LIB.mmt_batchnorm_sync_bwd_dx(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), M, C, pitch, w.data_ptr(),
                                            save.data_ptr(), sums.data_ptr(), n_total.data_ptr(), 1, ws.data_ptr(), 3 * C,
                                            _st()), "bwd_dx")
    return dx


def _virtual(xp, dyp, C, par, no_exchange=False):
    """The four phases on W virtual ranks.  no_exchange: every rank's slot of the gathered buffer carries rank 0's
    triple (what a missing all-gather would look like)."""
    W = len(xp)
    triples = [_stats(x, C) for x in xp]
    gathered = torch.cat([triples[0] if no_exchange else t for t in triples])  # [W * 3][C], where the all-gather would
    fwd = [_apply(x, C, gathered, W, par) for x in xp]
    bs = [_bwd_sums(x, dy, C, f[1]) for x, dy, f in zip(xp, dyp, fwd)]
    total = torch.stack([s for _, s in bs]).sum(0)  # where the all-reduce would
    dxs = [_bwd_dx(x, dy, C, par, f[1], total, f[4]) for x, dy, f in zip(xp, dyp, fwd)]
    torch.cuda.synchronize()
    return {"y": [f[0] for f in fwd], "save": [f[1] for f in fwd], "rm": [f[2] for f in fwd], "rv": [f[3] for f in fwd],
            "n": [f[4] for f in fwd], "dgb": [b[0] for b in bs], "dx": dxs}


def _local(x, dy, C, par):
    """The parent's single-rank path on one map: (y, save, rm, rv, dx, dgb)."""
    L = _lib()
    pitch = x.shape[-1]
    M = x.numel() // pitch
    y, dx = torch.empty_like(x), torch.empty_like(x)
    save, dgb = torch.empty(4, C, device="cuda"), torch.empty(2, C, device="cuda")
    w, b = par["weight"].cuda(), par["bias"].cuda()
    rm, rv = par["running_mean"].cuda(), par["running_var"].cuda()
    nws = int(L.LIB.mmt_batchnorm_ws_floats(M, C))
    ws = torch.empty(nws, device="cuda")
    L.check(L.LIB.mmt_batchnorm_relu(x.data_ptr(), y.data_ptr(), M, C, pitch, w.data_ptr(), b.data_ptr(), rm.data_ptr(),
                                     rv.data_ptr(), MOM, EPS, 1, 1, save.data_ptr(), ws.data_ptr(), nws, _st()), "bn")
    L.check(L.LIB.mmt_batchnorm_relu_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), M, C, pitch, w.data_ptr(),
                                         save.data_ptr(), 1, 1, dgb.data_ptr(), ws.data_ptr(), nws, _st()), "bn bwd")
    torch.cuda.synchronize()
    return y, save, rm, rv, dx, dgb


def _ulp32(v):
    """The spacing of fp32 at |v|."""
    v = abs(float(v))
    return 2.0 ** -149 if v < 2.0 ** -126 else 2.0 ** (math.frexp(v)[1] - 24)


def _stat_errors(save, rm, rv, ref):
    """Worst absolute error over the channels of (mean, invstd, running mean, running variance) against fp64."""
    got = {"mean": save[0], "invstd": save[1], "running_mean": rm, "running_var": rv}
    return {k: (v.double().cpu() - ref[k]).abs().max().item() for k, v in got.items()}


def _map_errors(out, ref, batches, C):
    rel = lambda a, r: ((a.double().cpu() - r).norm() / r.norm().clamp_min(1e-300)).item()  # noqa: E731
    e, r0 = {"y": 0.0, "dx": 0.0}, 0
    for r, b in enumerate(batches):
        sl = slice(r0, r0 + b)
        r0 += b
        e["y"] = max(e["y"], rel(out["y"][r][..., :C], ref["y"][sl]))
        e["dx"] = max(e["dx"], rel(out["dx"][r][..., :C], ref["dx"][sl]))
    dgb = torch.stack(out["dgb"]).double().sum(0)
    e["dgamma"], e["dbeta"] = rel(dgb[0], ref["dgamma"]), rel(dgb[1], ref["dbeta"])
    return e


MAP_BARS = {"y": 1e-2, "dx": 2e-2, "dgamma": 1e-3, "dbeta": 1e-3}  # test_hip_batchnorm_relu's (relative L2)


@pytest.mark.parametrize("batches,H,C", [((1, 1), 7, 8),        # fewer rows than row lanes
                                         ((1, 2), 20, 384),     # C8 = 48 does not divide 256; unequal counts
                                         ((1, 2, 1), 20, 1),    # pitch 8 with 7 padding channels; three ranks
                                         ((2, 2), 40, 96),
                                         ((4, 4), 80, 48)])     # 256 workgroups a rank: bn_lane_sums' 8-load loop
def test_virtual_ranks_match_full_batch(batches, H, C):
    """W virtual ranks in one process.  Across ranks: save, running statistics and n_total bitwise identical, n_total
    the total row count.  Per-channel statistics (save mean / invstd, running mean / variance; worst absolute error
    over the channels against fp64): no more than twice the error of the single-rank mmt_batchnorm_relu on the
    concatenated map, measured here against the same reference, plus four fp32 ulps of the largest reference value
    (the rows are partitioned into differently sized runs; nothing is less accurate).  Maps: test_hip_batchnorm_relu's
    bars.  Padding channels exactly 0.  Negative control: with rank 0's triple in every slot of the gathered buffer
    each of these checks fails by at least 10x its bar.  Bitwise repeatable."""
    xs, dys, par, xp, dyp, pitch = _case(batches, H, C)
    W = len(batches)
    ref = full_batch_reference(torch.cat(xs), torch.cat(dys), par["weight"], par["bias"], par["running_mean"],
                               par["running_var"], MOM, EPS)
    out = _virtual(xp, dyp, C, par)
    again = _virtual(xp, dyp, C, par)
    bad = _virtual(xp, dyp, C, par, no_exchange=True)
    loc = _local(torch.cat(xp), torch.cat(dyp), C, par)

    e_sync = _stat_errors(out["save"][0], out["rm"][0], out["rv"][0], ref)
    e_loc = _stat_errors(loc[1], loc[2], loc[3], ref)
    e_bad = _stat_errors(bad["save"][0], bad["rm"][0], bad["rv"][0], ref)
    bars = {k: 2.0 * e_loc[k] + 4.0 * _ulp32(ref[k].abs().max()) for k in e_sync}
    m_sync, m_bad = _map_errors(out, ref, batches, C), _map_errors(bad, ref, batches, C)
    for k in e_sync:
        print("B %s H %d C %d %s: sync %.3g local %.3g bar %.3g no-exchange %.3g"
              % (batches, H, C, k, e_sync[k], e_loc[k], bars[k], e_bad[k]))
    for k in m_sync:
        print("B %s H %d C %d %s: sync %.3g bar %.3g no-exchange %.3g" % (batches, H, C, k, m_sync[k], MAP_BARS[k], m_bad[k]))

    rows = sum(batches) * H * H
    for r in range(W):
        for k in ("save", "rm", "rv", "n"):
            assert torch.equal(out[k][r], out[k][0]), (k, r)
        assert out["n"][r].item() == float(rows)
        if pitch != C:
            assert not out["y"][r][..., C:].any() and not out["dx"][r][..., C:].any()
    for k in e_sync:
        assert e_sync[k] <= bars[k], (k, e_sync[k], bars[k])
    for k in m_sync:
        assert m_sync[k] <= MAP_BARS[k], (k, m_sync[k])
    # the bars discriminate: a missing exchange misses every one of them by 10x
    for k in e_sync:
        assert e_bad[k] >= 10.0 * bars[k], (k, e_bad[k], bars[k])
    for k in m_sync:
        assert m_bad[k] >= 10.0 * MAP_BARS[k], (k, m_bad[k])
    for k in out:
        for a, b in zip(out[k], again[k]):
            assert torch.equal(a, b), k


@pytest.mark.parametrize("B,H,C", [(2, 20, 384), (1, 7, 8), (2, 20, 1)])
def test_one_forced_rank_equals_local_path_bitwise(B, H, C):
    """W = 1: the fold passes rank 0's moments through, the exchange is fp64 and the sums run in the same order, so
    the four phases give mmt_batchnorm_relu + _bwd's y, save, running statistics, dx and dgb bit for bit."""
    _, _, par, xp, dyp, _ = _case((B,), H, C)
    out = _virtual(xp, dyp, C, par)
    y, save, rm, rv, dx, dgb = _local(xp[0], dyp[0], C, par)
    assert out["n"][0].item() == float(B * H * H)
    for name, a, b in (("y", out["y"][0], y), ("save", out["save"][0], save), ("running_mean", out["rm"][0], rm),
                       ("running_var", out["rv"][0], rv), ("dx", out["dx"][0], dx), ("dgb", out["dgb"][0], dgb)):
        assert torch.equal(a, b), (name, (a.float() - b.float()).abs().max().item())
