"""The score decoder's training kernels (csrc/spm_train.hip): mmt_spm_attention_train_fwd / _bwd / mmt_spm_dq_sum
and mmt_bce_logits / _bwd against fp64, with PyTorch's own fp32 device result as the yardstick, plus exact
probes that account for every key."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(1, 16, 12), (2, 128, 12), (1, 288, 16), (3, 300, 2), (2, 1, 2), (2, 257, 2)]
GUARD = 3  # NaN guard rows on both sides of every output


def _L():
    from mmt_amd import _lib
    return _lib


def _st():
    return torch.cuda.current_stream().cuda_stream


def _guarded(rows, cols):
    """(whole NaN-filled buffer, the payload rows in its middle)."""
    buf = torch.full((rows + 2 * GUARD, cols), float("nan"), device="cuda")
    return buf, buf[GUARD:GUARD + rows]


def _guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all())


def hip_fwd(q, kv, H, scale):
    """q (B, C) or (1, C), kv (B, Lk, 2C) on the device -> out, prob (payload views) and their guarded buffers."""
    L = _L()
    B, Lk, C2 = kv.shape
    C = C2 // 2
    qs = C if q.shape[0] == B else 0
    ob, out = _guarded(B, C)
    pb, prob = _guarded(B * H, Lk)
    L.check(L.LIB.mmt_spm_attention_train_fwd(q.data_ptr(), qs, kv.data_ptr(), out.data_ptr(), prob.data_ptr(), B, Lk,
                                              C, H, scale, _st()), "mmt_spm_attention_train_fwd")
    torch.cuda.synchronize()
    return out, prob.view(B, H, Lk), (ob, pb)


def hip_bwd(q, kv, prob, dout, H, scale):
    L = _L()
    B, Lk, C2 = kv.shape
    C = C2 // 2
    qs = C if q.shape[0] == B else 0
    qb, dq = _guarded(B, C)
    kb, dkv = _guarded(B * Lk, 2 * C)
    L.check(L.LIB.mmt_spm_attention_bwd(q.data_ptr(), qs, kv.data_ptr(), prob.data_ptr(), dout.data_ptr(),
                                        dq.data_ptr(), dkv.data_ptr(), B, Lk, C, H, scale, _st()),
            "mmt_spm_attention_bwd")
    torch.cuda.synchronize()
    return dq, dkv.view(B, Lk, 2 * C), (qb, kb)


def attention(q, kv, H, scale):
    """softmax(q k^T scale) v per head in q's dtype; q (B, C) (an expanded shared row included)."""
    B, Lk, C2 = kv.shape
    C = C2 // 2
    k = kv[..., :C].reshape(B, Lk, H, 64).transpose(1, 2)
    v = kv[..., C:].reshape(B, Lk, H, 64).transpose(1, 2)
    a = torch.softmax(q.reshape(B, H, 1, 64) @ k.transpose(-1, -2) * scale, -1)
    return (a @ v).reshape(B, C), a.reshape(B, H, Lk)


def grads(q, kv, dout, H, scale, shared):
    """autograd of attention(): (dq, dkv); shared: q (1, C) expanded over the batch, dq (1, C)."""
    q, kv = q.detach().clone().requires_grad_(True), kv.detach().clone().requires_grad_(True)
    out, _ = attention(q.expand(kv.shape[0], -1) if shared else q, kv, H, scale)
    out.backward(dout)
    return q.grad, kv.grad


def _data(B, Lk, H, shared, seed=0):
    C = 64 * H
    g = torch.Generator().manual_seed(1000 * seed + 7 * Lk + H + (1 if shared else 0))
    q = torch.randn(1 if shared else B, C, generator=g)
    kv = torch.randn(B, Lk, 2 * C, generator=g)
    dout = torch.randn(B, C, generator=g)
    return q, kv, dout, C


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("B,Lk,H", SHAPES)
def test_train_fwd_matches_inference_kernel_and_fp64(B, Lk, H, shared):
    """out has mmt_spm_attention's bits; prob within 1e-5 of the fp64 softmax, every row summing to 1 within
    Lk 2^-23; nothing written outside out / prob."""
    L = _L()
    q, kv, _, C = _data(B, Lk, H, shared)
    scale = C ** -0.5
    qd, kvd = q.cuda(), kv.cuda()
    out, prob, bufs = hip_fwd(qd, kvd, H, scale)
    ref_out = torch.empty(B, C, device="cuda")
    L.check(L.LIB.mmt_spm_attention(qd.data_ptr(), 0 if shared else C, kvd.data_ptr(), ref_out.data_ptr(), B, Lk, C, H,
                                    scale, _st()), "mmt_spm_attention")
    torch.cuda.synchronize()
    assert torch.equal(out, ref_out)
    _, p64 = attention(q.double().expand(B, -1), kv.double(), H, scale)
    perr = (prob.cpu().double() - p64).abs().max().item()
    serr = (prob.cpu().double().sum(-1) - 1).abs().max().item()
    print("prob err %.3g, row-sum err %.3g (bound %.3g)" % (perr, serr, Lk * 2.0 ** -23))
    assert perr <= 1e-5
    assert serr <= Lk * 2.0 ** -23
    assert all(_guards_intact(b) for b in bufs)
    assert torch.isfinite(out).all() and torch.isfinite(prob).all()


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("Lk,hi", [(16, 2), (128, 1)])
def test_exact_probe_accounts_for_every_key(Lk, hi, shared):
    """scale 0.125, q_h = e_0, k_j[0] = 1: every score is 0.125, every exponential exp(0) = 1 and prob = 1 / Lk
    exactly; the other k channels, v and dout are small integers, so every quantity of the forward and the
    backward is a sum of dyadic rationals that fp32 holds exactly in any order (dq at Lk = 128: 21 bits).  out,
    prob, dq, dk and dv equal the fp64 evaluation of the formulas bit for bit (-0.0 == 0.0): a skipped, doubled or
    misplaced key changes them.  The outputs lie in NaN-filled buffers: the guard rows stay NaN, the payload is
    finite everywhere."""
    B, H, scale = 2, 2, 0.125
    C = 64 * H
    g = torch.Generator().manual_seed(Lk + hi)
    ri = lambda *s: torch.randint(-hi, hi + 1, s, generator=g).float()  # noqa: E731
    q = torch.zeros(1 if shared else B, H, 64)
    q[:, :, 0] = 1.0
    q = q.view(-1, C)
    k = ri(B, Lk, H, 64)
    k[..., 0] = 1.0
    kv = torch.cat([k.view(B, Lk, C), ri(B, Lk, C)], -1).contiguous()
    dout = ri(B, C)
    qd, kvd, dd = q.cuda(), kv.cuda(), dout.cuda()
    out, prob, fb = hip_fwd(qd, kvd, H, scale)
    dq, dkv, bb = hip_bwd(qd, kvd, prob, dd, H, scale)
    # the formulas in fp64
    k64, v64 = kv[..., :C].double().view(B, Lk, H, 64), kv[..., C:].double().view(B, Lk, H, 64)
    do64, q64 = dout.double().view(B, H, 64), q.double().expand(B, C).reshape(B, H, 64)
    p64 = torch.full((B, H, Lk), 1.0 / Lk, dtype=torch.float64)
    o64 = torch.einsum("bhk,bkhd->bhd", p64, v64)
    dp = torch.einsum("bhd,bkhd->bhk", do64, v64)
    ds = p64 * (dp - (p64 * dp).sum(-1, keepdim=True))
    dv = torch.einsum("bhk,bhd->bkhd", p64, do64).reshape(B, Lk, C)
    dk = scale * torch.einsum("bhk,bhd->bkhd", ds, q64).reshape(B, Lk, C)
    dq64 = scale * torch.einsum("bhk,bkhd->bhd", ds, k64).reshape(B, C)
    assert ds.abs().max() > 0
    for name, got, exp in (("out", out, o64.reshape(B, C)), ("prob", prob, p64), ("dq", dq, dq64),
                           ("dk", dkv[..., :C], dk), ("dv", dkv[..., C:], dv)):
        got = got.cpu().double()
        assert torch.isfinite(got).all(), name
        assert bool((got == exp).all()), (name, (got - exp).abs().max().item())
    assert all(_guards_intact(b) for b in fb + bb)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("B,Lk,H", SHAPES)
def test_bwd_random_data_within_4x_of_torch_fp32(B, Lk, H, shared):
    """N(0, 1) data: dq, dk, dv against fp64 autograd of softmax(q k^T scale) v on the CPU.  The yardstick is
    torch's own fp32 autograd of the same expression on the device (the path the kernel replaces): per tensor,
    the HIP max-abs error may be at most 4x the yardstick's (a different but equally valid fp32 summation
    order).  With a shared query the kernel's dq rows summed in order (mmt_spm_dq_sum) are held against the
    autograd of the expanded query.  Two launches give the same bits."""
    L = _L()
    q, kv, dout, C = _data(B, Lk, H, shared, seed=1)
    scale = C ** -0.5
    qd, kvd, dd = q.cuda(), kv.cuda(), dout.cuda()
    out, prob, _ = hip_fwd(qd, kvd, H, scale)
    dq, dkv, bufs = hip_bwd(qd, kvd, prob, dd, H, scale)
    out2, prob2, _ = hip_fwd(qd, kvd, H, scale)
    dq2, dkv2, _ = hip_bwd(qd, kvd, prob2, dd, H, scale)
    assert torch.equal(out, out2) and torch.equal(prob, prob2) and torch.equal(dq, dq2) and torch.equal(dkv, dkv2)
    assert all(_guards_intact(b) for b in bufs)
    assert torch.isfinite(dq).all() and torch.isfinite(dkv).all()
    if shared:
        rows, dq = dq, torch.full((1, C), float("nan"), device="cuda")
        L.check(L.LIB.mmt_spm_dq_sum(rows.data_ptr(), dq.data_ptr(), B, C, _st()), "mmt_spm_dq_sum")
        acc = torch.zeros(C, device="cuda")
        for b in range(B):
            acc = acc + rows[b]
        assert torch.equal(dq[0], acc)  # the rows in order
    q64, kv64 = grads(q.double(), kv.double(), dout.double(), H, scale, shared)
    q32, kv32 = grads(qd, kvd, dd, H, scale, shared)
    for name, got, yard, ref in (("dq", dq, q32, q64), ("dk", dkv[..., :C], kv32[..., :C], kv64[..., :C]),
                                 ("dv", dkv[..., C:], kv32[..., C:], kv64[..., C:])):
        e_hip = (got.cpu().double() - ref).abs().max().item()
        e_torch = (yard.cpu().double() - ref).abs().max().item()
        print("spm_bwd (B %d, Lk %d, H %d, shared %d) %s: hip %.3g torch-fp32 %.3g" % (B, Lk, H, shared, name, e_hip,
                                                                                        e_torch))
        assert e_hip <= 4 * e_torch, (name, e_hip, e_torch)


BASE_LOGITS = [0.0, 1e-3, -1e-3, 8.0, -8.0, 50.0, -50.0, 200.0, -200.0]
BASE_LABELS = [0.0, 1.0, 0.3]


def _bce(x, y, weight, dloss):
    L = _L()
    B = x.numel()
    loss = torch.full((3,), float("nan"), device="cuda")
    dx = torch.full((B + 2,), float("nan"), device="cuda")
    dl = torch.tensor([dloss], device="cuda")
    L.check(L.LIB.mmt_bce_logits(x.data_ptr(), y.data_ptr(), weight, loss[1:].data_ptr(), B, _st()), "mmt_bce_logits")
    L.check(L.LIB.mmt_bce_logits_bwd(x.data_ptr(), y.data_ptr(), dl.data_ptr(), weight, dx[1:].data_ptr(), B, _st()),
            "mmt_bce_logits_bwd")
    torch.cuda.synchronize()
    assert torch.isnan(loss[0]) and torch.isnan(loss[2]) and torch.isnan(dx[0]) and torch.isnan(dx[-1])
    return loss[1].clone(), dx[1:-1].clone()


@pytest.mark.parametrize("B", [1, 3, 16, 65])
def test_bce_logits(B):
    """Loss and dlogits against F.binary_cross_entropy_with_logits in fp64 (logits 0, +-1e-3, +-8, +-50, +-200
    against labels 0, 1, 0.3), each at most 4x torch's fp32 device result's error; finite at +-200; weight and
    dloss scale exactly by powers of two."""
    x = torch.tensor([BASE_LOGITS[(i + B) % 9] for i in range(B)])
    y = torch.tensor([BASE_LABELS[(i // 9 + i + B) % 3] for i in range(B)])
    xd, yd = x.cuda(), y.cuda()
    loss, dx = _bce(xd, yd, 1.0, 1.0)
    assert torch.isfinite(loss) and torch.isfinite(dx).all()
    x64 = x.double().requires_grad_(True)
    l64 = F.binary_cross_entropy_with_logits(x64, y.double())
    l64.backward()
    x32 = xd.clone().requires_grad_(True)
    l32 = F.binary_cross_entropy_with_logits(x32, yd)
    l32.backward()
    for name, got, yard, ref in (("loss", loss, l32.detach(), l64.detach()), ("dlogits", dx, x32.grad, x64.grad)):
        e_hip = (got.cpu().double() - ref).abs().max().item()
        e_torch = (yard.cpu().double() - ref).abs().max().item()
        print("bce B %d %s: hip %.3g torch-fp32 %.3g" % (B, name, e_hip, e_torch))
        assert e_hip <= 4 * e_torch, (name, e_hip, e_torch)
    loss4, dx2 = _bce(xd, yd, 4.0, 0.5)
    assert torch.equal(loss4, 4 * loss) and torch.equal(dx2, 2 * dx)
    lossh, dxh = _bce(xd, yd, 0.5, 0.25)
    assert torch.equal(lossh, 0.5 * loss) and torch.equal(dxh, 0.125 * dx)
    loss_b, dx_b = _bce(xd, yd, 1.0, 1.0)
    assert torch.equal(loss_b, loss) and torch.equal(dx_b, dx)


def test_hip_ops_wrappers_at_vitl_geometry():
    """HipOps.spm_attention (_HipSpmAttention) at the ViT-L decoder's geometry (B, Lk, H) = (2, 288, 16), per-row
    and shared query, and HipOps.bce_logits behind it: gradients against fp64 under the random-data bound."""
    from mmt_amd.train import HipOps
    B, Lk, H = 2, 288, 16
    for shared in (False, True):
        q, kv, dout, C = _data(B, Lk, H, shared, seed=2)
        scale = C ** -0.5
        qd, kvd = q.cuda().requires_grad_(True), kv.cuda().requires_grad_(True)
        out = HipOps.spm_attention(qd, kvd, H, scale)
        assert out.shape == (B, C)
        out.backward(dout.cuda())
        assert qd.grad.shape == q.shape and kvd.grad.shape == kv.shape
        q64, kv64 = grads(q.double(), kv.double(), dout.double(), H, scale, shared)
        q32, kv32 = grads(q.cuda(), kv.cuda(), dout.cuda(), H, scale, shared)
        for name, got, yard, ref in (("dq", qd.grad, q32, q64), ("dkv", kvd.grad, kv32, kv64)):
            e_hip = (got.cpu().double() - ref).abs().max().item()
            e_torch = (yard.cpu().double() - ref).abs().max().item()
            print("HipOps.spm_attention shared %d %s: hip %.3g torch-fp32 %.3g" % (shared, name, e_hip, e_torch))
            assert e_hip <= 4 * e_torch, (name, e_hip, e_torch)
    x = torch.tensor([0.3, -1.2, 2.0], device="cuda", requires_grad=True)
    y = torch.tensor([1.0, 0.0, 1.0], device="cuda")
    loss = HipOps.bce_logits(x, y, 2.0)
    assert loss.dim() == 0
    loss.backward()
    ref = x.detach().double().cpu().requires_grad_(True)
    lref = 2.0 * F.binary_cross_entropy_with_logits(ref, y.double().cpu())
    lref.backward()
    assert abs(loss.item() - lref.item()) <= 1e-6 and (x.grad.cpu().double() - ref.grad).abs().max().item() <= 1e-6
