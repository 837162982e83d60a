"""The corner head's training chain against exact probes (tests/head_probes.py): _HipConv3x3 (forward, dX, dW,
db) with its block-sum and im2col kernels, _HipAddUp's backward, mmt_batchnorm_relu / _bwd, mmt_corner_score_train /
_bwd and mmt_corner_boxes / _bwd.

Every comparison is bitwise (torch.equal, or gemm_probes.same on a NaN-guarded storage image) except the three
with a derived bar: the batch-norm moments where M is odd or x a general integer pattern (head_probes.BN_MEAN_ULPS
/ BN_INV_ULPS and what follows from them), the batch norm's bf16 dx (one bf16 rounding of the fp64 reference,
head_probes.bf16_bar) and the soft-argmax of a constant map (head_probes.boxes_const_bar).  Outputs handed to the
C ABI are GUARD rows larger than the problem and NaN before the launch, and are compared whole: an element that
should have been written and was not, and a pitch or surplus element that was, both fail.  Outputs the autograd
wrappers allocate themselves are compared whole at their own size (the allocator's free blocks are NaN-filled
first).  test_head_probes_host.py shows that the references are exact and that one dropped, doubled or displaced
term moves them."""
import pytest
import torch

import gemm_probes as P
import head_probes as H

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32


def _lib():
    from mmt_amd import _lib
    return _lib


def _st():
    return torch.cuda.current_stream().cuda_stream


def _poison_free_blocks():
    """NaN bytes into the caching allocator's free blocks: the wrappers' torch.empty outputs start from them."""
    t = torch.full((1 << 22,), H.NAN, device="cuda")
    del t


def _vec(t, dtype=F32):
    """A 1-D operand with GUARD NaN elements behind it."""
    return torch.cat([t.reshape(-1).to(dtype), torch.full((H.GUARD,), H.NAN, dtype=dtype)]).cuda()


def _check(errors, what, got, want):
    """got (device) against a storage image `want` (host), every element, guards included."""
    got = got.cpu()
    if got.shape != want.shape or got.dtype != want.dtype:
        errors.append("%s: %s %s, expected %s %s" % (what, got.dtype, tuple(got.shape), want.dtype, tuple(want.shape)))
    elif not P.same(got, want):
        errors.append("%s: %s" % (what, P.describe(got, want)))


def _check_equal(errors, what, got, want):
    got = got.detach().cpu()
    if got.shape != want.shape or got.dtype != want.dtype:
        errors.append("%s: %s %s, expected %s %s" % (what, got.dtype, tuple(got.shape), want.dtype, tuple(want.shape)))
    elif not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        i = tuple(bad.nonzero()[0].tolist())
        errors.append("%s: %d of %d elements differ; first at %s: got %r, expected %r" %
                      (what, int(bad.sum()), bad.numel(), i, got[i].item(), want[i].item()))


def _check_bar(errors, what, got, ref, bar):
    """|got - ref| <= bar elementwise (float64); returns the worst |got - ref| / bar."""
    err = (got.detach().cpu().double() - ref).abs()
    ratio = err / bar
    ratio = torch.where(torch.isnan(ratio) & (err == 0), torch.zeros_like(ratio), ratio)  # 0 / 0: exact where the bar is 0
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if not worst <= 1.0:
        i = tuple((~(ratio <= 1.0)).nonzero()[0].tolist())
        errors.append("%s: %.3g x the bar at %s (got %r, reference %r, bar %.3g)" %
                      (what, worst, i, got.detach().cpu().double()[i].item(), ref[i].item(), bar[i].item() if bar.dim() else float(bar)))
    return worst


def _report(errors):
    assert not errors, "%d checks failed:\n%s" % (len(errors), "\n".join(errors[:8]))


# ------------------------------------------------------------------------------------------------ 1. conv3x3
@pytest.mark.parametrize("c", H.CONV_CASES, ids=lambda c: "B%d-H%d-up%d-%dto%d%s" % (c.B, c.Hi, c.up, c.Cin, c.Cout, "-pad" if c.keep_pad else ""))
def test_conv3x3_forward_and_gradients_exact(c):
    """HipOps.conv3x3 on integer one-hot maps: y, dX (the flipped-tap conv on the wb layout and the up x up block
    sums), dW (channel-major im2col) and db equal float64 F.conv2d autograd of the nearest-upsampled input bit for
    bit; prepared weights give the same bits; with keep_pad, finite non-zero values in dY's padding channels
    change nothing and y's padding channels are 0."""
    from mmt_amd.train import HipOps
    pr = H.conv_problem(c)
    errors = []
    want_y = (pr["y_pad"] if c.keep_pad else pr["y"]).to(BF16)
    fills = (False, True) if (c.keep_pad and c.Cp > c.Cout) else (False,)
    for prep in (False, True):
        for fill in fills:
            tag = "%s%s" % ("prep " if prep else "", "filled " if fill else "")
            x = pr["x"].to(BF16).cuda().requires_grad_(True)
            w = pr["w"].float().cuda().requires_grad_(True)
            b = pr["b"].float().cuda().requires_grad_(True)
            layouts = HipOps.conv_wprep([(w, b)])[0] if prep else None
            _poison_free_blocks()
            y = HipOps.conv3x3(x, w, b, c.up, c.keep_pad, layouts)
            if c.keep_pad:
                dy = pr["dy_pad"].clone()
                if fill:
                    dy[..., c.Cout:] = pr["pad_fill"]
            else:
                dy = pr["dy"]
            _poison_free_blocks()
            y.backward(dy.to(BF16).cuda())
            torch.cuda.synchronize()
            _check_equal(errors, tag + "y", y, want_y)
            _check_equal(errors, tag + "dx", x.grad, pr["dx"].to(BF16))
            _check_equal(errors, tag + "dw", w.grad, pr["dw"].float())
            _check_equal(errors, tag + "db", b.grad, pr["db"].float())
    _report(errors)


def test_upsample_sum_kernel_exact():
    """mmt_upsample_sum_bf16 on rectangular maps, chunk counts below, at and raggedly above 256."""
    L = _lib()
    errors = []
    for case in H.UPSUM_CASES:
        B, Hi, Wi, C, up = case
        src, ref = H.upsum_problem(case)
        inp = H.image(src.numel() // C, C, src, BF16).cuda()
        out = H.poison(B * Hi * Wi, C, BF16).cuda()
        L.check(L.LIB.mmt_upsample_sum_bf16(inp.data_ptr(), out.data_ptr(), B, Hi, Wi, C, up, _st()), "upsample_sum %s" % (case,))
        _check(errors, "upsample_sum %s" % (case,), out, H.image(B * Hi * Wi, C, ref, BF16))
    _report(errors)


def test_im2col_kernels_exact():
    """mmt_im2col3x3_cm_bf16 (columns c * 9 + tap) and mmt_im2col3x3_up_bf16 (tap * C + c) of the nearest-upsampled
    map against F.unfold, rectangular maps, chunk counts below, at and raggedly above 256."""
    L = _lib()
    errors = []
    for case in H.IM2COL_CASES:
        B, Hh, W, C, up = case
        src, cm, tm = H.im2col_problem(case)
        inp = H.image(src.numel() // C, C, src, BF16).cuda()
        for name, fn, ref in (("cm", L.LIB.mmt_im2col3x3_cm_bf16, cm), ("up", L.LIB.mmt_im2col3x3_up_bf16, tm)):
            out = H.poison(B * Hh * W, 9 * C, BF16).cuda()
            L.check(fn(inp.data_ptr(), out.data_ptr(), B, Hh, W, C, up, _st()), "im2col %s %s" % (name, case))
            _check(errors, "im2col %s %s" % (name, case), out, H.image(B * Hh * W, 9 * C, ref, BF16))
    _report(errors)


# ------------------------------------------------------------------------------------------------ 2. add_up
def test_add_up_backward_exact():
    """HipOps.add_up with integer maps: the forward, da = the exact up x up block sums of dout, db = dout itself."""
    from mmt_amd.train import HipOps
    errors = []
    for case in H.ADDUP_CASES:
        a, b, dout, out, da = H.addup_problem(case)
        ad, bd = a.to(BF16).cuda().requires_grad_(True), b.to(BF16).cuda().requires_grad_(True)
        _poison_free_blocks()
        o = HipOps.add_up(ad, bd, case[4])
        o.backward(dout.to(BF16).cuda())
        torch.cuda.synchronize()
        _check_equal(errors, "add_up %s out" % (case,), o, out.to(BF16))
        _check_equal(errors, "add_up %s da" % (case,), ad.grad, da.to(BF16))
        _check_equal(errors, "add_up %s db" % (case,), bd.grad, dout.to(BF16))
    _report(errors)


# ------------------------------------------------------------------------------------------------ 3. batch norm
def _run_bn(case, errors, worst):
    L = _lib()
    pr = H.bn_problem(case)
    M, C, pitch = case.M, case.C, case.pitch
    tag = "%s " % (case,)
    x, dy = H.image(M, pitch, pr["x"], BF16).cuda(), H.image(M, pitch, pr["dy"], BF16).cuda()
    y, dx = H.poison(M, pitch, BF16).cuda(), H.poison(M, pitch, BF16).cuda()
    gamma, beta = _vec(pr["gamma"]), _vec(pr["beta"])
    rm, rv = _vec(pr["rm0"]), _vec(pr["rv0"])
    save, dgb = H.poison(4, C, F32).cuda(), H.poison(2, C, F32).cuda()
    nws = int(L.LIB.mmt_batchnorm_ws_floats(M, C))
    ws = torch.full((nws + H.GUARD,), H.NAN, device="cuda")
    L.check(L.LIB.mmt_batchnorm_relu(x.data_ptr(), y.data_ptr(), M, C, pitch, gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(),
                                     rv.data_ptr(), H.BN_MOM, H.BN_EPS, case.training, case.relu, save.data_ptr(), ws.data_ptr(),
                                     nws, _st()), tag + "forward")
    L.check(L.LIB.mmt_batchnorm_relu_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), M, C, pitch, gamma.data_ptr(), save.data_ptr(),
                                         case.training, case.relu, dgb.data_ptr(), ws.data_ptr(), nws, _st()), tag + "backward")
    torch.cuda.synchronize()
    guard = torch.full((H.GUARD,), H.NAN)
    nanrows = lambda t: bool(torch.isnan(t.cpu()[-H.GUARD:]).all())  # noqa: E731
    want_save = torch.stack([pr["mean"], pr["inv"], pr["sc"], pr["sh"]])
    _check(errors, tag + "dbeta", dgb[1:], H.image(1, C, pr["dbeta"], F32))  # an exact integer sum in every case
    if pr["exact"]:
        _check(errors, tag + "save", save, H.image(4, C, want_save, F32))
        _check(errors, tag + "y", y, H.image(M, pitch, pr["y"], BF16))
        _check(errors, tag + "running_mean", rm.cpu(), torch.cat([pr["rm1"], guard]))
        _check(errors, tag + "running_var", rv.cpu(), torch.cat([pr["rv1"], guard]))
        _check_equal(errors, tag + "dgamma", dgb[0], pr["dgamma"].float())
    else:
        if not (nanrows(save) and nanrows(y) and nanrows(rm) and nanrows(rv)):
            errors.append(tag + "a guard element of save / y / the running statistics was written")
        s = save.cpu()
        worst["mean"] = max(worst["mean"], _check_bar(errors, tag + "save[0]", s[0], pr["mean"], H.bn_mean_bar(pr["mean"])) * H.BN_MEAN_ULPS)
        worst["inv"] = max(worst["inv"], _check_bar(errors, tag + "save[1]", s[1], pr["inv"], H.bn_inv_bar(pr["inv"])) * H.BN_INV_ULPS)
        # scale = gamma * invstd: invstd's bar and the product; shift = beta - mean * scale: both bars, a product, a subtract
        _check_bar(errors, tag + "save[2]", s[2], pr["sc"], (2 * H.BN_INV_ULPS + 1) * H.U32 * pr["sc"].abs())
        _check_bar(errors, tag + "save[3]", s[3], pr["sh"], 12 * H.U32 * ((pr["mean"] * pr["sc"]).abs() + pr["beta"].abs()) + 2.0 ** -40)
        yv = y.cpu()[:M]
        _check_bar(errors, tag + "y", yv, pr["y"], H.bf16_bar(pr["y"], pr["y_delta"]))
        rmb, rvb = H.bn_running_bars(pr)
        _check_bar(errors, tag + "running_mean", rm[:C], pr["rm1"].double() if not case.training else
                   0.75 * pr["rm0"].double() + 0.25 * pr["mean"], rmb + 2.0 ** -40)
        vu = pr["var"] * M / max(M - 1, 1)
        _check_bar(errors, tag + "running_var", rv[:C], 0.75 * pr["rv0"].double() + 0.25 * vu, rvb)
        _check_bar(errors, tag + "dgamma", dgb[0], pr["dgamma"], pr["dgamma_bar"] + 2.0 ** -40)
        if not bool((yv[:, C:] == 0).all()):
            errors.append(tag + "y is not 0 in the padding channels")
    dxv = dx.cpu()
    if case.training:
        worst["dx"] = max(worst["dx"], _check_bar(errors, tag + "dx", dxv[:M], pr["dx"], H.bf16_bar(pr["dx"], pr["dx_delta"])))
        if not (nanrows(dx) and bool((dxv[:M, C:] == 0).all())):
            errors.append(tag + "dx: a guard row written, or padding channels not 0")
    else:  # eval: dx = gamma * invstd * g, exact
        _check(errors, tag + "dx", dx, H.image(M, pitch, pr["dx"], BF16))
    if not nanrows(dgb):
        errors.append(tag + "a guard element of dgb was written")


@pytest.mark.parametrize("C,pitch", H.BN_CP)
def test_batchnorm_row_census(C, pitch):
    """mmt_batchnorm_relu / _bwd over the M and (C, pitch) edges.  Balanced censuses (x = m_c +- 1 in equal counts,
    eps 3, |m_c| up to 254) and the eval runs: save, y, the running statistics, dgamma, dbeta and the eval dx bit
    for bit.  Odd M and general integer x: save[0] within 1 fp32 ulp of the float64 mean (exact pivoted sums, a
    double finalize, one cast), save[1] within 3 ulp of the float64 1 / sqrt(var + eps) (cast, add, sqrtf, divide:
    5 half-ulps if the device functions round to 1 ulp), y within one bf16 rounding, dbeta still exact.  The training dx
    (it divides by M) within one bf16 rounding of the float64 reference everywhere (head_probes.bf16_bar).
    Padding channels of y and dx are 0 although x and dY are non-zero there; training 0 and relu 0 included."""
    errors = []
    worst = {"mean": 0.0, "inv": 0.0, "dx": 0.0}
    cases = H.bn_cases(C, pitch)
    for case in cases:
        _run_bn(case, errors, worst)
    print("batch norm C %d pitch %d, %d cases: worst save[0] %.3f ulp (bar %d), save[1] %.3f ulp (bar %d), dx %.3f of its bar"
          % (C, pitch, len(cases), worst["mean"], H.BN_MEAN_ULPS, worst["inv"], H.BN_INV_ULPS, worst["dx"]))
    _report(errors)


@pytest.mark.parametrize("C,pitch", [(8, 8), (50, 56)])
def test_bn_relu_wrapper_matches_the_kernels(C, pitch):
    """HipOps.bn_relu on a training nn.BatchNorm2d (C = 50: the wrapper pads the rows to 56 and slices them back):
    the balanced census' exact y, running statistics, dgamma and dbeta; dx within one bf16 rounding."""
    from mmt_amd.train import HipOps
    case = H.BNCase(32, C, pitch)
    pr = H.bn_problem(case)
    bn = torch.nn.BatchNorm2d(C, eps=H.BN_EPS, momentum=H.BN_MOM).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(pr["gamma"].float())
        bn.bias.copy_(pr["beta"].float())
        bn.running_mean.copy_(pr["rm0"].float())
        bn.running_var.copy_(pr["rv0"].float())
    x = pr["x"][:, :C].to(BF16).reshape(2, 4, 4, C).cuda().requires_grad_(True)
    _poison_free_blocks()
    y = HipOps.bn_relu(x, bn)
    y.backward(pr["dy"][:, :C].to(BF16).reshape(2, 4, 4, C).cuda())
    torch.cuda.synchronize()
    errors = []
    _check_equal(errors, "y", y.reshape(32, C), pr["y"][:, :C].to(BF16))
    _check_equal(errors, "running_mean", bn.running_mean, pr["rm1"])
    _check_equal(errors, "running_var", bn.running_var, pr["rv1"])
    _check_equal(errors, "dgamma", bn.weight.grad, pr["dgamma"].float())
    _check_equal(errors, "dbeta", bn.bias.grad, pr["dbeta"].float())
    _check_bar(errors, "dx", x.grad.reshape(32, C), pr["dx"][:, :C], H.bf16_bar(pr["dx"], pr["dx_delta"])[:, :C])
    assert int(bn.num_batches_tracked) == 1
    _report(errors)


# ------------------------------------------------------------------------------------------------ 4. corner score
def _score_buffers(c, pr):
    B, fh, c4 = c.B, c.fh, c.c4
    n, n3, n4 = B * fh * fh, B * (fh // 4) ** 2, B * (fh // 2) ** 2
    return dict(n=n, n3=n3, n4=n4, x4=H.image(n, c4, pr["x4"], BF16).cuda(), w5=_vec(pr["w5"]), b5=_vec(pr["b5"]),
                a3=H.image(n3, c.p3, H.padded_rows(pr["a3"], c.p3, H.NAN), BF16).cuda(),   # padding channels NaN: never read
                a4=H.image(n4, c.p4, H.padded_rows(pr["a4"], c.p4, H.NAN), BF16).cuda(),
                dsm=H.image(n, 1, pr["dsm"], F32).cuda())


@pytest.mark.parametrize("c", H.SCORE_CASES, ids=lambda c: "B%d-fh%d-c%d-p%d%d" % (c.B, c.fh, c.c4, c.p3, c.p4))
def test_corner_score_train_exact(c):
    """mmt_corner_score_train / _bwd on integer maps: sm, dx4, da3 (4x4 sums), da4 (2x2 sums), dw5 and db5 (band
    partials, 16 interleaved band groups) bit for bit; padding channels of pitch-8 da3 / da4 rows 0, pitch 1 writes
    its element only."""
    L = _lib()
    pr = H.score_problem(c)
    B, fh, c4 = c.B, c.fh, c.c4
    t = _score_buffers(c, pr)
    errors = []
    sm = H.poison(t["n"], 1, F32).cuda()
    L.check(L.LIB.mmt_corner_score_train(t["x4"].data_ptr(), t["w5"].data_ptr(), t["b5"].data_ptr(), t["a3"].data_ptr(), c.p3,
                                         t["a4"].data_ptr(), c.p4, sm.data_ptr(), B, fh, c4, _st()), "forward")
    dx4 = H.poison(t["n"], c4, BF16).cuda()
    da3, da4 = H.poison(t["n3"], c.p3, BF16).cuda(), H.poison(t["n4"], c.p4, BF16).cuda()
    dw, db = H.poison(c4, 1, F32).cuda(), H.poison(1, 1, F32).cuda()
    nws = int(L.LIB.mmt_corner_score_train_ws_floats(B, fh, c4))
    ws = torch.full((nws + H.GUARD,), H.NAN, device="cuda")
    L.check(L.LIB.mmt_corner_score_train_bwd(t["dsm"].data_ptr(), t["x4"].data_ptr(), t["w5"].data_ptr(), dx4.data_ptr(),
                                             da3.data_ptr(), c.p3, da4.data_ptr(), c.p4, dw.data_ptr(), db.data_ptr(),
                                             ws.data_ptr(), B, fh, c4, _st()), "backward")
    torch.cuda.synchronize()
    _check(errors, "sm", sm, H.image(t["n"], 1, pr["sm"], F32))
    _check(errors, "dx4", dx4, H.image(t["n"], c4, pr["dx4"], BF16))
    _check(errors, "da3", da3, H.image(t["n3"], c.p3, H.padded_rows(pr["da3"], c.p3, 0.0), BF16))
    _check(errors, "da4", da4, H.image(t["n4"], c.p4, H.padded_rows(pr["da4"], c.p4, 0.0), BF16))
    _check(errors, "dw5", dw, H.image(c4, 1, pr["dw5"], F32))
    _check(errors, "db5", db, H.image(1, 1, pr["db5"], F32))
    if not bool(torch.isnan(ws[nws:]).all()):
        errors.append("the workspace was written past mmt_corner_score_train_ws_floats")
    _report(errors)


@pytest.mark.parametrize("c", [H.SCORE_CASES[1], H.SCORE_CASES[5]], ids=["padded-rows", "one-channel"])
def test_corner_score_wrapper_exact(c):
    """HipOps.corner_score (_HipCornerScore: the strides and pitches it hands the kernels) on the same integer maps:
    the score map and every gradient bit for bit, the padded rows' padding channels 0."""
    from mmt_amd.train import HipOps
    pr = H.score_problem(c)
    B, fh, c4 = c.B, c.fh, c.c4
    conv5 = torch.nn.Conv2d(c4, 1, 1).cuda()
    with torch.no_grad():
        conv5.weight.copy_(pr["w5"].float().view(1, c4, 1, 1))
        conv5.bias.copy_(pr["b5"].float())
    x4 = pr["x4"].to(BF16).cuda().requires_grad_(True)
    rows = lambda t, p: H.padded_rows(t, p, 0.0).to(BF16).view(t.shape + (p,)).cuda().requires_grad_(True)  # noqa: E731
    a3, a4 = rows(pr["a3"], c.p3), rows(pr["a4"], c.p4)
    _poison_free_blocks()
    sm = HipOps.corner_score(x4, conv5, a3, a4)
    sm.backward(pr["dsm"].float().view(B, fh * fh).cuda())
    torch.cuda.synchronize()
    errors = []
    _check_equal(errors, "sm", sm, pr["sm"].float().view(B, fh * fh))
    _check_equal(errors, "dx4", x4.grad, pr["dx4"].to(BF16))
    _check_equal(errors, "da3", a3.grad, H.padded_rows(pr["da3"], c.p3, 0.0).to(BF16).view(a3.shape))
    _check_equal(errors, "da4", a4.grad, H.padded_rows(pr["da4"], c.p4, 0.0).to(BF16).view(a4.shape))
    _check_equal(errors, "dw5", conv5.weight.grad, pr["dw5"].float().view(1, c4, 1, 1))
    _check_equal(errors, "db5", conv5.bias.grad, pr["db5"].float())
    _report(errors)


def test_corner_score_train_rejects_documented_shapes():
    """c4 = 64, fh = 132 and fh % 4 != 0 return MMT_EBADARG (before any launch: the outputs stay NaN)."""
    L = _lib()
    c = H.SCORE_CASES[0]
    t = _score_buffers(c, H.score_problem(c))
    outs = [H.poison(64, 64, BF16).cuda() for _ in range(3)] + [H.poison(64, 1, F32).cuda() for _ in range(3)]
    dx4, da3, da4, dw, db, ws = outs
    for bad in H.SCORE_REJECTED:
        fh, c4 = bad.get("fh", c.fh), bad.get("c4", c.c4)
        rc = L.LIB.mmt_corner_score_train_bwd(t["dsm"].data_ptr(), t["x4"].data_ptr(), t["w5"].data_ptr(), dx4.data_ptr(),
                                              da3.data_ptr(), 1, da4.data_ptr(), 1, dw.data_ptr(), db.data_ptr(), ws.data_ptr(),
                                              c.B, fh, c4, _st())
        assert rc == H.EBADARG, (bad, rc)
        if fh % 4:
            rc = L.LIB.mmt_corner_score_train(t["x4"].data_ptr(), t["w5"].data_ptr(), t["b5"].data_ptr(), t["a3"].data_ptr(), 1,
                                              t["a4"].data_ptr(), 1, ws.data_ptr(), c.B, fh, c4, _st())
            assert rc == H.EBADARG, (bad, rc)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs)


# ------------------------------------------------------------------------------------------------ 5. corner boxes
def _boxes(tl, br, B, fh, stride, img, dxy):
    L = _lib()
    n = fh * fh
    tld, brd = H.image(B, n, tl, F32).cuda(), H.image(B, n, br, F32).cuda()
    xyxy, stats = H.poison(B, 4, F32).cuda(), H.poison(B, 8, F32).cuda()
    L.check(L.LIB.mmt_corner_boxes(tld.data_ptr(), brd.data_ptr(), xyxy.data_ptr(), stats.data_ptr(), B, fh, stride, img, _st()),
            "mmt_corner_boxes")
    dxyd = H.image(B, 4, dxy, F32).cuda()
    dtl, dbr = H.poison(B, n, F32).cuda(), H.poison(B, n, F32).cuda()
    L.check(L.LIB.mmt_corner_boxes_bwd(tld.data_ptr(), brd.data_ptr(), stats.data_ptr(), dxyd.data_ptr(), dtl.data_ptr(),
                                       dbr.data_ptr(), B, fh, stride, img, _st()), "mmt_corner_boxes_bwd")
    torch.cuda.synchronize()
    return xyxy, stats, dtl, dbr


@pytest.mark.parametrize("fh,stride", H.BOX_CASES)
def test_corner_boxes_peak_maps_exact(fh, stride):
    """Logit 120 at one pixel, 0 elsewhere (every other weight is 0 in fp32): xyxy = stride * (col, row) of the peak
    / img and the saved statistics bit for bit, the peak at the four corners, indices 255 and 256 and the last one,
    one map per peak, another peak for br than for tl; the backward is exactly 0.  HipOps.corner_boxes agrees."""
    from mmt_amd.train import HipOps
    pr = H.peak_problem(fh, stride)
    B, n = len(pr["pt"]), fh * fh
    dxy = torch.arange(1, 4 * B + 1).view(B, 4).float()
    xyxy, stats, dtl, dbr = _boxes(pr["tl"], pr["br"], B, fh, stride, pr["img"], dxy)
    errors = []
    _check(errors, "xyxy", xyxy, H.image(B, 4, pr["xyxy"], F32))
    _check(errors, "stats", stats, H.image(B, 8, pr["stats"], F32))
    _check(errors, "d tl", dtl, H.image(B, n, torch.zeros(B, n), F32))
    _check(errors, "d br", dbr, H.image(B, n, torch.zeros(B, n), F32))
    got = HipOps.corner_boxes(pr["tl"].cuda(), pr["br"].cuda(), fh, stride, pr["img"])
    _check_equal(errors, "HipOps.corner_boxes", got, pr["xyxy"])
    _report(errors)


@pytest.mark.parametrize("fh,stride", H.BOX_CASES)
def test_corner_boxes_constant_maps(fh, stride):
    """Constant maps: the softmax is uniform (the saved maximum and sum exactly the constant and n), E[x] = E[y] =
    stride (fh - 1) / 2 within (ceil(n / 256) + 12) fp32 half-ulps (head_probes.boxes_const_bar: the divide, each
    term's product, a thread's sequential adds, the block sum's 8 levels, the scaling), d score within the same bar
    (+ 8 half-ulps of its own steps) of the float64 closed form's magnitudes."""
    pr = H.const_problem(fh, stride)
    B, n = pr["tl"].shape
    xyxy, stats, dtl, dbr = _boxes(pr["tl"], pr["br"], B, fh, stride, pr["img"], pr["dxy"])
    errors = []
    st = stats.cpu()[:B].view(B, 2, 4)
    assert torch.equal(st[:, :, 0], torch.tensor([[3.0, -7.0]] * B)) and torch.equal(st[:, :, 1], torch.full((B, 2), float(n)))
    assert bool(torch.isnan(xyxy.cpu()[B:]).all() and torch.isnan(dtl.cpu()[B:]).all() and torch.isnan(dbr.cpu()[B:]).all())
    worst = _check_bar(errors, "xyxy", xyxy[:B], pr["xyxy"], H.boxes_const_bar(fh) * pr["xyxy"].abs())
    wd = max(_check_bar(errors, "d tl", dtl[:B], pr["d"][0], pr["dbar"][0]), _check_bar(errors, "d br", dbr[:B], pr["d"][1], pr["dbar"][1]))
    print("corner boxes fh %d: constant-map expectation %.3f of its bar (%.3g relative), d score %.3f of its bar"
          % (fh, worst, H.boxes_const_bar(fh), wd))
    _report(errors)
