"""The corner-head probes themselves (tests/head_probes.py), on the CPU: every reference stays inside the bounds
that make equality the right bar, the shape lists cover the edge classes they claim (computed from the shapes),
one removed, doubled or displaced term changes the expected output at or above the bar, and no probe excludes
any element of a compared tensor."""
import os

import pytest
import torch
import torch.nn.functional as F

import gemm_probes as P
import head_probes as H
from conftest import ROOT


def _src(name):
    return open(os.path.join(ROOT, "multi-modal-tracking_amd", "csrc", name)).read()


def test_constants_match_the_library_sources():
    hdr = open(os.path.join(ROOT, "include", "mmt_hip.h")).read()
    assert "#define MMT_EBADARG (%d)" % H.EBADARG in hdr
    bn = _src("batchnorm.hip")
    assert "BN_THREADS = %d" % H.BN_THREADS in bn and "BN_FCH = 32" in bn and H.BN_FLANES == H.BN_THREADS // 32
    assert "const int64_t nb = (M + 31) / 32;" in bn and "nb < 256 ? nb : 256" in bn
    assert "k + 7 * BN_FLANES < nblk; k += 8 * BN_FLANES" in bn
    assert "CB_T = %d" % H.CB_T in _src("loss.hip")
    head = _src("head.hip")
    assert "fh > 128" in head and "c4 > 63" in head and "red[16][65]" in head


# ------------------------------------------------------------------------------------------------ conv3x3
def test_conv_shapes_cover_the_edge_classes():
    seen = set()
    for c in H.CONV_CASES:
        assert c.Cin % 8 == 0 and c.up in (1, 2, 4)
        for s in H.conv_gemm_specs(c):
            assert P.kernel_of(s) is not None and P.kernel_of(s)[0] == "glds", (c, s)
        seen |= H.conv_classes(c)
    assert H.CONV_REQUIRED <= seen, H.CONV_REQUIRED - seen
    assert {c.Cin for c in H.CONV_CASES} >= {8, 24, 48, 96}
    assert any(c.keep_pad and c.Cp - c.Cout > 1 for c in H.CONV_CASES)
    for c in H.CONV_CASES:  # the cases stay small: a few milliseconds of GPU time each
        assert c.M * max(c.Cin, c.Cp) * 9 <= 1 << 19


@pytest.mark.parametrize("c", H.CONV_CASES)
def test_conv_reference_is_exact(c):
    pr = H.conv_problem(c)
    for name in ("y", "dx"):
        assert H.bf16_exact(pr[name]), (name, float(pr[name].abs().max()))
    for name in ("dw", "db"):
        assert H.f32_exact(pr[name]), name
    assert int((pr["x"] != 0).sum()) == c.B * c.Hi * c.Hi and int((pr["dy"] != 0).sum()) == c.M  # one-hot, never 0
    assert int(pr["w"].abs().min()) >= 1 and int(pr["w"].abs().max()) <= 2 and bool((pr["pad_fill"] != 0).all())
    for t in (pr["x"], pr["dy"], pr["w"], pr["b"]):
        assert torch.equal(t.to(torch.bfloat16).to(torch.int64), t)
    # worst-case partial sums: 9 taps x amplitude 3 x |w| 2 + |bias| 8 (y); 9 x 2 x 2 = 36 a dX pixel, which bf16
    # stores exactly before the block sum; dW below M * 3 * 2
    assert 9 * 3 * 2 + 8 <= 256 and c.M * 6 < 2 ** 24
    # the same numbers from the GEMM probes' own conv reference, on the operand layouts the GEMMs read: the forward
    # on wf, and dX as the flipped-tap conv (conv_k3 2) of dY on wb, before the block sums
    wf, wb = H.conv_layouts(c, pr["w"])
    y2 = P.conv_ref(pr["x"][None], wf[None], c.Ho, c.up, c.Cin, 1)[0].view(c.B, c.Ho, c.Ho, c.Cp)
    bias = torch.zeros(c.Cp, dtype=torch.int64)
    bias[:c.Cout] = pr["b"]
    assert torch.equal((y2 + bias).double(), pr["y_pad"])
    dxu = P.conv_ref(pr["dy_pad"][None], wb[None], c.Ho, 1, c.Cp, 2)[0].view(c.B, c.Ho, c.Ho, c.Cin)
    assert int(dxu.abs().max()) <= 36
    assert torch.equal(H.block_sum(dxu, c.up).double(), pr["dx"])
    # dY's padding channels never reach dX (wb's padding columns are 0) nor dW[:Cout] / db[:Cout]
    if c.Cp > c.Cout:
        filled = pr["dy_pad"].clone()
        filled[..., c.Cout:] = pr["pad_fill"]
        dxf = P.conv_ref(filled[None], wb[None], c.Ho, 1, c.Cp, 2)[0].view(c.B, c.Ho, c.Ho, c.Cin)
        assert torch.equal(dxf, dxu)


def test_conv_probe_discriminates():
    """One tap at a corner pixel removed, doubled or displaced; one element of a block sum dropped; flip = False."""
    for c in (H.CONV_CASES[7], H.CONV_CASES[8], H.CONV_CASES[9]):
        pr = H.conv_problem(c)
        xu = H.up_nchw(pr["x"], c.up)
        w = pr["w"].double()
        for (yy, xx) in ((0, 0), (c.Ho - 1, c.Ho - 1)):           # corner pixels of the last image
            b = c.B - 1
            for (ky, kx) in ((1, 1), (2, 2) if yy == 0 else (0, 0)):  # taps inside the map at that corner
                term = w[:, :, ky, kx] @ xu[b, :, yy + ky - 1, xx + kx - 1]
                assert term.abs().min() >= 1                         # removing or doubling it moves every channel
            moved = F.conv2d(xu.roll(1, 3), w, pr["b"].double(), padding=1).permute(0, 2, 3, 1)
            if c.Cout >= 8:                                          # the taps read one pixel aside
                assert (moved[b, yy, xx] != pr["y"][b, yy, xx]).any()
            assert (moved != pr["y"]).float().mean().item() >= 0.5
        wf, wb = H.conv_layouts(c, pr["w"])
        noflip = P.conv_ref(pr["dy_pad"][None], wb[None], c.Ho, 1, c.Cp, 1)[0].view(c.B, c.Ho, c.Ho, c.Cin)
        assert (H.block_sum(noflip, c.up).double() != pr["dx"]).float().mean().item() >= 0.5
        dxu = P.conv_ref(pr["dy_pad"][None], wb[None], c.Ho, 1, c.Cp, 2)[0].view(c.B, c.Ho, c.Ho, c.Cin)
        assert int(dxu.abs().min()) >= 0 and (dxu != 0).float().mean().item() >= 0.9
        if c.up > 1:                                                 # up * up - 1 elements summed
            short = dxu.clone()
            short[:, c.up - 1::c.up, c.up - 1::c.up] = 0
            assert (H.block_sum(short, c.up).double() != pr["dx"]).float().mean().item() >= 0.9
        # a pixel dropped from dW / db: the bias gradient of its channel moves by its amplitude
        assert int(pr["dy"].sum(-1).abs().min()) >= 1


def test_direct_kernel_probes_are_exact_and_cover_the_workgroup_edges():
    chunks = []
    for case in H.UPSUM_CASES:
        src, ref = H.upsum_problem(case)
        assert H.bf16_exact(ref.double()) and int(src.abs().min()) >= 1
        assert torch.equal(src.to(torch.bfloat16).to(torch.int64), src)
        chunks.append(ref.numel() // 8)
        if case[4] > 1:  # one element of a block dropped: every sum moves
            assert bool(((ref - src[:, ::case[4], ::case[4]]) != ref).all())
    assert any(n < 256 for n in chunks) and any(n % 256 == 0 for n in chunks) and any(n > 256 and n % 256 for n in chunks)
    assert {c[4] for c in H.UPSUM_CASES} == {1, 2, 4} and any(c[1] != c[2] for c in H.UPSUM_CASES)
    chunks = []
    for case in H.IM2COL_CASES:
        B, Hh, W, C, up = case
        src, cm, tm = H.im2col_problem(case)
        assert cm.shape == tm.shape == (B * Hh * W, 9 * C) and H.bf16_exact(cm)
        # column c * 9 + tap of pixel (y, x) is the tap's pixel of the upsampled map, 0 outside it
        xu = H.up_nchw(src, up)
        y, x, ch, tap = Hh - 1, 0, C - 1, 2                          # (ky, kx) = (0, 2): above-right of the bottom-left pixel
        assert cm[(B - 1) * Hh * W + y * W + x, ch * 9 + tap] == (xu[B - 1, ch, y - 1, x + 1] if Hh > 1 and W > 1 else 0)
        assert torch.equal(tm[:, tap * C + ch], cm[:, ch * 9 + tap])
        chunks.append(B * Hh * W * C // 8)
    assert any(n < 256 for n in chunks) and any(n % 256 == 0 for n in chunks) and any(n > 256 and n % 256 for n in chunks)
    assert {c[4] for c in H.IM2COL_CASES} == {1, 2, 4} and any(c[1] != c[2] for c in H.IM2COL_CASES)
    chunks = []
    for case in H.ADDUP_CASES:
        a, b, dout, out, da = H.addup_problem(case)
        assert H.bf16_exact(out.double()) and H.bf16_exact(da.double()) and int(dout.abs().min()) >= 1
        chunks.append(b.numel() // 8)
        if case[4] > 1:
            assert bool(((da - dout[:, ::case[4], ::case[4]]) != da).all())
    assert any(c[3] == 8 for c in H.ADDUP_CASES) and any(n > 256 and n % 256 for n in chunks)


# ------------------------------------------------------------------------------------------------ batch norm
def test_bn_shapes_cover_the_thresholds():
    assert {1, 31, 32, 33, 8191, 8192, 8193} <= set(H.BN_MS)
    assert any(M > 8192 and M % 256 for M in H.BN_MS)
    nb = {M: H.bn_blocks(M) for M in H.BN_MS}
    assert nb[32] == 1 and nb[33] == 2 and nb[8191] == nb[8192] == nb[8193] == 256 and nb[1] == 1
    paths = {M: H.bn_lane_path(n) for M, n in nb.items()}
    assert any(all(p == 0 for p, _ in ps) for ps in paths.values())                    # only the tail loop
    assert any(ps == {(1, 0)} for ps in paths.values())                                # exactly one unrolled pass
    assert any(all(p >= 1 for p, _ in ps) and any(t for _, t in ps) for ps in paths.values())  # a pass and a tail
    assert any({p for p, _ in ps} == {0, 1} for ps in paths.values())                  # lanes on either side
    assert set(H.BN_CP) == {(1, 8), (8, 8), (50, 56), (48, 48), (24, 24), (1032, 1032), (2048, 2048)}
    c8 = [p // 8 for _, p in H.BN_CP]
    assert any(256 % n == 0 for n in c8) and any(256 % n and n not in (6, 12) and n <= 128 for n in c8)
    assert any(n > 128 and 256 // n == 1 for n in c8) and any(p > C and C % 8 for C, p in H.BN_CP)
    for C, pitch in H.BN_CP:
        cases = H.bn_cases(C, pitch)
        kinds = {(c.kind, c.training, c.relu) for c in cases}
        assert {("balanced", 1, 1), ("odd", 1, 1), ("offset", 1, 1), ("general", 0, 1)} <= kinds
        assert all(c.M % 2 == 0 for c in cases if c.kind in ("balanced", "offset"))
        assert sum(c.M * c.pitch for c in cases) <= 12 << 20
        if pitch <= 256:
            assert {c.M for c in cases if c.training and c.relu} == set(H.BN_MS)
            assert any(not c.training and not c.relu for c in cases) and any(c.training and not c.relu for c in cases)


@pytest.mark.parametrize("case", [H.BNCase(8192, 50, 56, "offset"), H.BNCase(2048, 24, 24), H.BNCase(34, 1032, 1032, "offset"),
                                  H.BNCase(2048, 48, 48, relu=0)])
def test_bn_balanced_census_is_exact(case):
    pr = H.bn_problem(case)
    C = case.C
    x = pr["x"]
    assert int(x.abs().min()) >= 1 and torch.equal(x.to(torch.bfloat16).to(torch.int64), x)
    assert torch.equal(pr["var"], torch.ones(C, dtype=torch.float64)) and torch.equal(pr["inv"], torch.full((C,), 0.5, dtype=torch.float64))
    assert torch.equal(pr["mean"], pr["mean"].round()) and float(pr["mean"].abs().max()) <= 254
    for name in ("y", "dbeta", "sc", "sh"):
        assert torch.equal(pr[name], pr[name].round()), name
    assert H.bf16_exact(pr["y"]) and torch.equal(pr["dgamma"] * 2, (pr["dgamma"] * 2).round())
    if case.relu:  # both sides of the mask, and pre-activations exactly at the threshold
        assert 0.2 <= pr["mask"].float().mean().item() <= 0.8 and pr["margin"] == 0.0
    # the pivoted sums of the kernel: d = x - x[0] in {0, +-2}: exact in fp32 in any order, where the plain sum of
    # squares of the offset case is not
    d = (x[:, :C] - x[0, :C]).double()
    assert float((d * d).sum(0).max()) < 2 ** 24
    if case.kind == "offset" and case.M >= 8192:
        assert float((x[:, :C].double() ** 2).sum(0).max()) > 2 ** 24
    assert torch.equal(pr["rm1"].double(), 0.75 * pr["rm0"] + 0.25 * pr["mean"])
    # padding channels: non-zero in x and dY, zero in y and dx
    if case.pitch > C:
        assert int(x[:, C:].abs().min()) >= 1 and float(pr["y"][:, C:].abs().max()) == 0 and float(pr["dx"][:, C:].abs().max()) == 0


def test_bn_one_row_moves_the_mean_a_hundred_bars():
    """At the largest M, dropping or doubling any one row moves every channel's mean by >= 100 x the bar it is
    compared at, and the bias gradient (an exact integer sum) by at least 1 wherever the row passes the ReLU."""
    M = max(H.BN_MS)
    for kind in ("odd", "general"):
        case = H.BNCase(M, 50, 56, kind)
        pr = H.bn_problem(case)
        assert not pr["exact"] and pr["margin"] >= 1e-3
        x = pr["x"][:, :50].double()
        bar = H.bn_mean_bar(pr["mean"])
        tot = x.sum(0)
        for sign, n in ((-1, M - 1), (1, M + 1)):
            moved = ((tot + sign * x) / n - pr["mean"]).abs()     # [M][C]: the mean without / with row m twice
            assert bool((moved >= 100 * bar).all()), (kind, sign, float((moved / bar).min()))
        assert float((pr["mean"] - pr["mean"].float().double()).abs().max()) > 0   # not representable: a bar is needed
        assert 0.2 <= pr["mask"].float().mean().item() <= 0.8 and int(pr["dy"].abs().min()) >= 1
    for C, pitch in H.BN_CP:
        for case in H.bn_cases(C, pitch):
            if not H.bn_exact(case) and case.M * pitch <= 1 << 19:
                assert H.bn_problem(case)["margin"] >= 1e-3, case
    assert H.BN_MEAN_ULPS <= 2 and H.BN_INV_ULPS <= 4


# ------------------------------------------------------------------------------------------------ corner score
def test_score_shapes_and_exactness():
    assert {c.fh for c in H.SCORE_CASES} == {4, 12, 128} and {c.c4 for c in H.SCORE_CASES} == {8, 48, 56}
    bands = {c.bands for c in H.SCORE_CASES}
    assert any(b < 16 for b in bands) and 16 in bands and 17 in bands and any(b > 32 for b in bands)
    assert any(c.fh == 4 for c in H.SCORE_CASES)                                    # one band an image
    assert any((c.B * c.fh * c.fh) % 256 for c in H.SCORE_CASES if c.fh == 12)      # the forward's ragged tail
    assert {(c.p3, c.p4) for c in H.SCORE_CASES} >= {(1, 1), (8, 8), (1, 8), (8, 1)}
    for c in H.SCORE_CASES:
        pr = H.score_problem(c)
        for name in ("dx4", "da3", "da4"):
            assert H.bf16_exact(pr[name].double()), (c, name)
        for name in ("sm", "dw5", "db5"):
            assert H.f32_exact(pr[name].double()), (c, name)
        assert int(pr["dsm"].abs().min()) >= 1 and int((pr["x4"] != 0).sum()) == c.B * c.fh * c.fh
        # one band partial dropped (or added twice): db5 moves, by an odd number
        assert bool((pr["band_b"] % 2 == 1).all()) and pr["band"].shape == (c.bands, c.c4)
        # one element of a 4x4 / 2x2 block dropped: the sum moves
        assert bool(((pr["da3"] - pr["dsm"][:, ::4, ::4]) != pr["da3"]).all())
        assert bool(((pr["da4"] - pr["dsm"][:, 1::2, 1::2]) != pr["da4"]).all())
        # against fp64 autograd of the composition the kernel replaces
        x = pr["x4"].double().requires_grad_(True)
        w, b = pr["w5"].double().requires_grad_(True), pr["b5"].double().requires_grad_(True)
        a3, a4 = pr["a3"].double().requires_grad_(True), pr["a4"].double().requires_grad_(True)
        up = lambda t, f: F.interpolate(t[:, None], scale_factor=f)[:, 0]  # noqa: E731
        sm = F.linear(x, w[None], b)[..., 0] + up(a3, 4) + up(a4, 2)
        sm.backward(pr["dsm"].double())
        for got, ref in ((sm.detach(), pr["sm"]), (x.grad, pr["dx4"]), (a3.grad, pr["da3"]), (a4.grad, pr["da4"]),
                         (w.grad, pr["dw5"]), (b.grad, pr["db5"])):
            assert torch.equal(got, ref.double())
    assert len(H.SCORE_REJECTED) == 3


# ------------------------------------------------------------------------------------------------ corner boxes
def test_boxes_probes():
    ns = [fh * fh for fh, _ in H.BOX_CASES]
    assert [fh for fh, _ in H.BOX_CASES] == [7, 16, 17, 80]
    assert any(n < 256 for n in ns) and 256 in ns and any(n > 256 and n % 256 for n in ns)
    assert torch.exp(torch.tensor(-H.PEAK_LOGIT)).item() == 0.0
    for fh, stride in H.BOX_CASES:
        n = fh * fh
        ps = H.peak_pixels(fh)
        assert {0, fh - 1, n - fh, n - 1} <= set(ps) and (n <= 256 or {255, 256} <= set(ps)) and (n < 256 or 255 in ps)
        pr = H.peak_problem(fh, stride)
        assert not bool((pr["pt"] == pr["pb"]).any())
        # fp64 soft-argmax of the peak maps: exactly the peak's coordinates; the peak moved by one moves them
        for m, p in ((pr["tl"], pr["pt"]), (pr["br"], pr["pb"])):
            sm = torch.softmax(m.double(), 1)
            k = torch.arange(n)
            ex, ey = (sm * (stride * (k % fh))).sum(1), (sm * (stride * (k // fh))).sum(1)
            # (what is left of the other weights, ~1e-50, is 0 in the stored type)
            assert torch.equal(ex.float(), stride * (p % fh).float()) and torch.equal(ey.float(), stride * (p // fh).float())
            q = (p + 1) % n
            assert bool(((stride * (q % fh) != ex) | (stride * (q // fh) != ey)).all())
        assert bool((pr["e"] == pr["e"].round()).all()) and float(pr["e"].max()) == stride * (fh - 1)
        cp = H.const_problem(fh, stride)
        sm = torch.softmax(cp["tl"].double(), 1)
        k = torch.arange(n)
        assert abs(float((sm * (stride * (k % fh))).sum(1)[0]) / cp["img"] - float(cp["xyxy"][0, 0])) <= 1e-12
        # autograd of the fp64 composition gives the closed form
        t = cp["tl"].double().requires_grad_(True)
        s = torch.softmax(t, 1)
        xy = torch.stack([(s * (stride * (k % fh))).sum(1), (s * (stride * (k // fh))).sum(1)], 1) / cp["img"]
        xy.backward(cp["dxy"][:, :2].double())
        assert float((t.grad - cp["d"][0]).abs().max()) <= 1e-12 * max(1.0, float(cp["d"][0].abs().max()))
        # the strided loop's tail dropped (k >= 256 floor(n / 256)) moves the expectation by far more than the bar
        if n % 256 and n > 256:
            kept = k < n // 256 * 256
            short = float((sm[0] * kept * (stride * (k // fh))).sum()) / cp["img"]
            assert abs(short - float(cp["xyxy"][0, 1])) >= 100 * H.boxes_const_bar(fh) * float(cp["xyxy"][0, 1])
        assert H.boxes_const_bar(fh) <= 40 * H.U32


def test_nothing_is_excluded():
    """Storage images carry the whole expectation: the body everywhere inside, NaN outside, and same() looks at
    every element (the excluded share is 0)."""
    body = torch.arange(24.0).view(3, 8)
    img = H.image(3, 8, body, torch.bfloat16)
    assert img.shape == (3 + H.GUARD, 8) and torch.isnan(img[3:]).all() and torch.equal(img[:3].float(), body)
    assert P.same(img, img)
    for i, j in ((0, 0), (2, 7), (3, 0), (3 + H.GUARD - 1, 7)):
        hit = img.clone()
        hit[i, j] = 1000.0
        assert not P.same(hit, img), (i, j)
    miss = img.clone()
    miss[1, 1] = H.NAN
    assert not P.same(miss, img)
    assert torch.isnan(H.poison(3, 8, torch.float32)).all()
    rows = H.padded_rows(torch.tensor([5, 6]), 8, 0.0)
    assert rows.shape == (2, 8) and rows[:, 0].tolist() == [5.0, 6.0] and float(rows[:, 1:].abs().max()) == 0
    assert H.padded_rows(torch.tensor([5]), 1, H.NAN).tolist() == [[5.0]]
    ref = torch.tensor([1.0, -300.0, 0.0], dtype=torch.float64)
    bar = H.bf16_bar(ref, torch.tensor(1e-6, dtype=torch.float64))
    assert bool((bar >= (ref.bfloat16().double() - ref).abs()).all()) and float(bar[2]) <= 2e-6
