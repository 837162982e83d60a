"""The deformable-attention probes themselves (tests/msda_probes.py), on the CPU: the constants are the sources',
the operands and references of the exact families are exact (so equality is the right bar on the device), the
position classes and bucket lengths the probes claim are computed from their inputs, one dropped, displaced or
mis-weighted term moves the named output by at least the comparison's resolution, and the C ABI rejects every
host-checkable bad argument before any launch."""
import os

import pytest
import torch

import msda_probes as M
from conftest import ROOT

F64, F32, BF16, F16 = M.F64, M.F32, M.BF16, M.F16
IDS = M.key_id


def test_constants_match_the_library_sources():
    hdr = open(os.path.join(ROOT, "include", "mmt_hip.h")).read()
    assert "#define MMT_EBADARG (%d)" % M.EBADARG in hdr
    src = open(os.path.join(ROOT, "multi-modal-tracking_amd", "csrc", "msda.hip")).read()
    assert "MT_NQ_MAX = %d" % M.NQ_MAX in src and M.NQ_MAX == 484 and max(hw for hw, _ in M.BAR_SIZES) ** 2 == M.NQ_MAX
    assert "constexpr int BUCKET_LONG = %d;" % M.BUCKET_LONG in src and M.BUCKET_LONG == 24
    assert "constexpr int MT_VT = %d;" % M.VT in src and M.VT == 1024
    assert "MT_NH = %d, MT_NL = %d, MT_NP = %d, MT_DH = %d" % (M.NH, M.NL, M.NP, M.DH) in src
    assert "const int words = (nq + 1) / 2;" in src and "per = (items + MT_VT - 1) / MT_VT * 64" in src
    assert "if (len > BUCKET_LONG)" in src
    # the sizes the issue sets
    assert {hw for hw, _ in M.EXACT_SIZES} == {4, 8, 16} and {B for _, B in M.EXACT_SIZES} == {1, 3}
    assert all(hw <= 8 for hw, B in M.EXACT_SIZES if B == 3)
    assert {hw for hw, _ in M.BAR_SIZES} == {5, 20, 22} and {B for _, B in M.BAR_SIZES} == {1, 2}
    assert (5 * 5) % 2 == 1 and all(B <= 3 and hw <= 22 for _, hw, B, _ in M.EXACT_KEYS + M.BAR_KEYS)


# ------------------------------------------------------------------------------------------------ operands
def _multiple(t, q):
    return bool((t / q == (t / q).round()).all())


@pytest.mark.parametrize("key", M.EXACT_KEYS, ids=IDS)
def test_exact_operands(key):
    pr = M.problem(key)
    hw, nq = pr["hw"], pr["nq"]
    assert hw & (hw - 1) == 0
    for name in ("value", "off", "logits", "g"):
        t = pr[name]
        assert torch.equal(t.to(BF16).double(), t), name
    assert torch.equal(pr["value"].to(F16).double(), pr["value"])  # the fp16 inference path takes the same values
    assert _multiple(pr["off"], pr["q_off"]) and _multiple(pr["value"], 1.0) and _multiple(pr["g"], 1.0)
    assert bool((pr["g"] != 0).all()) and float(pr["g"].abs().max()) <= 3
    assert float(pr["value"].abs().max()) <= (125 if pr["family"] == "gather" else 4)
    assert set(pr["logits"].unique().tolist()) <= {0.0, -200.0}
    a = torch.softmax(pr["logits"].float(), -1)
    assert set(a.unique().tolist()) <= {0.0, 0.125, 0.25, 0.5, 1.0}
    assert _multiple(a.double(), pr["q_a"]) and bool((a.sum(-1) == 1).all())
    if pr["family"] == "gather":
        assert bool(((a == 1).sum(-1) == 1).all())
    else:
        assert {0.125, 0.25, 0.5} <= set(a.unique().tolist())
    # (ref + off / hw) * hw - 0.5 in fp32 is the query's pixel plus the offset, exactly
    loc = pr["ref"].view(1, nq, 1, 1, 1, 2) + pr["off"].float() / hw
    c32 = loc * hw - 0.5
    q = torch.arange(nq)
    want = torch.stack([q % hw, q // hw], -1).double().view(1, nq, 1, 1, 1, 2) + pr["off"]
    assert c32.dtype == F32 and torch.equal(c32.double(), want)
    assert torch.equal(torch.stack(M.coords(pr), -1), want)


def _abs_bounds(pr):
    """Sum of |terms| of every output element, or a bound on it.  out and gv: the oracle on |value| and |grad_out|
    (every weight is >= 0).  goff: hw * sum over 64 channels and four taps of |coefficient| |v| |g| a, the four
    coefficients of an axis summing to 2.  gawl: a_i gaw_i and a_i a_j gaw_j over j, |gaw| <= 64 max|g| max|v|."""
    r = M.run_oracle(dict(pr, value=pr["value"].abs(), g=pr["g"].abs()))
    vmax, gmax, amax = float(pr["value"].abs().max()), float(pr["g"].abs().max()), float(M.weights(pr).max())
    return dict(out=float(r["out"].max()), gv=float(r["gv"].max()), goff=2.0 * pr["hw"] * M.DH * gmax * vmax * amax,
                gawl=2.0 * M.DH * gmax * vmax * amax)


@pytest.mark.parametrize("key", M.EXACT_KEYS, ids=IDS)
def test_exact_references(key):
    """Every term of every sum is a multiple of the product of its operands' quanta and sum |terms| stays below 2^24
    of them: any fp32 summation order is exact.  The oracle in fp32 then equals the oracle in fp64 bit for bit."""
    pr, ref = M.problem(key), M.reference(key)
    q_w, q_d, q_a = pr["q_off"] ** 2, pr["q_off"], pr["q_a"]
    quanta = dict(out=q_w * q_a, gv=q_w * q_a, goff=q_d * q_a, gawl=q_w * q_a * q_a)
    bounds = _abs_bounds(pr)
    for name in M.OUTPUTS:
        assert bounds[name] / quanta[name] < 2 ** 24, (name, bounds[name] / quanta[name])
        assert _multiple(ref[name] if name != "goff" else ref["gl"], quanta[name]), name
        assert float(ref[name].abs().max()) <= bounds[name], name
    r32 = M.run_oracle(pr, F32)
    for name in M.OUTPUTS + ("gl", "ga"):
        assert r32[name].dtype == F32 and torch.equal(r32[name].double(), ref[name]), name
        assert torch.equal(ref[name].float().double(), ref[name]), name
    assert any(bool((ref[n] != 0).any()) for n in M.OUTPUTS)
    assert bool((ref["out"] != 0).any()) and bool((ref["gv"] != 0).any()) and bool((ref["goff"] != 0).any())
    if pr["family"] != "gather":  # one-hot weights: the softmax backward is a (ga - a ga) = 0 in every slot
        assert bool((ref["gawl"] != 0).any())


# ------------------------------------------------------------------------------------------------ coverage
@pytest.mark.parametrize("hw,B", M.EXACT_SIZES)
def test_position_classes_are_covered(hw, B):
    pairs = M.class_pairs(M.problem(("gather", hw, B, "")))
    need = {(a, b) for a in M.INT_CLASSES for b in M.INT_CLASSES}
    assert need <= pairs, sorted(need - pairs)
    pairs = M.class_pairs(M.problem(("blend", hw, B, "")))
    need = {(a, b) for a in range(8) for b in range(8)}
    assert need <= pairs, sorted(need - pairs)


@pytest.mark.parametrize("hw,B", M.EXACT_SIZES)
def test_bucket_lengths_are_covered(hw, B):
    nq = hw * hw
    n = {p: M.bucket_lengths(M.problem(("buckets", hw, B, p))) for p in M.BUCKET_PATTERNS}
    assert int(n["pixel"].max()) == 4 * nq and int((n["pixel"] == 4 * nq).sum()) >= B * M.NH * M.NL
    assert int((n["half"] == 4 * nq).sum()) == 4 * B * M.NH * M.NL and int((n["half"] == 0).sum()) == (nq - 4) * B * M.NH * M.NL
    assert int(n["zero"].min()) == 4 and int(n["zero"].max()) == 16
    long = n["long"]
    for want in (0, 1, M.BUCKET_LONG, M.BUCKET_LONG + 1):
        assert int((long == want).sum()) >= B * M.NH * M.NL, want
    assert set(long.unique().tolist()) == {0, 1, M.BUCKET_LONG, M.BUCKET_LONG + 1}
    seen = set().union(*[set(t.unique().tolist()) for t in n.values()])
    assert {0, 1, M.BUCKET_LONG, M.BUCKET_LONG + 1, 4 * nq} <= seen
    for p in ("pixel", "half", "long"):  # lists fed by the item runs of more than one wave
        assert M.bucket_wave_spread(M.problem(("buckets", hw, B, p))) > 1, p
    # every entry of a `long` list has a weight that matters: tap 0 of an integer position
    valid, _, wt = M.tap_table(M.problem(("buckets", hw, B, "long")))
    assert bool(((wt == 1) | (wt == 0))[valid].all()) and int((wt[valid] == 1).sum()) * 2 >= int(valid.sum())


@pytest.mark.parametrize("key", M.BAR_KEYS, ids=IDS)
def test_bar_problems_keep_their_margin(key):
    pr = M.problem(key)
    hw = pr["hw"]
    for name in ("off", "logits", "g"):
        assert torch.equal(pr[name].to(BF16).double(), pr[name]), name
    assert torch.equal(pr["value"].to(BF16).double(), pr["value"]) and torch.equal(pr["value"].to(F16).double(), pr["value"])
    x, y = M.coords(pr)
    for c in (x, y):
        near = (c - c.round()).abs() < M.MARGIN
        assert int((near & (c.round() >= -1) & (c.round() <= hw)).sum()) == 0
    # fp32 and fp64 decide alike: the coordinates of the fp32 run are within 2^-16 pixel of the fp64 ones
    loc32 = pr["ref"].view(1, pr["nq"], 1, 1, 1, 2) + pr["off"].float() / hw
    c32 = (loc32 * hw - 0.5).double()
    assert float((c32 - torch.stack([x, y], -1)).abs().max()) < 2.0 ** -16
    inside = (x > -1) & (y > -1) & (x < hw) & (y < hw)
    assert 0 < int(inside.sum()) and (pr["variant"] == "collapse" or int((~inside).sum()) > 0)
    if pr["variant"] == "collapse":  # a 2 x 2 (where the point is near a pixel, 3 x 3) patch of a level takes every tap
        n = M.bucket_lengths(pr)
        assert int((n > 0).sum()) <= 9 * pr["B"] * M.NH * M.NL and int(n.max()) >= pr["nq"] > M.BUCKET_LONG
        assert int(n.sum()) == 16 * pr["nq"] * pr["B"] * M.NH * M.NL  # every tap of every sample is in the map
    assert pr["off"].numel() == pr["B"] * pr["nq"] * 128
    d = M.delta(key)
    assert all(d[n] > 0 for n in M.OUTPUTS)


def test_bar_margin_rule_moves_no_sample_across_the_border():
    """The generator's move is 1/8 pixel away from the nearby integer: every sample is still there, its in-range flag
    and its floor are what they were before the move, and only offenders moved."""
    for key in M.BAR_KEYS:
        _, hw, B, variant = key
        pr = M.problem(key)
        before = dict(pr, off=M.bar_unmoved(hw, B, variant)["off"])
        assert before["off"].shape == pr["off"].shape
        cb, ca = torch.stack(M.coords(before), -1), torch.stack(M.coords(pr), -1)
        changed = cb != ca
        assert int(changed.sum()) == pr["moved"] and bool((((ca - cb).abs()[changed] - 0.125).abs() <= 2.0 ** -5).all())
        near = ((cb - cb.round()).abs() < M.MARGIN) & (cb.round() >= -1) & (cb.round() <= hw)
        assert torch.equal(near, changed)
        assert torch.equal((cb > -1) & (cb < hw), (ca > -1) & (ca < hw))
        inside = (ca > -1) & (ca < hw)
        assert torch.equal(cb.floor()[inside & (cb != cb.round())], ca.floor()[inside & (cb != cb.round())])


# ------------------------------------------------------------------------------------------------ negative controls
def restate(pr, mut=None, arg=0):
    """A private restatement of the reference (forward and hand-derived backward, float64), with one mutation:
    drop_tap k, shift_pixel k / shift_row k (tap k reads the next pixel / row), swap_levels, swap_xy, next_weight (a
    sample takes the next point's weight), softmax_skip j (sample j left out of the softmax backward's sum),
    minus_one_inside (the range test's lower `>` as `>=`)."""
    B, hw, nq = pr["B"], pr["hw"], pr["nq"]
    a = M.weights(pr)
    x, y = (t.reshape(B, nq, M.NH, M.NL * M.NP) for t in M.coords(pr))
    if mut == "swap_xy":
        x, y = y, x
    lower = (x >= -1) & (y >= -1) if mut == "minus_one_inside" else (x > -1) & (y > -1)
    inside = lower & (x < hw) & (y < hw)
    x0, y0 = x.floor(), y.floor()
    lw, lh = x - x0, y - y0
    hh, hwt = 1 - lh, 1 - lw
    b, q, m, i = M._grid(B, nq)
    shape = (B, nq, M.NH, M.NL * M.NP)
    lev = (i // M.NP).expand(shape)
    if mut == "swap_levels":
        lev = 1 - lev
    au = torch.roll(a, -1, -1) if mut == "next_weight" else a
    g = pr["g"].view(B, nq, M.NH, 1, M.DH)
    bil = torch.zeros(shape + (M.DH,), dtype=F64)
    ddx, ddy = torch.zeros_like(bil), torch.zeros_like(bil)
    gv = torch.zeros(B, M.NL, nq, M.NH, M.DH, dtype=F64)
    taps = ((0, 0, hh * hwt, -hh, -hwt), (0, 1, hh * lw, hh, -lw), (1, 0, lh * hwt, -lh, hwt), (1, 1, lh * lw, lh, lw))
    for k, (dy, dx, w, cx, cy) in enumerate(taps):
        xi, yi = x0.long() + dx, y0.long() + dy
        if mut == "shift_pixel" and k == arg:
            xi = xi + 1
        if mut == "shift_row" and k == arg:
            yi = yi + 1
        ok = inside & (xi >= 0) & (xi <= hw - 1) & (yi >= 0) & (yi <= hw - 1)
        if mut == "drop_tap" and k == arg:
            ok = torch.zeros_like(ok)
        idx = (b.expand(shape), lev, yi.clamp(0, hw - 1) * hw + xi.clamp(0, hw - 1), m.expand(shape))
        v = pr["value"][idx] * ok[..., None]
        bil += w[..., None] * v
        ddx += cx[..., None] * v
        ddy += cy[..., None] * v
        gv.index_put_(idx, (w * ok * au)[..., None] * g, accumulate=True)
    out = (au[..., None] * bil).sum(3).reshape(B, nq, M.CM)
    gaw = (g * bil).sum(-1)
    gx, gy = hw * au * (g * ddx).sum(-1), hw * au * (g * ddy).sum(-1)
    gl = torch.stack([gx, gy], -1).reshape(B, nq, M.NH, M.NL, M.NP, 2)
    terms = au * gaw
    if mut == "softmax_skip":
        terms = terms.clone()
        terms[..., arg] = 0
    gawl = au * (gaw - terms.sum(-1, keepdim=True))
    return dict(out=out, gv=gv, gl=gl, goff=gl / hw, ga=gaw, gawl=gawl)


def test_restatement_equals_the_oracle():
    for key in M.EXACT_KEYS:
        ref, mine = M.reference(key), restate(M.problem(key))
        for name in M.OUTPUTS + ("gl",):
            assert torch.equal(mine[name], ref[name]), (key, name)
        assert torch.equal(mine["ga"], ref["ga"]), key  # d / d weight of every sample, weighted or not
    for key in M.BAR_KEYS[:4]:
        ref, mine = M.reference(key), restate(M.problem(key))
        for name in M.OUTPUTS:
            assert float((mine[name] - ref[name]).abs().max()) <= 1e-12 * max(1.0, float(ref[name].abs().max())), (key, name)


# (mutation, its argument, family, variant, the output that must move)
CONTROLS = ([("drop_tap", 0, "gather", "", "out"), ("drop_tap", 0, "gather", "", "gv")] +
            [("drop_tap", k, "blend", "", n) for k in range(4) for n in M.OUTPUTS] +
            [("drop_tap", k, "buckets", "half", "gv") for k in range(4)] +
            [("drop_tap", 0, "buckets", p, "gv") for p in ("pixel", "zero", "long")] +
            [(s, k, "blend", "", n) for s in ("shift_pixel", "shift_row") for k in range(4) for n in M.OUTPUTS] +
            [(s, 0, "gather", "", n) for s in ("shift_pixel", "shift_row") for n in ("out", "gv")] +
            [(s, 0, f, "", n) for s in ("swap_levels", "swap_xy", "next_weight") for f in ("gather", "blend")
             for n in ("out", "gv", "goff")] +
            [("next_weight", 0, "blend", "", "gawl"), ("swap_levels", 0, "blend", "", "gawl")] +
            [("softmax_skip", j, "blend", "", "gawl") for j in range(8)] +
            [("minus_one_inside", 0, f, "", "goff") for f in ("gather", "blend")])


@pytest.mark.parametrize("hw,B", M.EXACT_SIZES)
def test_mutations_move_the_exact_references(hw, B):
    """Any change shows under equality: after the single rounding to bf16 (to fp32 for the generic op and the fp32
    inference path, which is implied) at least one element of the named output differs."""
    for mut, arg, family, variant, name in CONTROLS:
        key = (family, hw, B, variant)
        ref, got = M.reference(key), restate(M.problem(key), mut, arg)
        moved = M.expected(got[name], BF16) != M.expected(ref[name], BF16)
        assert bool(moved.any()), (mut, arg, family, variant, name)


@pytest.mark.parametrize("hw,B", M.EXACT_SIZES)
def test_a_sample_at_minus_one_shows_only_in_grad_off(hw, B):
    """A range test that takes a sample at exactly -1 as inside is invisible in the forward, in grad_value and in the
    logit gradient: the sample's only in-map taps are those of column (row) 0, whose bilinear weight is lw = 0 (lh =
    0).  It is visible in grad_off alone, where d bilinear / dx = hh (v(0) - v(-1)) does not vanish with lw."""
    for family in ("gather", "blend"):
        key = (family, hw, B, "")
        pr, ref = M.problem(key), M.reference(key)
        x, y = M.coords(pr)
        on_edge = ((x == -1) & (y > -1) & (y < hw)) | ((y == -1) & (x > -1) & (x < hw))
        assert int((on_edge & (M.weights(pr).view(x.shape) > 0)).sum()) > 0
        got = restate(pr, "minus_one_inside")
        for name in ("out", "gv", "gawl"):
            assert torch.equal(got[name], ref[name]), (family, name)
        moved = M.expected(got["goff"], BF16) != M.expected(ref["goff"], BF16)
        assert bool(moved.any())
        assert bool((moved.reshape(x.shape + (2,)).any(-1) <= on_edge).all())  # only those samples' gradients


@pytest.mark.parametrize("key", [k for k in M.BAR_KEYS if k[1] == 5 or (k[1], k[2]) == (22, 1)], ids=IDS)
def test_mutations_move_the_bar_references(key):
    """Under the bar: at least one element of the named output moves by more than the bf16 bar of the comparison."""
    pr, ref, d = M.problem(key), M.reference(key), M.delta(key)
    cases = ([("drop_tap", k, n) for k in range(4) for n in M.OUTPUTS] +
             [(s, k, n) for s in ("shift_pixel", "shift_row") for k in range(4) for n in M.OUTPUTS] +
             [(s, 0, n) for s in ("swap_levels", "swap_xy", "next_weight") for n in M.OUTPUTS] +
             [("softmax_skip", j, "gawl") for j in range(8)])
    for mut, arg, name in cases:
        got = restate(pr, mut, arg)
        over = (got[name] - ref[name]).abs() / M.bar(ref[name], d[name], BF16)
        assert float(over.max()) > 1.0, (mut, arg, name, float(over.max()))


# ------------------------------------------------------------------------------------------------ host rejections
FAKE = 1 << 20  # 16-byte aligned, never dereferenced: every call below fails validation before a launch


def test_train_entry_points_reject_bad_arguments_on_the_host():
    from mmt_amd._lib import LIB

    def fwd(value=FAKE, off=FAKE, op=128, awl=FAKE, ap=64, ref=FAKE, out=FAKE, B=2, hw=20):
        return LIB.mmt_msda_bimodal_train_fwd(value, off, op, awl, ap, ref, out, B, hw, None)

    def bwd(value=FAKE, off=FAKE, op=128, awl=FAKE, ap=64, ref=FAKE, gout=FAKE, gv=FAKE, goff=FAKE, gawl=FAKE, B=2, hw=20):
        return LIB.mmt_msda_bimodal_train_bwd(value, off, op, awl, ap, ref, gout, gv, goff, gawl, B, hw, None)

    for f, ptrs, a16, a4 in ((fwd, ("value", "off", "awl", "ref", "out"), ("value", "awl", "out"), ("off",)),
                             (bwd, ("value", "off", "awl", "ref", "gout", "gv", "goff", "gawl"),
                              ("value", "awl", "gout", "gawl"), ("off", "goff"))):
        assert f(hw=23) == M.EBADARG and f(hw=22 + 10) == M.EBADARG       # hw * hw > 484
        assert f(hw=0) == M.EBADARG and f(hw=-4) == M.EBADARG and f(B=0) == M.EBADARG and f(B=-1) == M.EBADARG
        for op in (127, 126, 0, -128, 129, 193):                           # off_pitch < 128 or odd
            assert f(op=op) == M.EBADARG, op
        for ap in (63, 56, 0, -64, 65, 68, 196):                           # awl_pitch < 64 or no multiple of 8
            assert f(ap=ap) == M.EBADARG, ap
        for name in ptrs:
            assert f(**{name: None}) == M.EBADARG, name
        for name in a16:
            for d in (2, 4, 8):
                assert f(**{name: FAKE + d}) == M.EBADARG, (name, d)
        for name in a4:
            assert f(**{name: FAKE + 2}) == M.EBADARG, name


def test_inference_entry_point_rejects_bad_arguments_on_the_host():
    from mmt_amd._lib import LIB, MMT_BF16, MMT_F64

    def call(offw=FAKE, value=FAKE, out=FAKE, B=2, hw=20, dtype=MMT_BF16):
        return LIB.mmt_msda_bimodal(offw, value, out, B, hw, dtype, None)

    for name in ("offw", "value", "out"):
        assert call(**{name: None}) == M.EBADARG, name
    for name in ("value", "out"):
        for d in (2, 4, 8):
            assert call(**{name: FAKE + d}) == M.EBADARG, (name, d)
    assert call(B=0) == M.EBADARG and call(hw=0) == M.EBADARG and call(B=-2) == M.EBADARG
    for dtype in (MMT_F64, 4, 7, -1):  # fp32, bf16 and fp16 only
        assert call(dtype=dtype) == M.EBADARG, dtype
