"""Probe inputs and fp64 references of the corner head's training chain (no tests here): _HipConv3x3,
_HipAddUp, mmt_batchnorm_relu / _bwd, mmt_corner_score_train / _bwd and mmt_corner_boxes / _bwd.

Every family uses integer-valued operands chosen so that the kernels' arithmetic is exact: each fp32 partial sum
is an integer far below 2^24 in any order, and each bf16 result an integer of magnitude at most 256 (the
integers bf16 holds exactly), so the expected outputs are known bit for bit and the GPU tests compare with
torch.equal.  The three places where that cannot hold have a bar derived from the kernel's rounding steps,
stated beside the function that computes it: the batch-norm moments when M is odd (BN_MEAN_ULPS, BN_INV_ULPS),
the bf16 dx of the batch norm (bf16_bar) and the soft-argmax of a constant map (boxes_const_bar).

References are plain float64 torch on the CPU.  Storage images (image(), gemm_probes.same / describe) are
larger than the problem and NaN outside it, and are compared whole.

Row tiles of the conv GEMMs come from gemm_probes' mirror of the dispatcher (conv_gemm_specs), so the shape
classes the host test asserts are computed from the shapes, not listed by hand.
"""
import dataclasses
import functools

import torch
import torch.nn.functional as F

import gemm_probes as P

NAN = P.NAN
GUARD = 8            # surplus rows / elements behind every output, NaN before the launch
EBADARG = -10000     # MMT_EBADARG (include/mmt_hip.h)
U32 = 2.0 ** -24     # fp32 unit roundoff (half an ulp, relative)


def _gen(*key):
    h = 0
    for k in key:
        h = (h * 1000003 + int(k) + 12345) & 0x7FFFFFFF
    return torch.Generator().manual_seed(h)


def _nonzero(shape, lo, hi, g):
    """Integers of magnitude lo..hi with a random sign (never 0)."""
    return torch.randint(lo, hi + 1, shape, generator=g) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)


def image(rows, width, body, dtype, guard=GUARD):
    """[rows + guard][width] storage: `body` ([rows][width]) then NaN rows."""
    t = torch.full((rows + guard, width), NAN, dtype=dtype)
    t[:rows] = body.reshape(rows, width).to(dtype)
    return t


def poison(rows, width, dtype, guard=GUARD):
    return torch.full((rows + guard, width), NAN, dtype=dtype)


def bf16_exact(t):
    """Every value of the fp64 tensor is an integer of magnitude <= 256: bf16 holds it exactly."""
    return bool((t == t.round()).all()) and float(t.abs().max()) <= 256.0


def f32_exact(t):
    return bool((t == t.round()).all()) and float(t.abs().max()) < 2.0 ** 24


def bf16_bar(ref, delta):
    """|got - ref| allowed for a bf16 result whose fp32 value before the cast lies within `delta` of the fp64
    `ref`: round-to-nearest moves a value v by at most 2^-8 |v| (half an ulp of 8 significant bits), here of
    v = ref +- delta, plus delta itself."""
    return 2.0 ** -8 * (ref.abs() + delta) + delta


# ------------------------------------------------------------------------------------------------ 1. conv3x3
@dataclasses.dataclass(frozen=True)
class ConvCase:
    B: int
    Hi: int
    up: int
    Cin: int
    Cout: int
    keep_pad: bool = False

    @property
    def Ho(self):
        return self.Hi * self.up

    @property
    def Cp(self):
        return (self.Cout + 7) // 8 * 8

    @property
    def M(self):
        return self.B * self.Ho * self.Ho


CONV_CASES = (
    ConvCase(2, 1, 1, 8, 1),              # one pixel an image, M = 2 (dW through the padded transposes: M % 8 != 0)
    ConvCase(3, 1, 2, 24, 8),             # Ho = up = 2
    ConvCase(2, 1, 4, 48, 12),            # Ho = up = 4, Cout 12 in 16-channel rows, sliced
    ConvCase(1, 8, 1, 96, 48),            # M = 64: one row tile exactly
    ConvCase(2, 6, 1, 64, 1, True),       # K = 576 = 9 K-steps, no tail; image boundary at row 36 of a tile; keep_pad
    ConvCase(2, 3, 2, 8, 1, True),        # up 2, keep_pad
    ConvCase(3, 2, 4, 24, 48),            # up 4, M = 192
    ConvCase(1, 12, 1, 48, 8),            # M = 144: just above a tile multiple
    ConvCase(3, 5, 2, 96, 12),            # M = 300; 3600 im2col chunks, 900 block-sum chunks (ragged last workgroups)
    ConvCase(2, 5, 4, 8, 1),              # up 4, Cout 1 sliced, M = 800
    ConvCase(1, 3, 4, 48, 48),            # up 4, M = 144
    ConvCase(5, 4, 1, 24, 12, True),      # M = 80; keep_pad with four padding channels
)


def conv_gemm_specs(c):
    """The forward and dX launches of _HipConv3x3 as gemm_probes specs (one group, auto impl, no split)."""
    fwd = P.Spec(c.M, c.Cp, 9 * c.Cin, impl=0, groups=1, conv=(c.Ho, c.up, c.Cin, 1, 0))
    dx = P.Spec(c.M, c.Cin, 9 * c.Cp, impl=0, groups=1, bias=False, conv=(c.Ho, 1, c.Cp, 2, 0))
    return fwd, dx


def row_tile(spec):
    k = P.kernel_of(spec)
    return P.TILES[k[1]][0] if k[0] == "glds" else k[1]


def conv_classes(c):
    """Edge classes of a case, each computed from its shape."""
    out = {"up%d" % c.up, "cin%d" % c.Cin}
    out.add("cout1" if c.Cout == 1 else "cout8" if c.Cout == 8 else "cout48" if c.Cout == 48 else
            "cout_ragged" if c.Cout > 8 and c.Cout % 8 else "cout_other")
    if c.Cout == 1:
        out.add("cout1_keep_pad" if c.keep_pad else "cout1_sliced")
    out.add("k_tail" if (9 * c.Cin) % 64 else "k_no_tail")
    for s in conv_gemm_specs(c):
        bm = row_tile(s)
        r = c.M % bm
        out.add("m_at" if r == 0 else "m_above" if (c.M > bm and r <= bm // 2) else "m_below")
        if c.B >= 2 and (c.Ho * c.Ho) % bm:
            out.add("image_boundary_in_tile")
    if c.Hi == 1 and c.up > 1:
        out.add("one_pixel_lowres")
    if c.up > 1:
        n = c.B * c.Hi * c.Hi * c.Cin // 8
        out.add("upsum_ragged" if n % 256 else "upsum_full")
        if n > 256:
            out.add("upsum_multi_block")
    n = c.M * c.Cin // 8
    out.add("im2col_ragged" if n % 256 else "im2col_full")
    if n > 256:
        out.add("im2col_multi_block")
    if c.M % 8:
        out.add("m_not_multiple_of_8")
    return out


CONV_REQUIRED = {"up1", "up2", "up4", "cin8", "cin24", "cin48", "cin96", "cout1", "cout8", "cout_ragged", "cout48",
                 "cout1_keep_pad", "cout1_sliced", "k_tail", "k_no_tail", "m_at", "m_above", "m_below",
                 "image_boundary_in_tile", "one_pixel_lowres", "upsum_ragged", "upsum_multi_block", "im2col_ragged",
                 "im2col_multi_block", "m_not_multiple_of_8"}


def _one_hot(B, H, C, amax, g, signed=False):
    """[B][H][H][C] with one non-zero channel per pixel, amplitude 1..amax (signed: of either sign)."""
    ch = torch.randint(0, C, (B, H, H), generator=g)
    amp = _nonzero((B, H, H), 1, amax, g) if signed else torch.randint(1, amax + 1, (B, H, H), generator=g)
    return torch.zeros(B, H, H, C, dtype=torch.int64).scatter_(3, ch[..., None], amp[..., None])


def up_nchw(x_nhwc, up):
    """Nearest upsampling of an NHWC map, returned NCHW float64."""
    return x_nhwc.double().permute(0, 3, 1, 2).repeat_interleave(up, 2).repeat_interleave(up, 3)


def conv_autograd(x, w, b, dy, up):
    """float64 F.conv2d of the nearest-upsampled x and its autograd: (y, dx, dw, db), NHWC maps."""
    xr = x.double().requires_grad_(True)
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    y = F.conv2d(up_nchw(xr, up), wr, br, padding=1).permute(0, 2, 3, 1)
    y.backward(dy.double())
    return y.detach(), xr.grad, wr.grad, br.grad


@functools.lru_cache(maxsize=None)
def conv_problem(c):
    """Integer operands of a case and the expected outputs (float64; computed once, shared, never modified):
    x one-hot per pixel with amplitude 1..3, dy one-hot among the Cout valid channels with amplitude +-1 / +-2
    (either sign: the up x up block sums of dX then stay far below 256 with a single output channel too), w in
    {-2, -1, 1, 2}, bias in [-8, 8].  y, dy_pad and the expectations are in the padded Cp-channel rows; pad_fill
    is a finite non-zero filling for dY's padding channels (the keep_pad probe)."""
    g = _gen(c.B, c.Hi, c.up, c.Cin, c.Cout)
    x = _one_hot(c.B, c.Hi, c.Cin, 3, g)
    dy = _one_hot(c.B, c.Ho, c.Cout, 2, g, signed=True)
    w = _nonzero((c.Cout, c.Cin, 3, 3), 1, 2, g)
    b = torch.randint(-8, 9, (c.Cout,), generator=g)
    y, dx, dw, db = conv_autograd(x, w, b, dy, c.up)
    y_pad = torch.zeros(c.B, c.Ho, c.Ho, c.Cp, dtype=torch.float64)
    y_pad[..., :c.Cout] = y
    dy_pad = torch.zeros(c.B, c.Ho, c.Ho, c.Cp, dtype=torch.int64)
    dy_pad[..., :c.Cout] = dy
    pad_fill = _nonzero((c.B, c.Ho, c.Ho, c.Cp - c.Cout), 1, 3, g)
    return dict(x=x, dy=dy, dy_pad=dy_pad, w=w, b=b, y=y, y_pad=y_pad, dx=dx, dw=dw, db=db, pad_fill=pad_fill)


def conv_layouts(c, w):
    """The two operand layouts mmt_conv3x3_wprep makes: wf [Cp][(ky, kx, ci)] and wb [Cin][(ky, kx, co)], int64."""
    wp = torch.zeros(c.Cp, c.Cin, 3, 3, dtype=torch.int64)
    wp[:c.Cout] = w
    return wp.permute(0, 2, 3, 1).reshape(c.Cp, 9 * c.Cin), wp.permute(1, 2, 3, 0).reshape(c.Cin, 9 * c.Cp)


def block_sum(t_nhwc, up):
    """[B][H*up][W*up][C] -> [B][H][W][C]: the up x up block sums (the backward of nearest upsampling)."""
    B, H, W, C = t_nhwc.shape
    return t_nhwc.reshape(B, H // up, up, W // up, up, C).sum((2, 4))


# direct C-ABI probes: (B, Hi, Wi, C, up) with Hi != Wi (a swapped H / W shows), chunk counts below one workgroup,
# a multiple of 256 and ragged above it
UPSUM_CASES = ((1, 1, 1, 8, 2), (2, 3, 5, 8, 4), (2, 8, 16, 8, 2), (3, 7, 5, 24, 4), (1, 16, 16, 16, 1))
IM2COL_CASES = ((1, 1, 1, 8, 1), (1, 2, 4, 8, 2), (2, 8, 16, 8, 1), (2, 12, 8, 24, 4), (3, 5, 7, 16, 1), (1, 4, 12, 48, 4))


def upsum_problem(case):
    B, Hi, Wi, C, up = case
    src = _nonzero((B, Hi * up, Wi * up, C), 1, 256 // (up * up) if up > 1 else 256, _gen(*case))
    return src, block_sum(src, up)


def im2col_problem(case):
    """`case` = (B, H, W, C, up) at the upsampled size; -> (low-resolution source, channel-major columns
    [pix][c * 9 + tap], tap-major columns [pix][tap * C + c]), integers of magnitude 1..256."""
    B, H, W, C, up = case
    src = _nonzero((B, H // up, W // up, C), 1, 256, _gen(*case, 9))
    cols = F.unfold(up_nchw(src, up), 3, padding=1)              # [B][C * 9][H * W]: torch's (c, ky, kx) order
    cm = cols.permute(0, 2, 1).reshape(B * H * W, C * 9)
    tm = cm.view(-1, C, 9).permute(0, 2, 1).reshape(B * H * W, 9 * C)
    return src, cm, tm


# ------------------------------------------------------------------------------------------------ 2. add_up
ADDUP_CASES = ((1, 2, 2, 8, 2), (2, 12, 20, 8, 4), (3, 10, 6, 24, 2), (2, 16, 16, 8, 1))  # (B, H, W, C, up), b's size


def addup_problem(case):
    """a [B][H/up][W/up][C], b and dout [B][H][W][C]: |a|, |b| <= 100 (the sum exact in bf16), |dout| <= 256 / up^2."""
    B, H, W, C, up = case
    g = _gen(*case, 2)
    a = _nonzero((B, H // up, W // up, C), 1, 100, g)
    b = _nonzero((B, H, W, C), 1, 100, g)
    dout = _nonzero((B, H, W, C), 1, 256 // (up * up), g)
    out = a.repeat_interleave(up, 1).repeat_interleave(up, 2) + b
    return a, b, dout, out, block_sum(dout, up)


# ------------------------------------------------------------------------------------------------ 3. batch norm
BN_THREADS, BN_FLANES = 256, 8
BN_CP = ((1, 8), (8, 8), (50, 56), (48, 48), (24, 24), (1032, 1032), (2048, 2048))
BN_MS = (1, 31, 32, 33, 1920, 2048, 3191, 8191, 8192, 8193, 8449)
BN_MS_WIDE = (1, 33, 34, 2048)  # the 1032- and 2048-channel rows (R = 1: every row of a workgroup on one lane)
BN_EPS, BN_MOM = 3.0, 0.25
# save[0] = (float)(pivot + s / M): exact integer sums s, q (pivoted), two double operations (relative 2^-53
# each, on |pivot| <= 256: below 2^-44 absolute) and one cast to fp32 (half an ulp): 1 ulp = 2 U32 |mean| allowed.
BN_MEAN_ULPS = 1
# save[1] = 1.f / sqrtf((float)vb + eps): cast (<= U32), add (<= U32; together they reach the root halved: <= U32),
# sqrtf and the divide (<= 2 U32 each if the device functions are 1-ulp rather than correctly rounded) = 5 U32,
# plus the double finalize (q / M - ms^2 cancels at most 256^2 / 1: < 2^-36 relative): 3 ulp = 6 U32 allowed.
BN_INV_ULPS = 3


def bn_blocks(M):
    return min((M + 31) // 32, 256)


def bn_lane_path(nblk):
    """What bn_lane_sums' lanes do with nblk partials: the set of (unrolled passes > 0, tail iterations > 0)."""
    out = set()
    for lane in range(BN_FLANES):
        k, passes = lane, 0
        while k + 7 * BN_FLANES < nblk:
            k += 8 * BN_FLANES
            passes += 1
        out.add((passes, len(range(k, nblk, BN_FLANES))))
    return out


@dataclasses.dataclass(frozen=True)
class BNCase:
    M: int
    C: int
    pitch: int
    kind: str = "balanced"   # balanced: m_c +- 1 in equal counts (even M); odd: the same with one more row;
    training: int = 1        # general: m_c + k, k in {+-1, +-2, +-3}; offset: balanced with |m_c| up to 254
    relu: int = 1


def bn_cases(C, pitch):
    wide = pitch > 256
    out = []
    for M in (BN_MS_WIDE if wide else BN_MS):
        out.append(BNCase(M, C, pitch, "balanced" if M % 2 == 0 else "odd"))
    if not wide:
        out += [BNCase(8192, C, pitch, "offset"), BNCase(8449, C, pitch, "general"), BNCase(3191, C, pitch, "general", relu=0),
                BNCase(2048, C, pitch, "balanced", relu=0), BNCase(33, C, pitch, "general", training=0),
                BNCase(8193, C, pitch, "general", training=0, relu=0)]
    else:
        out += [BNCase(34, C, pitch, "offset"), BNCase(33, C, pitch, "general", training=0)]
    return out


def bn_exact(c):
    """Every output of the case is known bit for bit (dx excepted, which divides by M)."""
    return c.training == 0 or c.kind in ("balanced", "offset")


@functools.lru_cache(maxsize=4)
def bn_problem(c):
    """Operands and float64 references of a case.  gamma in {+-2, +-4}; beta integers in [-3, 3] (exact cases:
    pre-activations +-gamma / 2 + beta are integers, some exactly 0) or integers +- 3/8 (the others: no
    pre-activation within 1e-3 of the ReLU's threshold -- `margin`); dY in {+-1, +-2}; running mean / variance
    start as multiples of 4 (eval: variance 1, so that invstd = 1 / sqrt(1 + 3) = 0.5)."""
    g = _gen(c.M, c.C, c.pitch, len(c.kind), c.training, c.relu)
    M, C, pitch = c.M, c.C, c.pitch
    exact = bn_exact(c)
    mc = _nonzero((C,), 2, 254 if c.kind == "offset" else 2, g)      # |m_c| >= 2: m_c +- 1 is never 0
    if c.kind in ("balanced", "offset", "odd"):
        half = (M + 1) // 2
        sign = torch.cat([torch.ones(half), -torch.ones(M - half)]).to(torch.int64)
        k = torch.stack([sign[torch.randperm(M, generator=g)] for _ in range(min(C, 64))], 1)
        k = k[:, torch.arange(C) % k.shape[1]]
        k = k * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)      # which side has the extra row / the pivot
    else:
        k = _nonzero((M, C), 1, 3, g)
        if c.training:
            mc = mc.clamp(-2, 2)
    x = torch.zeros(M, pitch, dtype=torch.int64)
    x[:, :C] = mc[None] + k
    x[:, C:] = _nonzero((M, pitch - C), 1, 9, g)                      # padding channels: finite, non-zero
    dy = _nonzero((M, pitch), 1, 2, g)
    gamma = _nonzero((C,), 1, 2, g) * 2
    beta = torch.randint(-3, 4, (C,), generator=g).double()
    if not exact:
        beta = beta + 0.375 * (torch.randint(0, 2, (C,), generator=g) * 2 - 1).double()
    rm0 = torch.randint(-2, 3, (C,), generator=g) * 4
    rv0 = torch.full((C,), 4, dtype=torch.int64) if c.training else torch.ones(C, dtype=torch.int64)
    xd, dyd = x[:, :C].double(), dy[:, :C].double()
    if c.training:
        mean = xd.mean(0)
        var = ((xd - mean) ** 2).mean(0)
    else:
        mean, var = rm0.double(), rv0.double()
    inv = 1.0 / torch.sqrt(var + BN_EPS)
    sc = gamma.double() * inv
    pre = (xd - mean) * sc + beta
    mask = (pre > 0) if c.relu else torch.ones_like(pre, dtype=torch.bool)
    y = torch.zeros(M, pitch, dtype=torch.float64)
    y[:, :C] = pre.clamp(min=0) if c.relu else pre
    gg = dyd * mask
    xhat = (xd - mean) * inv
    dbeta, dgamma = gg.sum(0), (gg * xhat).sum(0)
    dx = torch.zeros(M, pitch, dtype=torch.float64)
    R = BN_THREADS // (pitch // 8)
    rows_blk = -(-M // bn_blocks(M)) + 1
    # dgamma where the statistics are not exact: every term g * xhat carries xhat's error (the mean's 2 U32 |mean|
    # times invstd, invstd's 6 U32, a subtract and two products: 10 U32 |xhat|), and the fp32 sums run over a
    # lane's rows of the workgroup, then its R lanes in order: (rows / R + R + 10) U32 of the terms' magnitudes
    dgamma_bar = (rows_blk // R + R + 10) * U32 * (gg.abs() * (xhat.abs() + 2 * inv * mean.abs())).sum(0)
    if c.training:
        dx[:, :C] = sc * (gg - dbeta / M - xhat * dgamma / M)
        # fp32 value before the cast: gamma * invstd (7 U32), the two casts of the means, xhat (10 U32 and the mean's
        # 2 U32 |mean| invstd), two products, two subtracts, the last product: 16 U32 of the terms' magnitudes, plus
        # dgamma's own bar where the statistics are not exact
        dx_delta = U32 * sc.abs() * (16 * (gg.abs() + (dbeta / M).abs() + xhat.abs() * (dgamma / M).abs())
                                     + 2 * inv * mean.abs() * (dgamma / M).abs())
        if not exact:
            dx_delta = dx_delta + sc.abs() * xhat.abs() * dgamma_bar / M
        vu = var * M / (M - 1) if M > 1 else var
        rm1 = ((1 - BN_MOM) * rm0.float() + BN_MOM * mean.float())
        rv1 = ((1 - BN_MOM) * rv0.float() + BN_MOM * vu.float())
    else:
        dx[:, :C] = sc * gg
        dx_delta = torch.zeros(M, C, dtype=torch.float64)
        rm1, rv1 = rm0.float(), rv0.float()
    delta = torch.zeros(M, pitch, dtype=torch.float64)
    delta[:, :C] = dx_delta
    # y where the statistics are not exact: x * scale + shift in fp32, scale = gamma * invstd within 7 U32, shift =
    # beta - mean * scale within 10 U32 |mean scale| + U32 |shift|, a product and an add: 12 U32 of the magnitudes
    y_delta = torch.zeros(M, pitch, dtype=torch.float64)
    y_delta[:, :C] = 12 * U32 * (xd.abs() * sc.abs() + (mean * sc).abs() + beta.abs())
    return dict(x=x, dy=dy, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, mean=mean, var=var, inv=inv, sc=sc, sh=beta - mean * sc,
                y=y, mask=mask, dbeta=dbeta, dgamma=dgamma, dx=dx, dx_delta=delta, y_delta=y_delta, rm1=rm1, rv1=rv1,
                margin=float(pre.abs().min()) if c.relu else float("inf"), dgamma_bar=dgamma_bar, exact=exact)


def bn_mean_bar(mean):
    return BN_MEAN_ULPS * 2 * U32 * mean.abs() + 2.0 ** -40


def bn_inv_bar(inv):
    return BN_INV_ULPS * 2 * U32 * inv.abs()


def bn_running_bars(pr):
    """Running statistics where the batch moments are not exact: 0.75 * old (exact) + 0.25 * mean (the mean's bar,
    scaled exactly) and one add; the variance one cast of the double M / (M - 1) * var and one add."""
    return 2 * U32 * (pr["rm1"].double().abs() + pr["mean"].abs()), 4 * U32 * pr["rv1"].double().abs()


# ------------------------------------------------------------------------------------------------ 4. corner score
@dataclasses.dataclass(frozen=True)
class ScoreCase:
    B: int
    fh: int
    c4: int
    p3: int   # da3 / a3 row pitch (1 or 8)
    p4: int

    @property
    def bands(self):
        return self.B * self.fh // 4


SCORE_CASES = (ScoreCase(3, 4, 8, 1, 1), ScoreCase(16, 4, 48, 8, 8), ScoreCase(17, 4, 56, 8, 1), ScoreCase(33, 4, 8, 1, 8),
               ScoreCase(1, 12, 48, 8, 8), ScoreCase(11, 12, 56, 1, 1), ScoreCase(1, 128, 48, 8, 8), ScoreCase(2, 128, 8, 1, 1))
SCORE_REJECTED = (dict(c4=64), dict(fh=132), dict(fh=6))  # documented: c4 < 64, fh <= 128, fh % 4 == 0


@functools.lru_cache(maxsize=None)
def score_problem(c):
    """x4 one-hot (amplitude 1..4), w5 in +-[1, 8], b5, a3 / a4 in +-[1, 9]; dsm odd values in +-[1, 7] except the
    first pixel of every 4-row band, which is even: a band's dsm sum is odd, so no band partial of db5 is 0."""
    g = _gen(c.B, c.fh, c.c4, c.p3, c.p4)
    B, fh, c4 = c.B, c.fh, c.c4
    x4 = _one_hot(B, fh, c4, 4, g)
    w5, b5 = _nonzero((c4,), 1, 8, g), _nonzero((1,), 1, 8, g)
    a3, a4 = _nonzero((B, fh // 4, fh // 4), 1, 9, g), _nonzero((B, fh // 2, fh // 2), 1, 9, g)
    dsm = (torch.randint(0, 4, (B, fh, fh), generator=g) * 2 + 1) * (torch.randint(0, 2, (B, fh, fh), generator=g) * 2 - 1)
    dsm[:, ::4, 0] = _nonzero((B, fh // 4), 1, 4, g) * 2
    up = lambda t, f: t.repeat_interleave(f, 1).repeat_interleave(f, 2)  # noqa: E731
    sm = (x4 * w5).sum(-1) + b5 + up(a3, 4) + up(a4, 2)
    dx4 = dsm[..., None] * w5
    da3 = dsm.reshape(B, fh // 4, 4, fh // 4, 4).sum((2, 4))
    da4 = dsm.reshape(B, fh // 2, 2, fh // 2, 2).sum((2, 4))
    band = (dsm[..., None] * x4).reshape(c.bands, 4 * fh, c4).sum(1)      # [bands][c4]: the dw5 partials
    band_b = dsm.reshape(c.bands, 4 * fh).sum(1)                          # [bands]: the db5 partials
    return dict(x4=x4, w5=w5, b5=b5, a3=a3, a4=a4, dsm=dsm, sm=sm, dx4=dx4, da3=da3, da4=da4, dw5=band.sum(0),
                db5=band_b.sum(0, keepdim=True), band=band, band_b=band_b)


def padded_rows(t, pitch, fill):
    """[n] values -> [n][pitch] rows with the value in channel 0 and `fill` in the others."""
    out = torch.full((t.numel(), pitch), fill, dtype=torch.float64)
    out[:, 0] = t.reshape(-1).double()
    return out


# ------------------------------------------------------------------------------------------------ 5. corner boxes
CB_T = 256
BOX_CASES = ((7, 2.0), (16, 16.0), (17, 4.0), (80, 4.0))  # (fh, stride): n = 49, 256, 289, 6400
PEAK_LOGIT = 120.0  # expf(-120) is 0 in fp32 (below the smallest denormal): every weight but the peak's vanishes


def peak_pixels(fh):
    n = fh * fh
    return sorted({0, fh - 1, n - fh, n - 1} | {k for k in (255, 256) if k < n})


def peak_problem(fh, stride):
    """One map of the batch per peak pixel, tl at p[i] and br at p[i + 1]: xyxy and stats exactly."""
    ps = peak_pixels(fh)
    B, n, img = len(ps), fh * fh, fh * stride
    pt, pb = torch.tensor(ps), torch.tensor(ps[1:] + ps[:1])
    tl, br = torch.zeros(B, n), torch.zeros(B, n)
    tl[torch.arange(B), pt] = PEAK_LOGIT
    br[torch.arange(B), pb] = PEAK_LOGIT
    e = torch.stack([stride * (pt % fh), stride * (pt // fh), stride * (pb % fh), stride * (pb // fh)], 1).float()
    inv_img = (torch.ones((), dtype=torch.float32) / torch.tensor(img, dtype=torch.float32))
    stats = torch.stack([torch.stack([torch.full((B,), PEAK_LOGIT), torch.ones(B), e[:, 2 * c], e[:, 2 * c + 1]], 1)
                         for c in range(2)], 1)
    return dict(tl=tl, br=br, pt=pt, pb=pb, e=e, xyxy=e * inv_img, stats=stats, img=float(img))


def boxes_const_bar(fh):
    """Relative bar of the uniform map's expectation: p = 1 / n (one divide), each term stride * col * p (the
    product with p rounds; stride * col is exact), a thread's ceil(n / 256) sequential adds, log2(256) = 8 levels of
    the block sum, the scaling by 1 / img and its own rounding: (ceil(n / 256) + 8 + 4) U32."""
    return (-(-fh * fh // CB_T) + 8 + 4) * U32


def const_problem(fh, stride, B=2):
    n, img = fh * fh, fh * stride
    g = _gen(fh, 77)
    tl, br = torch.full((B, n), 3.0), torch.full((B, n), -7.0)
    dxy = _nonzero((B, 4), 1, 4, g).float()
    ex = stride * (fh - 1) / 2.0
    xyxy = torch.full((B, 4), ex / img, dtype=torch.float64)
    k = torch.arange(n)
    xs, ys = (stride * (k % fh)).double(), (stride * (k // fh)).double()
    gr = dxy.double() / img
    d, dbar = [], []
    for c in range(2):
        gx, gy = gr[:, 2 * c, None], gr[:, 2 * c + 1, None]
        d.append((gx * (xs - ex) + gy * (ys - ex)) / n)
        # p, the two differences (ex, ey carry the expectation's bar), two products, one add, the product with p
        dbar.append((boxes_const_bar(fh) + 8 * U32) * (gx.abs() * (xs + ex) + gy.abs() * (ys + ex)) / n)
    return dict(tl=tl, br=br, dxy=dxy, xyxy=xyxy, d=d, dbar=dbar, img=float(img))
