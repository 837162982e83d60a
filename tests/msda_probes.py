"""Probe inputs and fp64 references of the bimodal deformable attention (no tests here): mmt_msda_bimodal (inference),
mmt_msda_bimodal_train_fwd / _bwd (training) and, on the same problems, the generic mmt_ms_deform_attn_forward /
_backward_impl.

One problem description (value [B][2][nq][8][64], off [B][nq][8][2][4][2] in pixels, logits [B][nq][8][8], output
gradient [B][nq][512], reference points [nq][2] as (x, y), all float64 holding values the 16-bit types store exactly)
yields the training layouts (train_inputs), the inference layouts (infer_inputs) and the generic op's (generic_inputs).

Exact families (hw a power of two, cell-centre reference points, offsets multiples of 1/4 pixel): w_im = qx + ox and
h_im = qy + oy hold exactly in fp32 with or without FMA contraction; logits in {0, -200} make the softmax weights
exactly 0, 1/8, 1/4, 1/2 or 1; values and output gradients are small integers.  Every term of every fp32 sum is then
an integer multiple of a common quantum and the sums stay below 2^24 quanta, so each fp32 partial sum is exact in any
order and each output is the fp64 reference rounded once (expected()).
  gather   one-hot weights, integer-pixel offsets, values an integer code of (level, pixel, head, channel): a wrong
           index yields another integer.  The hot samples' positions are constructed to visit every pair of the axis
           classes integer offsets reach (< -1, == -1, a pixel, == hw, > hw).
  blend    weights 1/8 x 8, 1/2 x 2 and 1/4 x 4 in rotation, offsets multiples of 1/4 pixel, every pair of the eight
           axis classes among the samples of non-zero weight.
  buckets  the backward value gather's lists: every sample of a level on one pixel, on one half-pixel position, on its
           own query's pixel, and a pattern that leaves pixels with exactly BUCKET_LONG and BUCKET_LONG + 1 entries.

Bar families (hw 5, 20, 22; random bf16 logits and offsets, and a `collapse` variant that puts every sample of a
level near one point): no coordinate within 1/16 pixel of an integer of [-1, hw], so the in-range test and floor()
decide the same in fp32 and fp64 and no sample is excluded from any comparison.  The bar comes from the oracle's own
fp32 error (delta()), never from the kernel.

References: oracle.msda in float64 on loc = ref + off / hw.  Storage images (head_probes.image, gemm_probes.same /
describe) are GUARD rows larger than the problem, NaN outside it, and compared whole.
"""
import functools

import torch

import gemm_probes as P
import head_probes as H
from oracle.msda import ms_deform_attn, ms_deform_attn_backward

NAN = P.NAN
GUARD = H.GUARD
EBADARG = H.EBADARG          # MMT_EBADARG (include/mmt_hip.h)
NH, NL, NP, DH = 8, 2, 4, 64
CM = NH * DH
NQ_MAX = 484                 # MT_NQ_MAX (msda.hip): the training kernels' LDS lists hold 22 x 22 queries
BUCKET_LONG = 24             # buckets longer than this take bucket_sum<8>
VT = 1024                    # MT_VT: threads of the training value gather (16 waves share the items)
WIDE, WIDE_AWL = 208, 136    # the one-row form: offsets at column 0, logits at column 136 (272 B: 16-byte aligned)
F64, F32, BF16, F16 = torch.float64, torch.float32, torch.bfloat16, torch.float16

EXACT_SIZES = ((4, 1), (4, 3), (8, 1), (8, 3), (16, 1))          # (hw, B)
BUCKET_PATTERNS = ("pixel", "half", "zero", "long")
BAR_SIZES = ((5, 1), (5, 2), (20, 1), (20, 2), (22, 1), (22, 2))
BAR_VARIANTS = ("randn", "collapse")
MARGIN = 1.0 / 16

EXACT_KEYS = tuple([("gather", hw, B, "") for hw, B in EXACT_SIZES] + [("blend", hw, B, "") for hw, B in EXACT_SIZES] +
                   [("buckets", hw, B, p) for hw, B in EXACT_SIZES for p in BUCKET_PATTERNS])
BAR_KEYS = tuple(("bar", hw, B, v) for hw, B in BAR_SIZES for v in BAR_VARIANTS)
OUTPUTS = ("out", "gv", "goff", "gawl")


def key_id(k):
    return "%s-hw%d-B%d%s" % (k[0], k[1], k[2], "-" + k[3] if k[3] else "")


# ------------------------------------------------------------------------------------------------ geometry
def ref_points(hw):
    """Cell centres (x, y) in fp32, one correctly rounded division each: what mmt_msda_bimodal computes itself."""
    q = torch.arange(hw * hw)
    n = torch.tensor(float(hw), dtype=F32)
    return torch.stack([((q % hw).float() + 0.5) / n, ((q // hw).float() + 0.5) / n], 1)


def coords(pr):
    """(w_im, h_im) of every sample in float64 from the inputs: [B][nq][8][2][4] each."""
    loc = pr["ref"].double().view(1, pr["nq"], 1, 1, 1, 2) + pr["off"] / pr["hw"]
    c = loc * pr["hw"] - 0.5
    return c[..., 0], c[..., 1]


def axis_class(c, hw):
    """0: < -1, 1: == -1, 2: (-1, 0), 3: a pixel of [0, hw - 1], 4: fractional inside, 5: (hw - 1, hw), 6: == hw,
    7: > hw."""
    integer = c == c.floor()
    out = torch.full(c.shape, 4, dtype=torch.int64)
    out[integer & (c >= 0) & (c <= hw - 1)] = 3
    out[(c > -1) & (c < 0)] = 2
    out[(c > hw - 1) & (c < hw)] = 5
    out[c == -1] = 1
    out[c == hw] = 6
    out[c < -1] = 0
    out[c > hw] = 7
    return out


INT_CLASSES = (0, 1, 3, 6, 7)


def class_coord(cls, k, hw, quarter):
    """A coordinate of axis class `cls` (int64 tensor), varied by the integers `k` (>= 0); quarter: multiples of 1/4
    pixel, else integers (classes 2, 4, 5 do not exist then)."""
    k = k.to(torch.int64)
    f = ((k % 3) + 1).double() / 4
    far = (1 + k % 8).double() / 4 if quarter else (1 + k % 2).double()
    c = torch.zeros(cls.shape, dtype=F64)
    c = torch.where(cls == 0, -1 - far, c)
    c = torch.where(cls == 1, torch.full_like(c, -1.0), c)
    c = torch.where(cls == 2, -f, c)
    c = torch.where(cls == 3, (k % hw).double(), c)
    c = torch.where(cls == 4, (k % (hw - 1)).double() + f, c)
    c = torch.where(cls == 5, hw - 1 + f, c)
    c = torch.where(cls == 6, torch.full_like(c, float(hw)), c)
    c = torch.where(cls == 7, hw + far, c)
    return c


def _grid(B, nq):
    """Index tensors b, q, m, i (i = level * 4 + point) broadcasting to [B][nq][8][8]."""
    return (torch.arange(B).view(B, 1, 1, 1), torch.arange(nq).view(1, nq, 1, 1), torch.arange(NH).view(1, 1, NH, 1),
            torch.arange(NL * NP).view(1, 1, 1, NL * NP))


def _offsets(tx, ty, hw):
    """Targets (w_im, h_im) [B][nq][8][8] -> off [B][nq][8][2][4][2]: target minus the query's own pixel."""
    B, nq = tx.shape[:2]
    q = torch.arange(nq).view(1, nq, 1, 1)
    off = torch.stack([tx - (q % hw).double(), ty - (q // hw).double()], -1)
    return off.reshape(B, nq, NH, NL, NP, 2)


def _values(B, hw, amax):
    """An integer code of (batch, level, pixel, head, channel) in [-amax, amax]: multipliers coprime to the modulus,
    so an index that is off in one place reads another integer."""
    nq, mod = hw * hw, 2 * amax + 1
    b = torch.arange(B).view(B, 1, 1, 1, 1)
    l = torch.arange(NL).view(1, NL, 1, 1, 1)
    p = torch.arange(nq).view(1, 1, nq, 1, 1)
    m = torch.arange(NH).view(1, 1, 1, NH, 1)
    c = torch.arange(DH).view(1, 1, 1, 1, DH)
    return ((13 * b + 97 * l + 31 * p + 7 * m + 3 * c) % mod - amax).double()


def _gout(B, hw, amax):
    """Output gradients: non-zero integers of [-amax, amax] that depend on (batch, query, channel)."""
    nq = hw * hw
    b = torch.arange(B).view(B, 1, 1)
    q = torch.arange(nq).view(1, nq, 1)
    c = torch.arange(CM).view(1, 1, CM)
    k = (2 * b + 5 * q + 3 * c + c // DH) % (2 * amax)
    return torch.where(k < amax, k - amax, k - amax + 1).double()


def _blend_logits(B, nq):
    """0 / -200 patterns in rotation: eight zeros (weights 1/8), two (1/2), four (1/4)."""
    b, q, m, i = _grid(B, nq)
    kind = (b + q + m) % 3
    rot = (i + q + 3 * m) % 8
    hot = torch.where(kind == 0, torch.ones_like(rot, dtype=torch.bool),
                      torch.where(kind == 1, (rot == 0) | (rot == 5), rot % 2 == 0))
    return torch.where(hot, 0.0, -200.0).double().expand(B, nq, NH, NL * NP).contiguous()


# ------------------------------------------------------------------------------------------------ exact families
_INT_TABLE = torch.tensor([3, 0, 3, 1, 3, 6, 3, 7])
_Q_TABLE = torch.tensor([3, 4, 0, 4, 1, 4, 2, 3, 5, 4, 6, 4, 7])


def _gather(hw, B):
    nq = hw * hw
    b, q, m, i = _grid(B, nq)
    r = b * nq + q
    hot = (i == (b + q + m) % 8).expand(B, nq, NH, NL * NP)
    logits = torch.where(hot, 0.0, -200.0).double()
    cx = _INT_TABLE[(m + r) % 8]
    cy = _INT_TABLE[(r + 3 * m + r // 8) % 8]
    hx = class_coord(cx, r + 5 * m, hw, False).expand(B, nq, NH, NL * NP)
    hy = class_coord(cy, 3 * r + m + r // hw, hw, False).expand(B, nq, NH, NL * NP)
    g = H._gen(hw, B, 1)  # the samples of weight 0: drawn, anywhere from two pixels before the map to two behind it
    dx = torch.randint(-2, hw + 2, hot.shape, generator=g).double()
    dy = torch.randint(-2, hw + 2, hot.shape, generator=g).double()
    off = _offsets(torch.where(hot, hx, dx), torch.where(hot, hy, dy), hw)
    return dict(value=_values(B, hw, 125), off=off, logits=logits, g=_gout(B, hw, 3), q_off=1.0, q_a=1.0)


def _blend(hw, B):
    nq = hw * hw
    b, q, m, i = _grid(B, nq)
    s = ((b * nq + q) * NH + m) * (NL * NP) + i
    tx = class_coord(_Q_TABLE[s % 13], s // 7 + s, hw, True)
    ty = class_coord(_Q_TABLE[(s // 13) % 13], s // 11 + 2 * s, hw, True)
    return dict(value=_values(B, hw, 4), off=_offsets(tx, ty, hw), logits=_blend_logits(B, nq), g=_gout(B, hw, 3),
                q_off=0.25, q_a=0.125)


LONG_RUNS = (BUCKET_LONG, 1, BUCKET_LONG - 1, 2)  # samples on the last four positions of the last row (level 1: column)


def _buckets(hw, B, pattern):
    """The value gather's lists.  A bucket takes every in-map tap of every in-range sample, whatever its weight.
    long: per (batch, head, level) LONG_RUNS samples sit on the last four integer positions of the last row (level 1: the
    last column), where only the taps along the row are in the map: the four pixels there collect 24, 25, 24 and 25
    entries; one more sample sits alone in the far corner (two pixels with one entry each); the others are out of
    range.  Which sample goes where is a stride-29 walk over (query, point), so every list mixes many waves' items."""
    nq = hw * hw
    b, q, m, i = _grid(B, nq)
    l, p = i // NP, i % NP
    shape = (B, nq, NH, NL * NP)
    q_off = 1.0
    if pattern == "pixel":
        tx = ((b + m + 2 * l) % hw).double().expand(shape)
        ty = ((3 * m + l + 1) % hw).double().expand(shape)
    elif pattern == "half":
        tx = ((b + m + 2 * l) % (hw - 1)).double().expand(shape) + 0.5
        ty = ((3 * m + l + 1) % (hw - 1)).double().expand(shape) + 0.5
        q_off = 0.5
    elif pattern == "zero":
        tx, ty = (q % hw).double().expand(shape), (q // hw).double().expand(shape)
    else:
        ns = nq * NP
        j = ((q * NP + p) * 29 + 5 * m + b) % ns
        edges = [sum(LONG_RUNS[:n + 1]) for n in range(4)]
        pos = sum((j >= e).to(torch.int64) for e in edges)                  # 0..3 on the line, 4 from edges[3] on
        on_line, lone = pos < 4, j == edges[3]
        last = torch.full(shape, float(hw - 1), dtype=F64)
        along = (hw - 4 + pos.clamp(max=3)).double().expand(shape)
        tx = torch.where(l == 0, along, last)
        ty = torch.where(l == 0, last, along)
        tx = torch.where(lone.expand(shape), torch.where(l == 0, last, torch.zeros(shape, dtype=F64)), tx)
        ty = torch.where(lone.expand(shape), torch.where(l == 0, torch.zeros(shape, dtype=F64), last), ty)
        away = torch.where((j % 2 == 0).expand(shape), torch.full(shape, -3.0, dtype=F64), torch.full(shape, hw + 2.0, dtype=F64))
        keep = (on_line | lone).expand(shape)
        tx, ty = torch.where(keep, tx, away), torch.where(keep, ty, away)
    return dict(value=_values(B, hw, 4), off=_offsets(tx.contiguous(), ty.contiguous(), hw), logits=_blend_logits(B, nq),
                g=_gout(B, hw, 3), q_off=q_off, q_a=0.125)


# ------------------------------------------------------------------------------------------------ bar families
def _bf16(t):
    return t.to(BF16).double()


def bar_unmoved(hw, B, variant):
    """Random problems at sizes that are no power of two, before the margin rule.  Values are multiples of 1/16 in
    [-4, 4] (exact in bf16 and fp16), logits, offsets and output gradients bf16 values."""
    nq = hw * hw
    g = H._gen(hw, B, len(variant), 7)
    value = (torch.randn(B, NL, nq, NH, DH, generator=g) * 16).round().clamp(-64, 64).double() / 16
    logits = _bf16(torch.randn(B, nq, NH, NL * NP, generator=g))
    gout = _bf16(torch.randn(B, nq, CM, generator=g))
    ref = ref_points(hw)
    if variant == "collapse":  # every sample near (0.4737, 0.4737) of its level: four pixels take all the taps
        tgt = 0.4737 + (torch.rand(B, nq, NH, NL, NP, 2, generator=g) - 0.5) * 2e-3
        off = (tgt - ref.view(1, nq, 1, 1, 1, 2)) * hw
    else:
        off = torch.randn(B, nq, NH, NL, NP, 2, generator=g) * 2.0
    return dict(value=value, off=_bf16(off), logits=logits, g=gout)


def _bar(hw, B, variant):
    """bar_unmoved with the margin rule applied; `moved` counts the offsets it displaced."""
    pr = bar_unmoved(hw, B, variant)
    nq, ref, off = hw * hw, ref_points(hw), pr["off"]
    # the margin: a coordinate within 1/16 pixel of an integer of [-1, hw] moves 1/8 pixel away from that integer
    # (deterministic; it stays on its side, so no sample enters or leaves the range).  The moved offset is rounded to
    # bf16 again: exact where the offset's ulp is at most 1/8 and no binade is crossed, otherwise off by at most half
    # an ulp, which for the offsets here (below 32 pixels) leaves at least 1/16 pixel -- the host test checks it
    c = (ref.double().view(1, nq, 1, 1, 1, 2) + off / hw) * hw - 0.5
    near = ((c - c.round()).abs() < MARGIN) & (c.round() >= -1) & (c.round() <= hw)
    off = torch.where(near, _bf16(off + torch.where(c >= c.round(), 0.125, -0.125)), off)
    return dict(pr, off=off, moved=int(near.sum()))


@functools.lru_cache(maxsize=None)
def problem(key):
    """The inputs of a case (float64; computed once, shared, never modified)."""
    family, hw, B, variant = key
    pr = {"gather": lambda: _gather(hw, B), "blend": lambda: _blend(hw, B), "buckets": lambda: _buckets(hw, B, variant),
          "bar": lambda: _bar(hw, B, variant)}[family]()
    pr.update(family=family, hw=hw, B=B, nq=hw * hw, variant=variant, ref=ref_points(hw), exact=family != "bar")
    return pr


# ------------------------------------------------------------------------------------------------ references
def weights(pr, dtype=F64):
    """Softmax weights [B][nq][8][8].  Exact families: torch's fp32 CPU softmax (exactly dyadic: exp(-200) is 0 in
    fp32), widened; bar families: the softmax in `dtype`."""
    if pr["exact"]:
        return torch.softmax(pr["logits"].float(), -1).to(dtype)
    return torch.softmax(pr["logits"].to(dtype), -1)


def run_oracle(pr, dtype=F64):
    """oracle.msda forward and backward in `dtype`, and what the fused ops derive from them: out [B][nq][512], gv
    [B][2][nq][8][64], gl (grad_loc) and goff = gl / hw [B][nq][8][2][4][2], ga (d / d weights) and gawl =
    a (ga - sum a ga) [B][nq][8][8]."""
    B, hw, nq = pr["B"], pr["hw"], pr["nq"]
    a = weights(pr, dtype)
    loc = pr["ref"].to(dtype).view(1, nq, 1, 1, 1, 2) + pr["off"].to(dtype) / hw
    val = pr["value"].to(dtype).reshape(B, NL * nq, NH, DH)
    shapes, starts = [(hw, hw)] * NL, [0, nq]
    aw = a.view(B, nq, NH, NL, NP)
    out = ms_deform_attn(val, shapes, starts, loc, aw)
    gv, gl, ga = ms_deform_attn_backward(val, shapes, starts, loc, aw, pr["g"].to(dtype))
    ga = ga.reshape(B, nq, NH, NL * NP)
    gawl = a * (ga - (a * ga).sum(-1, keepdim=True))
    return dict(out=out, gv=gv.view(B, NL, nq, NH, DH), gl=gl, goff=gl / hw, ga=ga, gawl=gawl, a=a, loc=loc)


@functools.lru_cache(maxsize=None)
def reference(key):
    """The float64 reference of a case (computed once, shared, never modified)."""
    return run_oracle(problem(key), F64)


@functools.lru_cache(maxsize=None)
def delta(key):
    """Per output tensor of a bar case: 4 x the largest elementwise |oracle in fp32 - oracle in fp64| on the same
    inputs, and not less than 2^-20 max|ref|.  The factor 4 (the project's convention for a kernel against the fp32
    restatement of its reference) covers the kernel's other summation order, FMA contraction and the device's expf
    and division."""
    r64, r32 = reference(key), run_oracle(problem(key), F32)
    return {n: max(4.0 * float((r32[n].double() - r64[n]).abs().max()), 2.0 ** -20 * float(r64[n].abs().max()))
            for n in OUTPUTS + ("gl", "ga")}


def bar(ref, d, dtype):
    """|got - ref| allowed for an output of `dtype` whose fp32 value before the cast lies within `d` of the fp64
    `ref`: d itself for fp32; head_probes.bf16_bar for bf16; for fp16 the same with its 11 significant bits, plus half
    the spacing 2^-24 of its subnormals."""
    if dtype == F32:
        return torch.full_like(ref, d)
    if dtype == BF16:
        return H.bf16_bar(ref, d)
    return 2.0 ** -11 * (ref.abs() + d) + d + 2.0 ** -25


def expected(t, dtype):
    """The fp64 reference rounded once to the output type (round to nearest even)."""
    return t.to(F32).to(dtype)


# ------------------------------------------------------------------------------------------------ layouts
def train_inputs(pr):
    """value [B * 2 * nq][512], off [B * nq][128], awl [B * nq][64], gout [B * nq][512] bf16; ref fp32 [nq][2]."""
    B, nq = pr["B"], pr["nq"]
    return dict(value=pr["value"].reshape(B * NL * nq, CM).to(BF16), off=pr["off"].reshape(B * nq, 128).to(BF16),
                awl=pr["logits"].reshape(B * nq, 64).to(BF16), gout=pr["g"].reshape(B * nq, CM).to(BF16), ref=pr["ref"])


def wide_rows(off, awl, fill=NAN, guard=0):
    """[rows + guard][WIDE] bf16: off at column 0, awl at column WIDE_AWL, `fill` in the gap, the tail and the guard."""
    rows = off.shape[0]
    t = torch.full((rows + guard, WIDE), fill, dtype=BF16)
    t[:rows, :128] = off.to(BF16)
    t[:rows, WIDE_AWL:WIDE_AWL + 64] = awl.to(BF16)
    return t


def infer_inputs(pr, dtype):
    """value [2][B][nq][512] (level-major) in `dtype`, offw [B * nq][192] fp32: 128 offsets, then 64 logits."""
    B, nq = pr["B"], pr["nq"]
    value = pr["value"].permute(1, 0, 2, 3, 4).reshape(NL * B * nq, CM).to(dtype)
    offw = torch.cat([pr["off"].reshape(B * nq, 128), pr["logits"].reshape(B * nq, 64)], 1).float()
    return value, offw


def generic_inputs(pr):
    """fp32 operands of mmt_ms_deform_attn_forward / _backward_impl: value (B, 2 nq, 8, 64), loc (B, nq, 8, 2, 4, 2)
    = ref + off / hw in fp32 (exact for the exact families), weights (B, nq, 8, 2, 4), grad_out (B, nq, 512)."""
    B, hw, nq = pr["B"], pr["hw"], pr["nq"]
    loc = pr["ref"].view(1, nq, 1, 1, 1, 2) + pr["off"].float() / hw
    return dict(value=pr["value"].reshape(B, NL * nq, NH, DH).float(), loc=loc.contiguous(),
                aw=weights(pr, F32).view(B, nq, NH, NL, NP).contiguous(), gout=pr["g"].float())


# ------------------------------------------------------------------------------------------------ census
def class_pairs(pr, nonzero_only=True):
    """The (x class, y class) pairs among the samples (of non-zero weight), computed from the inputs."""
    x, y = coords(pr)
    cx, cy = axis_class(x, pr["hw"]), axis_class(y, pr["hw"])
    keep = (weights(pr).view(x.shape) > 0) if nonzero_only else torch.ones_like(cx, dtype=torch.bool)
    return set(zip(cx[keep].tolist(), cy[keep].tolist()))


def tap_table(pr):
    """Every tap as the gathers see it: (valid [B][nq][8][8][4], pixel, weight), tap order (0,0), (0,+1), (+1,0),
    (+1,+1) in (row, column)."""
    hw = pr["hw"]
    x, y = (t.reshape(pr["B"], pr["nq"], NH, NL * NP) for t in coords(pr))
    inside = (x > -1) & (y > -1) & (x < hw) & (y < hw)
    x0, y0 = x.floor(), y.floor()
    lw, lh = x - x0, y - y0
    valid, pix, wt = [], [], []
    for dy, dx, w in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
        xi, yi = x0.long() + dx, y0.long() + dy
        valid.append(inside & (xi >= 0) & (xi <= hw - 1) & (yi >= 0) & (yi <= hw - 1))
        pix.append(yi.clamp(0, hw - 1) * hw + xi.clamp(0, hw - 1))
        wt.append(w)
    return torch.stack(valid, -1), torch.stack(pix, -1), torch.stack(wt, -1)


def bucket_lengths(pr):
    """Entries per (batch, head, level, pixel) list of the value gather: [B][8][2][nq]."""
    B, nq = pr["B"], pr["nq"]
    valid, pix, _ = tap_table(pr)
    b, q, m, i = _grid(B, nq)
    flat = (((b * NH + m) * NL + i // NP) * nq)[..., None] + pix
    n = torch.zeros(B * NH * NL * nq, dtype=torch.int64)
    n.index_put_((flat[valid],), torch.ones(int(valid.sum()), dtype=torch.int64), accumulate=True)
    return n.view(B, NH, NL, nq)


def bucket_wave_spread(pr):
    """The largest number of distinct waves of msda_train_bwd_value_kernel whose item runs feed one list.  Items are
    i = 4 (4 q + p) + tap, wave w owns [w per, (w + 1) per), per = ceil(16 nq / VT) * 64."""
    B, nq = pr["B"], pr["nq"]
    valid, pix, _ = tap_table(pr)
    b, q, m, i = _grid(B, nq)
    per = (16 * nq + VT - 1) // VT * 64
    item = ((q * NP + i % NP) * 4)[..., None] + torch.arange(4)
    wave = (item // per).expand(valid.shape)
    flat = ((((b * NH + m) * NL + i // NP) * nq)[..., None] + pix)
    seen = torch.zeros(B * NH * NL * nq, VT // 64, dtype=torch.bool)
    seen[flat[valid], wave[valid]] = True
    return int(seen.sum(1).max())
