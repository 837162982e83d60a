"""Probe inputs, references and bars of the training step's glue kernels (no tests here): the eight entry points of
csrc/fusion_train.hip (mmt_ft_query_prep, mmt_ft_drop_residual, mmt_ft_relu_drop, mmt_ft_rows_cast and their _bwd),
mmt_box_loss / _bwd of csrc/loss.hip and mmt_adamw_step of csrc/optim.hip.

Bitwise families.  fusion_train.hip only moves, adds, or multiplies once with a bf16 rounding (done with bit
operations) before the next addition, so a torch restatement on the CPU -- fp32 operations in the kernel's stated
order, .bfloat16() where the kernel rounds -- predicts every bit.  The dropout keep factors come from a numpy uint64
restatement of the counter hash (ft_mix / ft_key / draws / drop_params below, written from the header's and the
source's comments).  The box loss on dyadic boxes of equal aspect ratio (loss_exact_batch) and AdamW on dyadic
operands (the census, moments and norm families) have results that are exact in fp32 in any order.

Bar families.  The box loss on random boxes: per-sample rows of dpred and the four scalars within 4x the worst error
of the same composition (train.box_loss) evaluated in float32 on the CPU against float64 (LOSS_ROW_EMUL,
LOSS_SCALAR_EMUL; the host test recomputes them).  The AdamW update on N(0, 1) data: p, m, v within a counted number
of fp32 roundings of the float64 formula (AW_N_P, AW_N_M, AW_N_V beside adamw_ref64).  Nothing in a bar comes from
the kernels.

Storage images (head_probes.image / poison, gemm_probes.same / describe) are GUARD rows or elements larger than the
problem, NaN outside it, and compared whole.  Functions with a `mut` argument restate the same arithmetic with one
planted defect (the host test's negative controls).
"""
import dataclasses
import functools
import math

import numpy as np
import torch

import gemm_probes as P
import head_probes as H

NAN = P.NAN
GUARD = H.GUARD
EBADARG = H.EBADARG
U32 = H.U32
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16

WG = 256                    # 8-element work items per workgroup of every kernel of fusion_train.hip
CHUNK = 1 << 16             # elements per AdamW chunk (optim.hip)
BL_T = 256                  # threads of box_loss_kernel / samples per workgroup of its backward (loss.hip)
ADAMW_MAX_GROUPS = 8        # MMT_ADAMW_MAX_GROUPS (mmt_hip.h)
MIX_A, MIX_B = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB  # splitmix64's finaliser
CTR_MUL = 0x9E3779B97F4A7C15                          # the step counter's multiplier in the key
WORD_MUL = 0xD1B54A32D192ED03                         # the draw word index's multiplier


def chunk_class(items):
    """Where a launch of `items` 8-element work items ends: below one workgroup, exactly one, whole workgroups, or
    k workgroups and a partial one."""
    return "below" if items < WG else "exact" if items == WG else "multiple" if items % WG == 0 else "ragged"


# ------------------------------------------------------------------------------------------------ the dropout hash
def ft_mix(x):
    """splitmix64's finaliser on a uint64 array (arithmetic modulo 2^64)."""
    x = np.array(x, dtype=np.uint64, ndmin=1)
    x ^= x >> np.uint64(30)
    x *= np.uint64(MIX_A)
    x ^= x >> np.uint64(27)
    x *= np.uint64(MIX_B)
    x ^= x >> np.uint64(31)
    return x


def ft_key(seed, counter, salt):
    """The call site's key: mix(seed ^ mix(counter * CTR_MUL + salt))."""
    c = np.array([counter], dtype=np.uint64) * np.uint64(CTR_MUL) + np.uint64(salt)
    return ft_mix(np.array([seed], dtype=np.uint64) ^ ft_mix(c))


def draws(key, n, mut=None):
    """The 16-bit draws of elements 0 .. n - 1: element e takes field e % 4 (bits 16 f .. 16 f + 15) of the word
    mix(key ^ (e // 4) * WORD_MUL).  mut fields_reversed: field 3 - e % 4."""
    words = ft_mix(key ^ (np.arange(-(-n // 4), dtype=np.uint64) * np.uint64(WORD_MUL)))
    shifts = np.arange(4, dtype=np.uint64) * np.uint64(16)
    if mut == "fields_reversed":
        shifts = shifts[::-1]
    return ((words[:, None] >> shifts[None, :]) & np.uint64(0xFFFF)).reshape(-1)[:n].astype(np.int64)


def drop_params(p, rng=True):
    """(on, thr, scale) as make_drop computes them from the float argument p: keep = 1 - float32(p) in double,
    thr = floor(keep * 65536 + 0.5), scale = float32(1 / keep); rng NULL or p == 0: no dropout."""
    p32 = float(np.float32(p))
    on = bool(rng) and p32 > 0.0
    keep = 1.0 - p32
    return on, int(keep * 65536.0 + 0.5), float(np.float32(1.0 / keep)) if on else 1.0


@dataclasses.dataclass(frozen=True)
class Drop:
    p: float
    rng: bool = True
    seed: int = 0x1234567
    counter: int = 0
    salt: int = 1

    @property
    def name(self):
        return "p%g%s-s%x-c%x-salt%d" % (self.p, "" if self.rng else "-norng", self.seed, self.counter, self.salt)


P_THR_FULL = 2.0 ** -17       # thr = 65536: every element kept, still scaled by float32(1 / (1 - 2^-17)) = 1 + 2^-17
P_THR_ONE = 1.0 - 2.0 ** -16  # thr = 1: only a draw of 0 is kept, scaled by 65536
P_THR_ROUND = 131069 / 262144  # (1 - p) 65536 = 32768.75: thr = 32769 rounded to nearest, 32768 truncated
DROPS = (Drop(0.5), Drop(0.1), Drop(0.0), Drop(0.5, rng=False), Drop(P_THR_FULL), Drop(P_THR_ONE), Drop(P_THR_ROUND))
# one key component varied at a time; the salts are the encoder step's 8 li + 1 .. 8 li + 3
KEYS = (Drop(0.5), Drop(0.5, seed=(1 << 61) + 12345), Drop(0.5, counter=1), Drop(0.5, counter=(1 << 32) + 5),
        Drop(0.5, salt=2), Drop(0.5, salt=3), Drop(0.5, salt=9), Drop(0.5, salt=10), Drop(0.5, salt=11))


def keep_factors(shape, dr, mut=None):
    """fp32 keep factors (scale or 0) of a call site's tensor of `shape`, indexed by its flat element index; None
    without dropout.  mut: salt_ignored, fields_reversed."""
    on, thr, scale = drop_params(dr.p, dr.rng)
    if not on:
        return None
    n = int(np.prod(shape))
    r = draws(ft_key(dr.seed, dr.counter, 0 if mut == "salt_ignored" else dr.salt), n, mut)
    return torch.from_numpy(np.where(r < thr, np.float32(scale), np.float32(0.0)).astype(np.float32)).view(shape)


def rng_state(dr):
    """{seed, counter} as the kernels read it (int64), or None."""
    return torch.tensor([dr.seed, dr.counter], dtype=torch.int64) if dr.rng else None


def _rbf(t):
    return t.bfloat16().float()


# ------------------------------------------------------------------------------------------------ 1. query_prep
QP_SHAPES = ((1, 1, 8), (3, 5, 24), (3, 37, 40), (1, 16, 64), (2, 400, 768))            # (B, nq, d)
QPB_SHAPES = ((1, 1, 8), (3, 5, 24), (3, 37, 40), (16, 5, 24), (1, 16, 64), (16, 37, 40), (2, 400, 768))
QP_FAMILIES = ("int", "randn")


def qp_items(B, nq, d):
    return B * 2 * nq * (d // 8)


def qpb_items(B, nq, d):
    return 2 * nq * (d // 8)   # one work item per 8 elements of lpos, looping over the batch


def _vals(shape, family, g, hi=100):
    return H._nonzero(shape, 1, hi, g).float() if family == "int" else torch.randn(shape, generator=g)


@functools.lru_cache(maxsize=None)
def qp_problem(shape, family):
    B, nq, d = shape
    g = H._gen(B, nq, d, len(family), 11)
    return dict(src=_vals((B, 2, nq, d), family, g), lpos=_vals((2, nq, d), family, g))


def qp_expected(pr, mut=None):
    """qbi [B][nq][2][d] = bf16(src + lpos) of the halves side by side, srcb = bf16(src).  mut halves_swapped."""
    q = (pr["src"] + pr["lpos"]).bfloat16()
    if mut == "halves_swapped":
        q = q.flip(1)
    return q.permute(0, 2, 1, 3).contiguous(), pr["src"].bfloat16()


@functools.lru_cache(maxsize=None)
def qpb_problem(shape, family):
    B, nq, d = shape
    g = H._gen(B, nq, d, len(family), 12)
    hi = 40  # integers: dthrough + dq + dsrcb stays below 256, and 16 samples' dq below 2^24
    return dict(dqbi=_vals((B, nq, 2, d), family, g, hi).bfloat16(), dsrcb=_vals((B, 2, nq, d), family, g, hi).bfloat16(),
                dthrough=_vals((B, 2, nq, d), family, g, hi))


def qpb_expected(pr, through, mut=None):
    """dsrc = (dthrough + unshuffle(dqbi)) + dsrcb; dlpos = the samples' unshuffle(dqbi) added in batch order from
    0.f.  mut: no_last_sample (dlpos over B - 1 samples)."""
    dq = pr["dqbi"].float().permute(0, 2, 1, 3)
    dsrc = ((pr["dthrough"] + dq) if through else dq) + pr["dsrcb"].float()
    acc = torch.zeros(dq.shape[1:], dtype=F32)
    for b in range(dq.shape[0] - (1 if mut == "no_last_sample" else 0)):
        acc = acc + dq[b]
    return dsrc.contiguous(), acc


# ------------------------------------------------------------------------------------------------ 2. drop_residual
DR_SHAPES = ((1, 2, 8), (3, 10, 24), (3, 74, 40), (1, 32, 64), (1, 64, 64), (2, 800, 768))   # (B, rows, d), rows even
DR_ODD_SHAPES = ((1, 1, 8), (3, 5, 24), (3, 37, 40))                                          # dup 0 only
DR_BIG = (2, 800, 768)


def dr_items(shape, dup, bwd):
    B, rows, d = shape
    return B * (rows // 2 if (dup and bwd) else rows) * (d // 8)


def _dr_cases():
    out = []
    for dup in (0, 1):
        for shape in DR_SHAPES + (() if dup else DR_ODD_SHAPES):
            # the frame's geometry: the model's p, and the two thresholds that need many draws to show
            drops = (Drop(0.1), Drop(P_THR_ONE), Drop(P_THR_ROUND)) if shape == DR_BIG else DROPS
            out += [(shape, dup, dr) for dr in drops]
    out += [((3, 74, 40), dup, k) for dup in (0, 1) for k in KEYS[1:]]
    return tuple(out)


DR_CASES = _dr_cases()


def dr_id(case):
    return "B%d-r%d-d%d-dup%d-%s" % (case[0] + (case[1], case[2].name))


@functools.lru_cache(maxsize=None)
def dr_problem(shape, dup):
    B, rows, d = shape
    g = H._gen(B, rows, d, dup, 13)
    dout = torch.randn(B, rows, d, generator=g)
    if dup:
        dout[:, rows // 2:] *= 3.0   # the halves differ in scale as well
    return dict(x=torch.randn(B, rows, d, generator=g), y=torch.randn(B, rows // 2 if dup else rows, d, generator=g).bfloat16(),
                dout=dout)


def dr_expected(pr, dup, dr, mut=None):
    """out = x + bf16(y * k), k indexed by out's flat element index; dup: y on both halves of the rows."""
    y = pr["y"].float()
    if dup:
        y = torch.cat([y, y], 1)
    k = keep_factors(pr["x"].shape, dr, mut)
    return pr["x"] + (y if k is None else _rbf(y * k))


def drb_expected(pr, dup, dr, mut=None):
    """dy = bf16(sum over the halves of bf16(bf16(dout) * k)), k at out's index.  mut mask_at_dy: both halves take
    the factors at dy's own flat index."""
    g = _rbf(pr["dout"])
    k = keep_factors(pr["dout"].shape, dr, mut)
    if dup and mut == "mask_at_dy" and k is not None:
        half = k.reshape(-1)[:k.numel() // 2].view(k.shape[0], k.shape[1] // 2, k.shape[2])
        k = torch.cat([half, half], 1)
    if k is not None:
        g = _rbf(g * k)
    if dup:
        h = g.shape[1] // 2
        g = g[:, :h] + g[:, h:]
    return g.bfloat16()


# ------------------------------------------------------------------------------------------------ 3. relu_drop
RD_NS = (8, 2048, 8 * 257)
RD_DROPS = (Drop(0.5, salt=2), Drop(0.1, salt=10), Drop(P_THR_FULL, salt=2), Drop(P_THR_ONE, salt=2))
RDB_DROPS = RD_DROPS + (Drop(0.0, salt=2), Drop(0.5, rng=False, salt=2))   # the forward refuses these two
BF16_MIN_NORMAL = 2.0 ** -126
RD_LARGE = 2.0 ** 100


@functools.lru_cache(maxsize=None)
def rd_problem(n):
    """h = relu(.) in bf16: exact zeros, the smallest positive normal, large values and |N(0, 1)|; dy N(0, 1)."""
    g = H._gen(n, 14)
    h = torch.randn(n, generator=g).abs()
    i = torch.arange(n)
    h[i % 4 == 0] = 0.0
    h[i % 8 == 1] = BF16_MIN_NORMAL
    h[i % 8 == 3] = RD_LARGE
    return dict(h=h.bfloat16(), dy=torch.randn(n, generator=g).bfloat16())


def rd_expected(pr, dr, mut=None):
    return (pr["h"].float() * keep_factors(pr["h"].shape, dr, mut)).bfloat16()


def rdb_expected(pr, dr, mut=None):
    g = pr["dy"].float()
    k = keep_factors(g.shape, dr, mut)
    if k is not None:
        g = g * k
    return torch.where(pr["h"].float() > 0, g, torch.zeros_like(g)).bfloat16()


# ------------------------------------------------------------------------------------------------ 4. rows_cast
RC_WINDOWS = ((1, 1, 0, 1), (3, 11, 0, 11), (3, 11, 4, 3), (3, 11, 10, 1), (2, 528, 128, 400))  # (S, rows, row0, nrows)
RC_CS = (8, 24, 768)
# one workgroup exactly: the forward (2 * 16 * 8 items) and the backward (1 * 32 * 8 items)
RC_CASES = tuple(w + (C,) for w in RC_WINDOWS for C in RC_CS) + ((2, 32, 8, 16, 64), (1, 32, 4, 8, 64))


def rc_items(case, bwd):
    S, rows, row0, nrows, C = case
    return S * (rows if bwd else nrows) * (C // 8)


@functools.lru_cache(maxsize=None)
def rc_problem(case):
    S, rows, row0, nrows, C = case
    g = H._gen(*case, 15)
    return dict(x=torch.randn(S, rows, C, generator=g) * 3, dout=torch.randn(S, nrows, C, generator=g).bfloat16())


def rc_expected(case, pr, mut=None):
    """(out, dx).  mut window_unwritten: the rows outside the window left as they were (NaN) by the backward."""
    S, rows, row0, nrows, C = case
    dx = torch.full((S, rows, C), NAN if mut == "window_unwritten" else 0.0, dtype=F32)
    dx[:, row0:row0 + nrows] = pr["dout"].float()
    return pr["x"][:, row0:row0 + nrows].bfloat16().contiguous(), dx


# ------------------------------------------------------------------------------------------------ 5. box loss
LOSS_W = (1.5, 3.0)      # (iou_w, l1_w): not the defaults, dyadic
LOSS_DLOSS = 0.75
LOSS_EXACT_BS = (1, 256, 512)
LOSS_BAR_BS = (3, 257, 300)

# Exact family: (pred xyxy, gt xyxy before the clamp, side of the enclosing square) in units of 2^-4.  Both boxes of
# a sample have the same aspect ratio (w / h bitwise equal: both atan terms cancel), the enclosing box is a square of
# side 2^-k (c_diag = 2 E^2 is a power of two) unless the centres coincide (inter_diag = 0), and the union is a power
# of two wherever the intersection's gradient is passed on (overlap or contact): then every quotient of the forward
# and of both backward derivations is a dyadic number of a few bits, the same in fp32 and fp64 in any order.
LOSS_CATEGORIES = {
    # no overlap in either axis: iou = 0, the gradient comes from u alone
    "disjoint2": (((0, 0, 2, 2), (6, 6, 8, 8), 8), ((0, 0, 3, 3), (6, 6, 8, 8), 8), ((5, 0, 8, 3), (0, 4, 4, 8), 8),
                  ((4, 4, 8, 8), (0, 0, 1, 1), 8), ((0, 2, 2, 4), (3, 0, 4, 1), 4)),
    # separated in one axis, overlapping in the other (w = h / 2 or h = w / 2): mi < 0 blocks the intersection's gradient
    "disjoint1": (((0, 0, 3, 6), (5, 2, 8, 8), 8), ((0, 2, 2, 6), (4, 0, 8, 8), 8), ((2, 5, 8, 8), (0, 0, 6, 3), 8),
                  ((6, 1, 8, 5), (0, 0, 4, 8), 8)),
    # contact (mi == 0): the clamp passes the gradient at its bound; corner contact, and edge contact with shared y edges
    "touching": (((0, 0, 4, 4), (4, 4, 8, 8), 8), ((2, 0, 4, 2), (0, 2, 2, 4), 4), ((4, 4, 8, 8), (0, 0, 4, 4), 8),
                 ((0, 0, 4, 8), (4, 0, 8, 8), 8)),
    # shared edges: min / max ties split 1/2, sign(0) = 0 in the L1 term
    "shared": (((0, 0, 8, 6), (0, 2, 8, 8), 8), ((0, 3, 8, 8), (0, 0, 8, 5), 8), ((0, 0, 6, 8), (2, 0, 8, 8), 8),
               ((0, 0, 8, 8), (0, 0, 4, 4), 8), ((6, 6, 8, 8), (0, 0, 8, 8), 8)),
    # gt reaching past [0, 1]: clamped before everything else (these sit at fixed positions)
    "clamped": (((13, 13, 15, 15), (12, 12, 20, 20), 0), ((8, 8, 16, 16), (14, 14, 22, 22), 0),
                ((0, 0, 8, 8), (-4, -4, 2, 2), 0), ((-2, 10, 6, 18), (-6, 12, 4, 24), 0)),
    # containment, concentric: iou 1/4 and 1/16, u = 0
    "contained": (((0, 0, 8, 8), (2, 2, 6, 6), 8), ((0, 0, 8, 8), (3, 3, 5, 5), 8), ((2, 2, 6, 6), (0, 0, 8, 8), 8),
                  ((0, 0, 4, 4), (1, 1, 3, 3), 4)),
    # iou above 0.5 with v = 0: alpha = 1 * 0 / (1 - iou + 0) = 0 exactly
    "iou_high": (((0, 0, 8, 8), (1, 1, 7, 7), 8), ((1, 1, 7, 7), (0, 0, 8, 8), 8), ((0, 0, 8, 7), (0, 1, 8, 8), 8),
                 ((0, 0, 8, 8), (0, 0, 6, 6), 8), ((0, 0, 8, 8), (2, 2, 8, 8), 8)),
}
LOSS_CAT_NAMES = tuple(LOSS_CATEGORIES)


def _loss_sample(cat, variant, i):
    """(pred cxcywh, gt xywh) of one exact sample, moved by a multiple of 2^-4 that depends on i (no value of the
    loss depends on it: it only changes the operands)."""
    p, g, E = LOSS_CATEGORIES[cat][variant % len(LOSS_CATEGORIES[cat])]
    ox, oy = ((5 * i) % (17 - E), (3 * i) % (17 - E)) if E else (0, 0)
    p = [(p[0] + ox) / 16.0, (p[1] + oy) / 16.0, (p[2] + ox) / 16.0, (p[3] + oy) / 16.0]
    g = [(g[0] + ox) / 16.0, (g[1] + oy) / 16.0, (g[2] + ox) / 16.0, (g[3] + oy) / 16.0]
    return ([(p[0] + p[2]) / 2, (p[1] + p[3]) / 2, p[2] - p[0], p[3] - p[1]], [g[0], g[1], g[2] - g[0], g[3] - g[1]])


@functools.lru_cache(maxsize=None)
def loss_exact_batch(B, only=None):
    """(pred [B][4], gt [B][4], category index per sample) in float64: sample i takes category i % 7 and that
    category's variant i // 7, so neighbours always differ; `only` names one category for all samples."""
    pred, gt, cats = [], [], []
    n = len(LOSS_CAT_NAMES)
    for i in range(B):
        c = LOSS_CAT_NAMES.index(only) if only else i % n
        p, g = _loss_sample(LOSS_CAT_NAMES[c], i if only else i // n, i)
        pred.append(p), gt.append(g), cats.append(c)
    return torch.tensor(pred, dtype=F64), torch.tensor(gt, dtype=F64), torch.tensor(cats)


@functools.lru_cache(maxsize=None)
def loss_random_batch(B):
    """Random boxes in the distribution of test_hip_box_loss_matches_autograd (gt corner U(0, 0.6), size 0.1 + U(0, 0.4);
    pred = the gt's centre moved by 0.05 N(0, 1) and its size scaled by 1 + 0.2 N(0, 1)): about half the samples have
    IoU above 0.5.  Samples are redrawn until no operand pair of a min / max is closer than 2^-10 and
    every width and height is at least 2^-4 (ties belong to the exact family).  float32 values, as float64."""
    g = H._gen(B, 16)
    gt = torch.zeros(B, 4)
    pred = torch.zeros(B, 4)
    todo = torch.ones(B, dtype=torch.bool)
    noise = 0.05
    for _ in range(64):
        ngt = torch.cat([torch.rand(B, 2, generator=g) * 0.6, 0.1 + torch.rand(B, 2, generator=g) * 0.4], 1)
        npred = torch.cat([ngt[:, :2] + ngt[:, 2:] / 2 + torch.randn(B, 2, generator=g) * noise,
                           ngt[:, 2:] * (1 + torch.randn(B, 2, generator=g) * 4 * noise)], 1)
        gt[todo], pred[todo] = ngt[todo], npred[todo]
        todo = ~loss_separated(pred.double(), gt.double())
        if not bool(todo.any()):
            break
    assert not bool(todo.any())
    return pred.double(), gt.double()


def loss_boxes(pred, gt):
    """The xyxy boxes the loss compares: pred from cxcywh, gt from xywh clamped to [0, 1]."""
    b1 = torch.cat([pred[:, :2] - 0.5 * pred[:, 2:], pred[:, :2] + 0.5 * pred[:, 2:]], -1)
    b2 = torch.cat([gt[:, :2], gt[:, :2] + gt[:, 2:]], -1).clamp(0.0, 1.0)
    return b1, b2


def loss_separated(pred, gt):
    """Per sample: every edge pair at least 2^-10 apart and every width / height at least 2^-4."""
    b1, b2 = loss_boxes(pred, gt)
    far = ((b1 - b2).abs() >= 2.0 ** -10).all(1)
    wide = torch.cat([b1[:, 2:] - b1[:, :2], b2[:, 2:] - b2[:, :2]], 1).min(1).values >= 2.0 ** -4
    return far & wide


def loss_iou(pred, gt):
    b1, b2 = loss_boxes(pred, gt)
    iwh = (torch.min(b1[:, 2:], b2[:, 2:]) - torch.max(b1[:, :2], b2[:, :2])).clamp(min=0)
    inter = iwh[:, 0] * iwh[:, 1]
    return inter / ((b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1]) + (b2[:, 2] - b2[:, 0]) * (b2[:, 3] - b2[:, 1]) - inter)


def loss_oracle(pred, gt, dtype=F64, mut=None):
    """train.box_loss under autograd on the CPU in `dtype`: (out[4] = loss, ciou, l1, mean iou; dpred [B][4]) for
    d loss = LOSS_DLOSS.  mut: sample_dropped (the last sample left out of the means), tie_one_zero (a tie's gradient
    all to one operand: the tied pred edges moved by 2^-30 towards the inside of gt)."""
    from mmt_amd import train
    p, g = pred.to(dtype).clone(), gt.to(dtype)
    if mut == "tie_one_zero":
        b1, b2 = loss_boxes(p, g)
        tie = b1 == b2
        b1 = b1 + tie * torch.tensor([1.0, 1.0, -1.0, -1.0], dtype=dtype) * 2.0 ** -30
        p = torch.cat([(b1[:, :2] + b1[:, 2:]) / 2, b1[:, 2:] - b1[:, :2]], 1)
    p.requires_grad_(True)
    n = p.shape[0] - (1 if mut == "sample_dropped" else 0)
    loss, st = train.box_loss(p[:n].view(n, 1, 4), g[:n], *LOSS_W)
    (LOSS_DLOSS * loss).backward()
    return torch.stack([loss.detach(), st["ciou"], st["l1"], st["iou"]]), p.grad.detach()


@functools.lru_cache(maxsize=None)
def loss_reference(kind, B):
    """(pred, gt, out, dpred) in float64, computed once, shared, never modified."""
    pred, gt = loss_exact_batch(B)[:2] if kind == "exact" else loss_random_batch(B)
    return (pred, gt) + loss_oracle(pred, gt, F64)


def loss_row_err(got, ref):
    """The worst sample: each row's max abs error relative to the larger of that row's max abs reference gradient and
    the batch median of the rows' max abs gradients."""
    scale = ref.abs().max(1).values
    scale = torch.maximum(scale, scale.median())
    return float(((got.double() - ref).abs().max(1).values / scale).max())


def loss_scalar_err(got, ref):
    return float(((got.double() - ref).abs() / ref.abs()).max())


# 4x the worst error of train.box_loss evaluated in float32 on the CPU against float64 over LOSS_BAR_BS (the project's
# rule for BWD_ROW_BAR); the host test recomputes the two measured values.  Nothing here comes from the kernels.
LOSS_ROW_EMUL = 9.59e-7
LOSS_SCALAR_EMUL = 3.48e-7
LOSS_ROW_BAR, LOSS_SCALAR_BAR = 4 * LOSS_ROW_EMUL, 4 * LOSS_SCALAR_EMUL


# ------------------------------------------------------------------------------------------------ 6. AdamW
AW_SIZES = (1, 3, 4, 7, 65535, 65536, 65537, 2 * 65536 + 5)
AW_GROUPS = tuple(i % 3 for i in range(len(AW_SIZES)))
AW_NO_SHADOW = (2, 5)       # tensors without a bf16 shadow (n = 4 and n = 65536)
AW_TOTAL = sum(AW_SIZES)
AW_ALIGN = {"p": 4, "g": 4, "m": 4, "v": 4, "shadow": 8}   # elements in 16 bytes
# misalignments in elements of the buffer's type: g alone, p / m / v alone, all four, the shadow alone
AW_LAYOUTS = {"aligned": {}, "g1": {"g": 1}, "g2": {"g": 2}, "g3": {"g": 3}, "p1": {"p": 1}, "m1": {"m": 1},
              "v1": {"v": 1}, "all": {"p": 1, "g": 2, "m": 3, "v": 1}, "sh1": {"shadow": 1}, "sh3": {"shadow": 3}}


def aw_chunks():
    """[(tensor, first element, elements)] in launch order."""
    return [(i, o, min(CHUNK, n - o)) for i, n in enumerate(AW_SIZES) for o in range(0, n, CHUNK)]


def aw_starts(layout, name):
    """(first element of every tensor in buffer `name`, the buffer's length): tensors at least GUARD elements apart,
    each start a multiple of 16 bytes plus the layout's misalignment."""
    a, mis = AW_ALIGN[name], AW_LAYOUTS[layout].get(name, 0)
    starts, pos = [], GUARD
    for n in AW_SIZES:
        s = -(-pos // a) * a + mis
        starts.append(s)
        pos = s + n + GUARD
    return starts, -(-pos // a) * a


def aw_image(flat, layout, name, dtype):
    """The NaN-filled buffer `name` with the tensors' values (flat: all tensors back to back) in place; the shadow
    buffer holds only the tensors that have one.  flat None: all NaN."""
    starts, total = aw_starts(layout, name)
    img = torch.full((total,), NAN, dtype=dtype)
    o = 0
    for i, (s, n) in enumerate(zip(starts, AW_SIZES)):
        if flat is not None and not (name == "shadow" and i in AW_NO_SHADOW):
            img[s:s + n] = flat[o:o + n].to(dtype)
        o += n
    return img


def aw_flat(img, layout, name):
    starts, _ = aw_starts(layout, name)
    return torch.cat([img[s:s + n] for s, n in zip(starts, AW_SIZES)])


def aw_per_element(values):
    """A per-group value spread over the flat element vector."""
    return torch.cat([torch.full((n,), float(values[g]), dtype=F64) for n, g in zip(AW_SIZES, AW_GROUPS)])


@dataclasses.dataclass(frozen=True)
class AWHyper:
    lr: tuple
    wd: tuple
    b1: float = 0.9
    b2: float = 0.999
    eps: float = 1e-8
    max_norm: float = 0.0


AW_CENSUS_HP = AWHyper(lr=(0.5, 0.25, 0.5), wd=(1.0, 3.0, 0.0))          # 1 - lr wd = 1/2, 1/4, 1
AW_CENSUS_FACTORS = (0.5, 0.25, 1.0)
AW_MOMENTS_HP = AWHyper(lr=(1e-3, 2e-4, 1e-4), wd=(1e-2, 1e-4, 0.0), b1=0.5, b2=0.75)
AW_NORM_HP = AWHyper(lr=(1e-3, 2e-4, 1e-4), wd=(1e-2, 1e-4, 0.0), max_norm=0.5)
AW_UPDATE_HPS = {"clip": AWHyper(lr=(1e-3, 2e-4, 1e-4), wd=(1e-2, 1e-4, 0.0), max_norm=1.0),      # norm ~ 572
                 "noclip": AWHyper(lr=(1e-3, 2e-4, 1e-4), wd=(1e-2, 1e-4, 0.0), max_norm=1e4)}
AW_UPDATE_STEPS = 3


@functools.lru_cache(maxsize=None)
def aw_problem(family):
    """Flat fp32 p, g, m, v of all tensors back to back.
    census: p integers of magnitude 1..100, g = -0.0 (so that zero_grad's +0.0 shows in the bits), m = v = 0;
    moments: g and m integers, v multiples of 1/4; norm: g = 1; update: N(0, 1) p and g, moments as after a step."""
    g = H._gen(len(family), 17)
    n = AW_TOTAL
    if family == "census":
        return dict(p=H._nonzero((n,), 1, 100, g).float(), g=torch.full((n,), -0.0), m=torch.zeros(n), v=torch.zeros(n))
    if family == "moments":
        return dict(p=torch.randn(n, generator=g), g=H._nonzero((n,), 1, 3, g).float(), m=H._nonzero((n,), 1, 8, g).float(),
                    v=torch.randint(0, 65, (n,), generator=g).float() / 4)
    if family == "norm":
        return dict(p=torch.randn(n, generator=g), g=torch.ones(n), m=torch.zeros(n), v=torch.zeros(n))
    return dict(p=torch.randn(n, generator=g), g=torch.randn(n, generator=g), m=0.1 * torch.randn(n, generator=g),
                v=0.001 * torch.randn(n, generator=g) ** 2)


def aw_census_expected(steps, mut=None):
    """(p, shadow as bf16) after `steps` census steps: p times its own group's factor once per step.  mut:
    chunk_last_skipped (the last element of the 65537-element tensor's first chunk keeps its value), group_zero (every tensor takes
    group 0's factor)."""
    p = aw_problem("census")["p"].double()
    f = aw_per_element((AW_CENSUS_FACTORS[0],) * 3 if mut == "group_zero" else AW_CENSUS_FACTORS)
    out = p * f ** steps
    if mut == "chunk_last_skipped":
        first = sum(AW_SIZES[:AW_SIZES.index(CHUNK + 1)])
        out[first + CHUNK - 1] = p[first + CHUNK - 1]
    return out.float(), out.float().bfloat16()


def aw_shadow_image(flat_bf16, layout, mut=None):
    """The shadow buffer's expected image.  mut tail_unwritten: the elements behind the last whole float4 of every
    chunk (the scalar tail of the vector path) left NaN."""
    img = aw_image(flat_bf16, layout, "shadow", BF16)
    if mut == "tail_unwritten":
        starts, _ = aw_starts(layout, "shadow")
        for i, o, n in aw_chunks():
            if i not in AW_NO_SHADOW:
                img[starts[i] + o + (n & ~3):starts[i] + o + n] = NAN
    return img


def aw_moments_expected(steps):
    """m, v after `steps` steps with the same g: m = m / 2 + g / 2, v = 3 v / 4 + g^2 / 4, exact in fp32."""
    pr = aw_problem("moments")
    m, v, g = pr["m"].double(), pr["v"].double(), pr["g"].double()
    for _ in range(steps):
        m, v = 0.5 * m + 0.5 * g, 0.75 * v + 0.25 * g * g
    return m.float(), v.float()


def aw_norm_bound():
    """Relative bound of the fp32 norm against float64: a thread adds CHUNK / 256 squares in sequence, the tree adds
    8 levels, the squares round once (or not at all, fused): (CHUNK / 256 + 8 + 1) U32 on the sum of squares, halved
    by the square root, plus the double sum's cast to fp32 (U32)."""
    return ((CHUNK // 256 + 9) / 2 + 1) * U32


def f32(x):
    return float(np.float32(x))


def aw_state_ref(hp, t, norm):
    """(clip factor, 1 - b1^t, sqrt(1 - b2^t)) in float64 from the norm the device reports."""
    c = min(1.0, hp.max_norm / (norm + 1e-6)) if hp.max_norm > 0 else 1.0
    return c, 1.0 - hp.b1 ** t, math.sqrt(1.0 - hp.b2 ** t)


# fp32 roundings on the way to each output of adamw_one (a division or square root counted as 2: one ulp):
#   g' = g c (1);  m: b1 m (1), (1 - b1) g' (1 + g' 1), the sum (1)                                       -> AW_N_M = 4
#   v: (1 - b2) g' (1 + g' 1), times g' (1 + g' 1), b2 v (1), the sum (1)                                 -> AW_N_V = 6
#   p: lr wd (1), 1 - . (1), p times it (1); lr / bc1 (2); m (4); times m (1); sqrt(v) (v's 6 halved = 3, the root
#      2), / bc2 (2), + eps (1); the quotient (2); the difference (1)                                      -> AW_N_P = 21
# bar = count x 2^-24 x the sum of the magnitudes of the terms: |b1 m| + |(1 - b1) g'| for m, b2 v + (1 - b2) g'^2
# for v, |p (1 - lr wd)| + (lr / bc1) (|b1 m| + |(1 - b1) g'|) / denom for p.
AW_N_M, AW_N_V, AW_N_P = 4, 6, 21


def adamw_ref64(p, g, m, v, hp, state):
    """One step in float64 on the hyperparameters as the kernel receives them -- float(lr), float(wd), float(beta),
    float(1 - beta) from the doubles, float(eps) -- and the device's own state (c, bc1, bc2): (p, m, v, bars)."""
    c, bc1, bc2 = (float(s) for s in state)
    lr, wd = aw_per_element([f32(x) for x in hp.lr]), aw_per_element([f32(x) for x in hp.wd])
    b1, b2, o1, o2, eps = f32(hp.b1), f32(hp.b2), f32(1.0 - hp.b1), f32(1.0 - hp.b2), f32(hp.eps)
    p, g, m, v = (t.double() for t in (p, g, m, v))
    gs = g * c
    p1 = p * (1.0 - lr * wd)
    m_terms = (b1 * m).abs() + (o1 * gs).abs()
    m2 = b1 * m + o1 * gs
    v2 = b2 * v + o2 * gs * gs
    denom = v2.sqrt() / bc2 + eps
    p2 = p1 - (lr / bc1) * m2 / denom
    bars = dict(m=AW_N_M * U32 * m_terms, v=AW_N_V * U32 * (b2 * v + o2 * gs * gs),
                p=AW_N_P * U32 * (p1.abs() + (lr / bc1) * m_terms / denom))
    return p2, m2, v2, bars


def adamw_f32(p, g, m, v, hp, state):
    """The same step op by op in numpy float32, each operation rounded on its own."""
    f = np.float32
    c, bc1, bc2 = (f(s) for s in state)
    lr = aw_per_element([f32(x) for x in hp.lr]).numpy().astype(f)
    wd = aw_per_element([f32(x) for x in hp.wd]).numpy().astype(f)
    b1, b2, o1, o2, eps = f(hp.b1), f(hp.b2), f(1.0 - hp.b1), f(1.0 - hp.b2), f(hp.eps)
    p, g, m, v = (t.numpy().astype(f) for t in (p, g, m, v))
    gs = g * c
    p1 = p * (f(1.0) - lr * wd)
    m2 = b1 * m + o1 * gs
    v2 = b2 * v + o2 * gs * gs
    denom = np.sqrt(v2) / bc2 + eps
    p2 = p1 - (lr / bc1) * m2 / denom
    return torch.from_numpy(p2), torch.from_numpy(m2), torch.from_numpy(v2)
