"""Training input: the reference's per-sample MixformerProcessing, as a host contract and on the device.

The reference prepares every training sample in DataLoader workers (lib/train/data/processing_rgbt.py:143-228
with the transform chain of lib/train/base_functions.py:177-183): a joint grayscale / flip of the full frames,
six sample_target crops (two templates and one search frame, two modalities each), a brightness jitter (the TIR
frame on uint8 before its JET map), a second flip of the crop and the ImageNet normalise.

draw_rolls                one sample's random numbers, from the reference's generators in the reference's order.
process_sample_reference  the contract: the whole pipeline on the host for one sample (numpy / torch on CPU).
crop_reference            one crop of it: what one mmt_train_crop_params entry computes.
TrainInputProcessor       the device form (csrc/train_input.hip: mmt_train_crops_table, two launches per batch);
                          the box arithmetic and the validity stay on the host, with the contract's functions.

cv2 is not part of this image: the resize, the colour conversions and the colour map restate OpenCV's published
8-bit arithmetic as oracle/preprocess.py does (tests compare the two), and are unpinned against cv2 itself.
"""
import ctypes
import math
import random
from dataclasses import dataclass

import numpy as np
import torch

from ._lib import LIB, TrainCropParams, check

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


# ------------------------------------------------------------------------------------------- configuration
@dataclass
class TrainInputConfig:
    """What MixformerProcessing and its transforms are built with (lib/train/base_functions.py:177-205)."""
    template_size: int = 128
    search_size: int = 320
    template_factor: float = 2.0
    search_factor: float = 5.0
    template_center_jitter: float = 0
    search_center_jitter: float = 4.5
    template_scale_jitter: float = 0
    search_scale_jitter: float = 0.5
    n_template: int = 2
    n_search: int = 1
    mean: tuple = MEAN
    std: tuple = STD
    brightness_jitter: float = 0.2   # ToTensorAndJitter(0.2)
    gray_p: float = 0.05             # ToGrayscale(probability=0.05)
    flip_p: float = 0.5              # RandomHorizontalFlip / RandomHorizontalFlip_Norm (probability=0.5)

    def draw(self):
        """draw_rolls with this configuration's frame counts and probabilities."""
        return draw_rolls(self.n_template, self.n_search, self.brightness_jitter, self.gray_p, self.flip_p)

    @classmethod
    def from_cfg(cls, cfg):
        """From a yacs-style config (cfg.DATA.TEMPLATE / cfg.DATA.SEARCH / cfg.DATA.MEAN / cfg.DATA.STD)."""
        t, s = cfg.DATA.TEMPLATE, cfg.DATA.SEARCH
        return cls(int(t.SIZE), int(s.SIZE), float(t.FACTOR), float(s.FACTOR), t.CENTER_JITTER, s.CENTER_JITTER,
                   t.SCALE_JITTER, s.SCALE_JITTER, int(getattr(t, "NUMBER", 1)), int(getattr(s, "NUMBER", 1)),
                   tuple(cfg.DATA.MEAN), tuple(cfg.DATA.STD))

    def group(self, name):
        """(frames, out_sz, factor, center_jitter, scale_jitter) of "template" or "search"."""
        if name == "template":
            return (self.n_template, self.template_size, self.template_factor, self.template_center_jitter,
                    self.template_scale_jitter)
        return (self.n_search, self.search_size, self.search_factor, self.search_center_jitter,
                self.search_scale_jitter)


def as_config(cfg_or_sizes):
    if isinstance(cfg_or_sizes, TrainInputConfig):
        return cfg_or_sizes
    if isinstance(cfg_or_sizes, (tuple, list)) and len(cfg_or_sizes) == 2:
        return TrainInputConfig(template_size=int(cfg_or_sizes[0]), search_size=int(cfg_or_sizes[1]))
    return TrainInputConfig.from_cfg(cfg_or_sizes)


GROUPS = ("template", "search")


# ------------------------------------------------------------------------------------------- random numbers
@dataclass
class Rolls:
    """One sample's random numbers.  Frames are ordered t0 .. t(N_t - 1), s0 .. s(N_s - 1)."""
    gray: bool
    joint_flip: bool
    crop_flip: tuple                 # per frame
    randn: np.ndarray                # (frames, 2) float32: torch.randn(2) of _get_jittered_box
    rand: np.ndarray                 # (frames, 2) float32: torch.rand(2)
    bf: tuple                        # per frame: RGB brightness factor (Python float)
    tf: tuple                        # per frame: TIR brightness factor


def draw_rolls(n_template=2, n_search=1, brightness_jitter=0.2, gray_p=0.05, flip_p=0.5):
    """The draws of one MixformerProcessing.__call__, in its order, from its three generators.
    random: ToGrayscale, RandomHorizontalFlip of the joint transform (once: the search group reuses the template
    group's rolls, new_roll=False), then RandomHorizontalFlip_Norm per frame.  torch: randn(2) then rand(2) per
    frame.  numpy.random: per frame the RGB factor then the TIR factor, both ToTensorAndJitter.roll() (the
    reference does not call roll_tir()).  A sample the reference rejects part-way stops drawing there; this
    always draws the whole sample.  The record holds the raw draws: the scale and centre jitter factors are applied
    by jitter_box from the configuration, so one record serves any of them."""
    n = n_template + n_search
    gray = random.random() < gray_p
    joint_flip = random.random() < flip_p
    lo, hi = max(0, 1 - brightness_jitter), 1 + brightness_jitter
    randn, rand, bf, tf, flips = [], [], [], [], []
    for _ in range(n):
        randn.append(torch.randn(2).numpy())
        rand.append(torch.rand(2).numpy())
        bf.append(float(np.random.uniform(lo, hi)))
        tf.append(float(np.random.uniform(lo, hi)))
        flips.append(random.random() < flip_p)
    return Rolls(gray, joint_flip, tuple(flips), np.stack(randn).astype(np.float32), np.stack(rand).astype(np.float32),
                 tuple(bf), tuple(tf))


# ------------------------------------------------------------------------------------------- pixel arithmetic
def rgb2gray(frame):
    """cv2.cvtColor(frame, COLOR_RGB2GRAY) (8-bit fixed point) replicated to three channels."""
    v = frame.astype(np.int64)
    g = ((v[..., 0] * 4899 + v[..., 1] * 9617 + v[..., 2] * 1868 + (1 << 13)) >> 14).astype(np.uint8)
    return np.stack([g, g, g], axis=2)


def jet_lut():
    """256 x 3 (B, G, R) uint8 JET table (the piecewise-linear jet formula, as oracle/preprocess.py:jet_lut)."""
    x = np.arange(256, dtype=np.float64) / 255.0
    r = np.clip(np.minimum(4 * x - 1.5, -4 * x + 4.5), 0, 1)
    g = np.clip(np.minimum(4 * x - 0.5, -4 * x + 3.5), 0, 1)
    b = np.clip(np.minimum(4 * x + 0.5, -4 * x + 2.5), 0, 1)
    lut = np.stack([b, g, r], 1).astype(np.float32) * np.float32(255.0)
    return np.clip(np.rint(lut), 0, 255).astype(np.uint8)


def apply_colormap(img, lut):
    """cv2.applyColorMap(img (H, W, 3) uint8): BGR2GRAY fixed point, then lut[gray][c]."""
    v = img.astype(np.int64)
    gray = (v[..., 0] * 1868 + v[..., 1] * 9617 + v[..., 2] * 4899 + (1 << 13)) >> 14
    return lut[gray]


def crop_geometry(box, factor):
    """(x1, y1, crop_sz) of sample_target (processing_utils.py:28-48; Python floats, round() half to even).
    crop_sz may be < 1: the callers decide."""
    x, y, w, h = [float(v) for v in box]
    crop_sz = math.ceil(math.sqrt(w * h) * factor)
    x1 = int(round(x + 0.5 * w - crop_sz * 0.5))
    y1 = int(round(y + 0.5 * h - crop_sz * 0.5))
    return x1, y1, crop_sz


def pad_flags(x1, y1, crop, H, W):
    """(rows, cols) bool (crop,): which rows / columns of the padded crop are padding, including the
    reference's x2_pad = max(x2 - W + 1, 0), which also drops the last image column / row."""
    xlim = W - 1 if x1 + crop >= W else W
    ylim = H - 1 if y1 + crop >= H else H
    ys, xs = np.arange(y1, y1 + crop), np.arange(x1, x1 + crop)
    return (ys < 0) | (ys >= ylim), (xs < 0) | (xs >= xlim)


def padded_crop(im, x1, y1, crop):
    """sample_target's crop with its constant-0 border, (crop, crop, 3) uint8."""
    H, W = im.shape[:2]
    rp, cp = pad_flags(x1, y1, crop, H, W)
    out = np.zeros((crop, crop, 3), dtype=np.uint8)
    if (~rp).any() and (~cp).any():
        ys, xs = np.arange(y1, y1 + crop)[~rp], np.arange(x1, x1 + crop)[~cp]
        out[np.ix_(~rp, ~cp)] = im[ys][:, xs]
    return out


def _is_area2(n, out_sz):
    scale = 1.0 / (float(out_sz) / n)
    return int(round(scale)) == 2 and abs(scale - 2) < 2.220446049250313e-16


def linear_taps(n, out_sz, edge):
    """(s0, s1, f) per output coordinate of cv2.resize's linear path, n -> out_sz: taps s0 and s1 with weights
    1 - f and f (float32).  edge=True is the column rule (a tap past either end takes the whole weight),
    edge=False the row rule (weights kept, indices clamped)."""
    scale = 1.0 / (float(out_sz) / n)
    d = np.arange(out_sz)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if not edge:
        return np.clip(s, 0, n - 1), np.clip(s + 1, 0, n - 1), f
    f = np.where(s < 0, np.float32(0), f)
    s = np.where(s < 0, 0, s)
    last = s >= n - 1
    f = np.where(last, np.float32(0), f).astype(np.float32)
    s = np.where(last, n - 1, s)
    return s, np.minimum(s + 1, n - 1), f


def _coef(v):
    return np.clip(np.rint(np.float32(v) * np.float32(2048.0)), -32768, 32767).astype(np.int64)


def resize_linear_u8(img, out_sz):
    """cv2.resize(img, (out_sz, out_sz)) of a square (n, n, 3) uint8 image: 11-bit fixed-point INTER_LINEAR, and
    INTER_AREA's (a + b + c + d + 2) >> 2 at an exact 2x downscale."""
    n = img.shape[0]
    src = img.astype(np.int64)
    if _is_area2(n, out_sz):
        d = np.arange(out_sz)
        a = src[2 * d][:, 2 * d] + src[2 * d][:, 2 * d + 1] + src[2 * d + 1][:, 2 * d] + src[2 * d + 1][:, 2 * d + 1]
        return ((a + 2) >> 2).astype(np.uint8)
    sx, sx1, fx = linear_taps(n, out_sz, True)
    r0, r1, fy = linear_taps(n, out_sz, False)
    a0, a1, b0, b1 = _coef(np.float32(1) - fx), _coef(fx), _coef(np.float32(1) - fy), _coef(fy)
    hrow = src[:, sx, :] * a0[None, :, None] + src[:, sx1, :] * a1[None, :, None]
    t = (((hrow[r0] >> 4) * b0[:, None, None]) >> 16) + (((hrow[r1] >> 4) * b1[:, None, None]) >> 16)
    return np.clip((t + 2) >> 2, 0, 255).astype(np.uint8)


def resize_linear_f64(m, out_sz):
    """cv2.resize of a square (n, n) float64 image: the same taps with float32 weights 1 - f and f, products and
    sums in float64; the 4-pixel mean at an exact 2x downscale."""
    n = m.shape[0]
    if _is_area2(n, out_sz):
        d = np.arange(out_sz)
        return (m[2 * d][:, 2 * d] + m[2 * d][:, 2 * d + 1] + m[2 * d + 1][:, 2 * d] + m[2 * d + 1][:, 2 * d + 1]) * 0.25
    sx, sx1, fx = linear_taps(n, out_sz, True)
    r0, r1, fy = linear_taps(n, out_sz, False)
    a0, a1 = (np.float32(1) - fx).astype(np.float64), fx.astype(np.float64)
    b0, b1 = (np.float32(1) - fy).astype(np.float64), fy.astype(np.float64)
    hrow = m[:, sx] * a0[None, :] + m[:, sx1] * a1[None, :]
    return hrow[r0] * b0[:, None] + hrow[r1] * b1[:, None]


def att_mask(x1, y1, crop, H, W, out_sz):
    """sample_target's attention mask: ones on the padding, cv2.resize, astype(bool) -- (out_sz, out_sz) bool."""
    rp, cp = pad_flags(x1, y1, crop, H, W)
    m = (rp[:, None] | cp[None, :]).astype(np.float64)
    return resize_linear_f64(m, out_sz) != 0


def att_rows_cols(x1, y1, crop, H, W, out_sz):
    """(rows, cols) bool (out_sz,) with att_mask == rows[:, None] | cols[None, :].  The padding mask is rows OR
    columns and every weight is >= 0, so a resized value is non-zero iff a tap of non-zero weight is padding;
    the first tap's weight 1 - f is never 0, the second's is f."""
    rp, cp = pad_flags(x1, y1, crop, H, W)
    if _is_area2(crop, out_sz):
        d = np.arange(out_sz)
        return rp[2 * d] | rp[2 * d + 1], cp[2 * d] | cp[2 * d + 1]
    sx, sx1, fx = linear_taps(crop, out_sz, True)
    r0, r1, fy = linear_taps(crop, out_sz, False)
    return rp[r0] | ((fy != 0) & rp[r1]), cp[sx] | ((fx != 0) & cp[sx1])


def mask_check_points(out_sz):
    """The rows / columns F.interpolate(mask[None, None].float(), size=out_sz // 16) (nearest) picks: 16 i for the
    sizes in use (multiples of 16)."""
    fs = out_sz // 16
    idx = np.floor(np.arange(fs, dtype=np.float32) * np.float32(out_sz / fs)).astype(np.int64)
    return np.minimum(idx, out_sz - 1)


def crop_is_valid(box, factor, H, W, out_sz, out_flip):
    """The reference's two validity conditions for one RGB crop, from the geometry alone: crop_sz >= 1, and the
    attention mask (flipped with the crop) not all-True at the points its 16x down-sampling picks.  With
    att = rows | cols, it is all-True there iff rows is all-True there or cols is.  (The reference's first check,
    the whole mask all-True, is implied.)"""
    x1, y1, crop = crop_geometry(box, factor)
    if crop < 1:
        return False
    rows, cols = att_rows_cols(x1, y1, crop, H, W, out_sz)
    if out_flip:
        cols = cols[::-1]
    p = mask_check_points(out_sz)
    return not (rows[p].all() or cols[p].all())


def crop_reference(image, box, factor, out_sz, lut=None, mean=MEAN, std=STD, gain=1.0 / 255.0, src_flip=False,
                   src_gray=False, out_flip=False):
    """What one mmt_train_crop_params entry computes, by the reference's steps on the host: the joint grayscale /
    flip of the whole frame, sample_target, the brightness jitter, the crop's flip, the normalise.
    Returns (out (3, s, s) float32, att (s, s) bool, patch (s, s, 3) uint8, crop record (4,) float64).
    A crop_sz < 1 (the reference raises) gives zero pixels and an all-True mask, as the kernel does."""
    frame = np.asarray(image)
    H, W = frame.shape[:2]
    if src_gray:
        frame = rgb2gray(frame)
    if src_flip:
        frame = np.fliplr(frame).copy()
    x1, y1, crop = crop_geometry(box, factor)
    if crop >= 1:
        patch = resize_linear_u8(padded_crop(frame, x1, y1, crop), out_sz)
        att = att_mask(x1, y1, crop, H, W, out_sz)
        rf = out_sz / crop
    else:
        patch = np.zeros((out_sz, out_sz, 3), np.uint8)
        att = np.ones((out_sz, out_sz), bool)
        rf = math.inf
    if lut is None:  # ToTensorAndJitter.transform_image, RGB: x.float().mul(bf / 255.0).clamp(0.0, 1.0)
        x = torch.from_numpy(patch.transpose((2, 0, 1)).copy()).float().mul(float(gain)).clamp(0.0, 1.0)
    else:            # TIR: jitter on uint8, JET, then x.float().div(255.0).clamp(0.0, 1.0)
        jit = (patch * float(gain)).clip(0.0, 255.0).astype(np.uint8)
        x = torch.from_numpy(apply_colormap(jit, lut).transpose((2, 0, 1)).copy()).float().div(255.0).clamp(0.0, 1.0)
    att = torch.from_numpy(att)
    if out_flip:
        x, att, patch = x.flip((2,)), att.flip((-1,)), np.fliplr(patch).copy()
    m = torch.tensor(mean, dtype=torch.float32)[:, None, None]
    s = torch.tensor(std, dtype=torch.float32)[:, None, None]
    out = (x - m) / s
    return out.numpy(), att.numpy(), patch, np.array([x1, y1, crop, rf], dtype=np.float64)


# ------------------------------------------------------------------------------------------- box arithmetic
def _corner_box(box, fx):
    """TransformBase._transform_bbox_single_: the box through its four corners (float32), fx applied to the x
    coordinates; the result is (min, max - min) per axis, whether anything was flipped or not."""
    x, y, w, h = box[0], box[1], box[2], box[3]
    x2, y2 = x + w, y + h
    xs = fx(torch.stack([x, x2, x2, x]))
    ys = torch.stack([y, y, y2, y2])
    tl = torch.stack([xs.min(), ys.min()])
    return torch.cat((tl, torch.stack([xs.max(), ys.max()]) - tl))


def joint_box(box, W0, flip):
    """RandomHorizontalFlip.transform_bbox of the joint transform: W0 is the width of the group's first RGB frame."""
    return _corner_box(box, (lambda xs: (W0 - 1) - xs) if flip else (lambda xs: xs))


def crop_flip_box(box, flip):
    """RandomHorizontalFlip_Norm.transform_bbox on the normalised label box."""
    return _corner_box(box, (lambda xs: 1 - xs) if flip else (lambda xs: xs))


def jitter_box(box, randn, rand, scale_jitter, center_jitter):
    """MixformerProcessing._get_jittered_box / _get_jittered_bbox_single_ (float32)."""
    scale = torch.exp(torch.as_tensor(randn) * scale_jitter)
    offset = torch.as_tensor(rand) - 0.5
    size = box[2:4] * scale
    max_offset = size.prod().sqrt() * torch.tensor(center_jitter).float()
    center = box[0:2] + 0.5 * box[2:4] + max_offset * offset
    return torch.cat((center - 0.5 * size, size), dim=0)


def label_box(box_in, box_extract, resize_factor, out_sz):
    """processing_utils.transform_image_to_crop(..., normalize=True): resize_factor a Python float."""
    crop_sz = torch.Tensor([out_sz, out_sz])
    c_ex = box_extract[0:2] + 0.5 * box_extract[2:4]
    c_in = box_in[0:2] + 0.5 * box_in[2:4]
    c_out = (crop_sz - 1) / 2 + (c_in - c_ex) * resize_factor
    wh = box_in[2:4] * resize_factor
    return torch.cat((c_out - 0.5 * wh, wh)) / crop_sz[0]


def _f32box(a):
    t = torch.as_tensor(np.asarray(a, dtype=np.float32).reshape(4).copy())
    return t


@dataclass
class FramePlan:
    """The host's part of one frame pair: everything the crops and labels need that is not a pixel."""
    group: str
    index: int
    H: int
    W: int
    box: list                        # the jittered RGB box, Python floats (both modalities are cropped with it)
    factor: float
    out_sz: int
    src_flip: bool
    src_gray: bool
    out_flip: bool
    bf: float
    tf: float
    crop_sz: int
    valid: bool
    anno_v: torch.Tensor = None      # (4,) float32 labels, set when crop_sz >= 1
    anno_i: torch.Tensor = None


def plan_sample(frames, annos, rolls, cfg):
    """(plans, valid): the box arithmetic and the validity of one sample, on the host, before any pixel is read.
    frames / annos: {"template": [[rgb, tir], ...], "search": [[rgb, tir], ...]}; only the frames' shapes are
    used.  valid is the reference's data["valid"]."""
    plans, k, valid = [], 0, True
    for g in GROUPS:
        n, out_sz, factor, cj, sj = cfg.group(g)
        if len(frames[g]) != n or len(annos[g]) != n:
            raise ValueError("%s: %d frame pairs expected, got %d frames and %d annos" % (g, n, len(frames[g]), len(annos[g])))
        W0 = frames[g][0][0].shape[1]
        for f in range(n):
            rgb, tir = frames[g][f]
            H, W = rgb.shape[:2]
            if tuple(tir.shape[:2]) != (H, W):
                raise ValueError("%s frame %d: the RGB and TIR frames differ in size: %s and %s"
                                 % (g, f, tuple(rgb.shape), tuple(tir.shape)))
            box_v = joint_box(_f32box(annos[g][f][0]), W0, rolls.joint_flip)
            box_i = joint_box(_f32box(annos[g][f][1]), W0, rolls.joint_flip)
            jit = jitter_box(box_v, rolls.randn[k], rolls.rand[k], sj, cj)
            # the reference's own size check, in float32 as it computes it
            small = bool((torch.ceil(torch.sqrt(jit[2] * jit[3]) * factor) < 1).item())
            box = jit.tolist()
            crop_sz = 0 if small else crop_geometry(box, factor)[2]
            ok = (not small) and crop_sz >= 1 and crop_is_valid(box, factor, H, W, out_sz, rolls.crop_flip[k])
            p = FramePlan(g, f, H, W, box, float(factor), out_sz, rolls.joint_flip, rolls.gray, rolls.crop_flip[k],
                          rolls.bf[k], rolls.tf[k], crop_sz, ok)
            if crop_sz >= 1:
                rf = out_sz / crop_sz
                p.anno_v = crop_flip_box(label_box(box_v, jit, rf, out_sz), rolls.crop_flip[k])
                p.anno_i = crop_flip_box(label_box(box_i, jit, rf, out_sz), rolls.crop_flip[k])
            valid = valid and ok
            plans.append(p)
            k += 1
    return plans, valid


def process_sample_reference(frames, annos, rolls, cfg):
    """The contract: MixformerProcessing.__call__ (mode "sequence") on one sample, on the host.
    frames: {"template": [[rgb, tir]] * N_t, "search": [[rgb, tir]] * N_s}, (H, W, 3) uint8 arrays of any sizes;
    annos: the same layout of (4,) float32 boxes (x, y, w, h).  Returns the fields the actor reads, stacked:
    template_images_v / _i (N_t, 3, s, s) float32, search_images_v / _i, template_anno_v / _i (N_t, 4),
    search_anno_v / _i, template_att_v / _i (N_t, s, s) bool, search_att_v / _i, and valid.  An invalid sample
    has valid alone, as the reference returns early."""
    cfg = as_config(cfg)
    check_sample(frames, annos)
    plans, valid = plan_sample(frames, annos, rolls, cfg)
    if not valid:
        return {"valid": False}
    lut = jet_lut()
    out = {}
    for g in GROUPS:
        acc = {k: [] for k in ("images_v", "images_i", "anno_v", "anno_i", "att_v", "att_i")}
        for p in (q for q in plans if q.group == g):
            rgb, tir = frames[g][p.index]
            common = dict(mean=cfg.mean, std=cfg.std, src_flip=p.src_flip, out_flip=p.out_flip)
            xv, av, _, _ = crop_reference(rgb, p.box, p.factor, p.out_sz, None, gain=p.bf / 255.0, src_gray=p.src_gray,
                                          **common)
            xi, ai, _, _ = crop_reference(tir, p.box, p.factor, p.out_sz, lut, gain=p.tf, **common)
            for k, v in (("images_v", xv), ("images_i", xi), ("att_v", av), ("att_i", ai)):
                acc[k].append(torch.from_numpy(v))
            acc["anno_v"].append(p.anno_v)
            acc["anno_i"].append(p.anno_i)
        for k, v in acc.items():
            out["%s_%s" % (g, k)] = torch.stack(v)
    out["valid"] = True
    return out


def check_frame(x, what):
    if not isinstance(x, np.ndarray) or x.dtype != np.uint8:
        raise ValueError("%s must be a uint8 numpy array, got %s" % (what, getattr(x, "dtype", type(x).__name__)))
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError("%s must be (H, W, 3), got shape %s" % (what, tuple(x.shape)))
    if x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("%s must not be empty, got shape %s" % (what, tuple(x.shape)))


def check_sample(frames, annos):
    for g in GROUPS:
        for f, pair in enumerate(frames[g]):
            if len(pair) != 2:
                raise ValueError("%s frame %d: an [rgb, tir] pair expected" % (g, f))
            check_frame(pair[0], "%s frame %d (RGB)" % (g, f))
            check_frame(pair[1], "%s frame %d (TIR)" % (g, f))
        for f, pair in enumerate(annos[g]):
            if len(pair) != 2 or any(np.asarray(b).size != 4 for b in pair):
                raise ValueError("%s anno %d: an [rgb, tir] pair of (4,) boxes expected" % (g, f))


# ------------------------------------------------------------------------------------------- the device form
def crop_params(image, H, W, box, factor, out_sz, lut, mean, std, gain, src_flip=False, src_gray=False, out_flip=False,
                out=None, att=None, patch=None, crop=None):
    """One mmt_train_crop_params from device addresses (ints; None or 0 for NULL)."""
    p = TrainCropParams()
    p.image, p.H, p.W, p.box, p.factor, p.out_sz, p.lut = image or None, H, W, box or None, factor, out_sz, lut or None
    for c in range(3):
        p.mean[c], p.std[c] = mean[c], std[c]
    p.gain = gain
    p.src_flip, p.src_gray, p.out_flip = int(bool(src_flip)), int(bool(src_gray)), int(bool(out_flip))
    p.out, p.att, p.patch, p.crop = out or None, att or None, patch or None, crop or None
    return p


def table_tensor(entries, device):
    """A list of TrainCropParams as a device byte tensor (8-byte aligned, as every torch allocation is)."""
    arr = (TrainCropParams * len(entries))(*entries)
    host = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy())
    return host.to(device)


def launch_train_crops(table, enable, n, out_sz, stream=None):
    """mmt_train_crops_table on the current stream: table a device byte tensor of n entries, enable None or n
    device bytes."""
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    check(LIB.mmt_train_crops_table(table.data_ptr(), enable.data_ptr() if enable is not None else None, n, out_sz, s),
          "mmt_train_crops_table")


def check_batch(samples, rolls, batch):
    if len(samples) != batch:
        raise ValueError("batch mismatch: the processor was built for %d samples, got %d" % (batch, len(samples)))
    if rolls is not None and len(rolls) != batch:
        raise ValueError("batch mismatch: %d samples, %d rolls" % (batch, len(rolls)))


ENTRY_BYTES = ctypes.sizeof(TrainCropParams)
FILL = float("nan")


class TrainInputProcessor:
    """B raw samples -> the actor's batch, on the device.  Owns persistent buffers (pinned and device frame
    staging, the two descriptor tables, the outputs), so the returned tensors are the same storage on every
    call: a captured training step can read them in place.  Frames of any sizes; the staging grows when a batch
    needs more.  Rows of an invalid sample are not written (they keep the NaN / all-True fill of construction, or
    the previous batch's contents): the caller drops or refills them."""

    def __init__(self, cfg_or_sizes, batch, device="cuda", frame_hw=(480, 640)):
        self.cfg = cfg = as_config(cfg_or_sizes)
        if batch < 1:
            raise ValueError("batch must be >= 1, got %r" % (batch,))
        self.B = B = int(batch)
        self.device = dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("TrainInputProcessor runs on the GPU (process_sample_reference is the host form)")
        self.n_frames = cfg.n_template + cfg.n_search
        self.out, self._att8 = {}, {}
        for g in GROUPS:
            n, s = cfg.group(g)[:2]
            if s % 16:
                raise ValueError("%s size must be a multiple of 16 (the backbone stride), got %d" % (g, s))
            for m in "vi":
                self.out["%s_images_%s" % (g, m)] = torch.full((n, B, 3, s, s), FILL, device=dev)
                self.out["%s_anno_%s" % (g, m)] = torch.full((n, B, 4), FILL, device=dev)
                self._att8["%s_att_%s" % (g, m)] = a = torch.ones((n, B, s, s), device=dev, dtype=torch.uint8)
                self.out["%s_att_%s" % (g, m)] = a.view(torch.bool)
        self.out["valid"] = torch.zeros(B, device=dev, dtype=torch.bool)
        self.crop = {g: torch.zeros((cfg.group(g)[0], B, 2, 4), device=dev, dtype=torch.float64) for g in GROUPS}
        self.lut = torch.from_numpy(jet_lut()).to(dev)
        self.n_entries = {g: 2 * cfg.group(g)[0] * B for g in GROUPS}
        self._tab_host = {g: torch.zeros(self.n_entries[g] * ENTRY_BYTES, dtype=torch.uint8).pin_memory() for g in GROUPS}
        self.table = {g: torch.zeros(self.n_entries[g] * ENTRY_BYTES, device=dev, dtype=torch.uint8) for g in GROUPS}
        self._en_host = {g: torch.zeros(self.n_entries[g], dtype=torch.uint8).pin_memory() for g in GROUPS}
        self.enable = {g: torch.zeros(self.n_entries[g], device=dev, dtype=torch.uint8) for g in GROUPS}
        self._box_host = torch.zeros((B * self.n_frames, 4), dtype=torch.float64).pin_memory()
        self.box = torch.zeros((B * self.n_frames, 4), device=dev, dtype=torch.float64)
        self._anno_host = {k: torch.full(tuple(v.shape), FILL).pin_memory() for k, v in self.out.items() if "_anno_" in k}
        self._valid_host = torch.zeros(B, dtype=torch.bool).pin_memory()
        self._frames_host = self._frames = None
        self._reserve(B * self.n_frames * 2 * int(frame_hw[0]) * int(frame_hw[1]) * 3)
        self._uploaded = torch.cuda.Event()
        self._busy = False

    def _reserve(self, nbytes):
        if self._frames is None or self._frames.numel() < nbytes:
            self._frames_host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
            self._frames = torch.empty(nbytes, device=self.device, dtype=torch.uint8)

    def process_batch(self, samples, rolls=None):
        """samples: B of (frames, annos) as process_sample_reference takes them; rolls: None (drawn here, one
        draw_rolls per sample in order) or B Rolls.  Returns the actor's dict with a leading batch axis:
        template_images_v (N_t, B, 3, s, s) and so on, and valid (B,).  Work is queued on the current stream."""
        cfg, B = self.cfg, self.B
        check_batch(samples, rolls, B)
        if rolls is None:
            rolls = [cfg.draw() for _ in range(B)]
        plans = []
        for (frames, annos), r in zip(samples, rolls):
            check_sample(frames, annos)
            plans.append(plan_sample(frames, annos, r, cfg))
        total = sum(2 * p.H * p.W * 3 for ps, ok in plans if ok for p in ps)
        if self._busy:
            self._uploaded.synchronize()  # the pinned staging is about to be overwritten
        self._reserve(total)
        stage = self._frames_host.numpy()
        base = self._frames.data_ptr()
        off = 0
        tabs = {g: (TrainCropParams * self.n_entries[g])() for g in GROUPS}
        for g in GROUPS:
            self._en_host[g].zero_()
        for b, ((frames, annos), (ps, ok)) in enumerate(zip(samples, plans)):
            self._valid_host[b] = bool(ok)
            if not ok:
                continue
            for k, p in enumerate(ps):
                self._box_host[b * self.n_frames + k] = torch.tensor(p.box, dtype=torch.float64)
                box_ptr = self.box.data_ptr() + (b * self.n_frames + k) * 32
                for m, name in enumerate("vi"):
                    img = frames[p.group][p.index][m]
                    n = img.size
                    stage[off:off + n] = img.reshape(-1)
                    e = (b * cfg.group(p.group)[0] + p.index) * 2 + m
                    tabs[p.group][e] = crop_params(
                        base + off, p.H, p.W, box_ptr, p.factor, p.out_sz, self.lut.data_ptr() if m else None, cfg.mean,
                        cfg.std, p.tf if m else p.bf / 255.0, p.src_flip, p.src_gray and not m, p.out_flip,
                        out=self.out["%s_images_%s" % (p.group, name)][p.index, b].data_ptr(),
                        att=self._att8["%s_att_%s" % (p.group, name)][p.index, b].data_ptr(),
                        crop=self.crop[p.group][p.index, b, m].data_ptr())
                    self._en_host[p.group][e] = 1
                    off += n
                    self._anno_host["%s_anno_%s" % (p.group, name)][p.index, b] = p.anno_i if m else p.anno_v
        if off:
            self._frames[:off].copy_(self._frames_host[:off], non_blocking=True)
        self.box.copy_(self._box_host, non_blocking=True)
        for g in GROUPS:
            ctypes.memmove(self._tab_host[g].data_ptr(), tabs[g], self.n_entries[g] * ENTRY_BYTES)
            self.table[g].copy_(self._tab_host[g], non_blocking=True)
            self.enable[g].copy_(self._en_host[g], non_blocking=True)
        for k, h in self._anno_host.items():
            self.out[k].copy_(h, non_blocking=True)
        self.out["valid"].copy_(self._valid_host, non_blocking=True)
        self._uploaded.record()
        self._busy = True
        self.launch()
        return self.out

    def launch(self):
        """The two launches alone, on the tables and frames as last uploaded."""
        for g in GROUPS:
            torch.ops.mmt.train_crops(self.table[g], self.enable[g], self.cfg.group(g)[1],
                                      self.out["%s_images_v" % g], self.out["%s_images_i" % g],
                                      self._att8["%s_att_v" % g], self._att8["%s_att_i" % g], self.crop[g])


from . import ops  # noqa: E402,F401  (registers torch.ops.mmt.train_crops)
