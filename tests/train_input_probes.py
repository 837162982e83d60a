"""Shared by the training-input tests: the fixture of tests/golden/train_input.npz (the reference's own
MixformerProcessing on seeded samples, tests/golden/make_golden_train_input.py) and the probe entries the
kernel is compared on.  No GPU here."""
import functools
import hashlib
import os
import random

import numpy as np
import torch

from conftest import GOLDEN

N_FRAMES = 3  # t0, t1, s0


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(GOLDEN, "train_input.npz")))


def fixture_config(i):
    from mmt_amd.train_input import TrainInputConfig
    fx = fixture()
    t, s = fx["sizes"][int(fx["s%d_config" % i])]
    return TrainInputConfig(template_size=int(t), search_size=int(s))


def fixture_sample(i):
    """(frames, annos) of fixture sample i, as process_sample_reference takes them."""
    fx = fixture()
    frames = [[fx["frame_%d_v" % k], fx["frame_%d_i" % k]] for k in range(N_FRAMES)]
    annos = [[fx["s%d_annos" % i][k, m] for m in range(2)] for k in range(N_FRAMES)]
    return {"template": frames[:2], "search": frames[2:]}, {"template": annos[:2], "search": annos[2:]}


def seeded_rolls(seed):
    from mmt_amd.train_input import draw_rolls
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    return draw_rolls()


def fixture_rolls(i):
    return seeded_rolls(int(fixture()["s%d_seed" % i]))


def samples_of(config_name):
    fx = fixture()
    c = list(fx["config_names"]).index(config_name)
    return [i for i in range(int(fx["n_samples"])) if int(fx["s%d_config" % i]) == c]


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


@functools.lru_cache(maxsize=None)
def contract(i):
    """process_sample_reference of fixture sample i, computed once and shared (do not modify)."""
    from mmt_amd.train_input import process_sample_reference
    frames, annos = fixture_sample(i)
    return process_sample_reference(frames, annos, fixture_rolls(i), fixture_config(i))


# ------------------------------------------------------------------ kernel probe entries
def probe_frame(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _entry(frame, box, factor, out_sz, tir=False, gain=None, src_flip=False, src_gray=False, out_flip=False):
    if gain is None:
        gain = 1.0 if tir else 1.0 / 255.0
    return dict(frame=frame, box=[float(v) for v in box], factor=float(factor), out_sz=out_sz, tir=tir, gain=float(gain),
                src_flip=src_flip, src_gray=src_gray, out_flip=out_flip)


# frames: a single pixel, odd x odd, even x even
FRAME_SHAPES = {"1x1": (1, 1), "23x37": (23, 37), "38x54": (38, 54)}

# (x, y, w, h) with factor 2: crop_sz = ceil(sqrt(w * h) * 2)
GEOMETRIES = {
    # name: (frame, box, factor)
    "inside_frac": ("38x54", [20.3, 12.7, 11.0, 9.5], 2.0),          # crop 21: fractional down-scale to 16
    "area2_16": ("38x54", [18.0, 10.0, 16.0, 16.0], 2.0),            # crop 32 = 2 * 16 exactly
    "area2_32": ("38x54", [-3.0, -13.0, 32.0, 32.0], 2.0),           # crop 64 = 2 * 32, across all four edges
    "up": ("23x37", [15.0, 9.0, 4.0, 5.0], 2.0),                     # crop 9: up-scale
    "left": ("23x37", [-2.0, 8.0, 8.0, 6.0], 2.0),
    "right": ("23x37", [31.0, 8.0, 8.0, 6.0], 2.0),
    "right_touch": ("23x37", [27.0, 8.0, 5.0, 5.0], 2.0),            # x2 == W exactly: the dropped last column
    "top": ("38x54", [20.0, -3.0, 7.0, 9.0], 2.0),
    "bottom": ("38x54", [20.0, 31.0, 7.0, 9.0], 2.0),
    "corner_tl": ("23x37", [-3.0, -2.0, 9.0, 7.0], 2.0),
    "corner_br": ("23x37", [30.0, 17.0, 9.0, 7.0], 2.0),
    "corner_tr": ("38x54", [49.0, -4.0, 9.0, 9.0], 2.0),
    "corner_bl": ("38x54", [-4.0, 33.0, 9.0, 9.0], 2.0),
    "outside": ("23x37", [80.0, 60.0, 6.0, 6.0], 2.0),               # entirely outside the frame: all padding
    "pixel": ("1x1", [-2.0, -3.0, 3.0, 4.0], 2.0),
    "pixel_big": ("1x1", [-20.0, -19.0, 40.0, 41.0], 2.0),
    "cover": ("23x37", [3.0, -2.0, 30.0, 26.0], 5.0),                # the search form: a crop much larger than the frame
    "tiny": ("38x54", [20.0, 20.0, 0.0, 3.0], 2.0),                  # crop_sz 0: zero pixels, att 1
}

# RGB gains: bf / 255 with bf below, at and past 1 (the upper clamp), and 0 (the lower)
RGB_GAINS = [1.0 / 255.0, 0.8 / 255.0, 1.2 / 255.0, 0.0, 2.0]
# TIR gains: v * tf an exact integer (1, 0.5, 2), just below one (0.999999...), past 255 (1.2, 300), 0
TIR_GAINS = [1.0, 0.5, 2.0, float(np.nextafter(1.0, 0.0)), 1.2, 0.8125, 300.0, 0.0]


@functools.lru_cache(maxsize=None)
def probe_entries(out_sz):
    """The entries of one launch at out_sz: every geometry in RGB and TIR form, all eight flag combinations on
    frames of odd and even width, and every gain."""
    frames = {k: probe_frame(h, w, 3 + i) for i, (k, (h, w)) in enumerate(FRAME_SHAPES.items())}
    out = []
    for name, (fk, box, factor) in GEOMETRIES.items():
        for tir in (False, True):
            out.append(("%s_%s" % (name, "tir" if tir else "rgb"), _entry(frames[fk], box, factor, out_sz, tir)))
    for fk, box in (("23x37", [28.0, 14.0, 9.0, 8.0]), ("38x54", [44.0, 3.0, 9.0, 8.0]), ("38x54", [18.0, 10.0, 16.0, 16.0]),
                    ("38x54", [10.0, 3.0, 32.0, 32.0])):  # the last two: the exact 2x at out_sz 16 and at 32
        for flags in range(8):
            sf, sg, of = bool(flags & 1), bool(flags & 2), bool(flags & 4)
            for tir in (False, True):
                out.append(("flags%d_%s_%s_%d" % (flags, fk, "tir" if tir else "rgb", int(box[2])),
                            _entry(frames[fk], box, 2.0, out_sz, tir, None, sf, sg, of)))
    for g in RGB_GAINS:
        out.append(("rgb_gain_%r" % g, _entry(frames["38x54"], [20.3, 12.7, 11.0, 9.5], 2.0, out_sz, False, g)))
    for g in TIR_GAINS:
        out.append(("tir_gain_%r" % g, _entry(frames["38x54"], [20.3, 12.7, 11.0, 9.5], 2.0, out_sz, True, g, True, False, True)))
    return out


@functools.lru_cache(maxsize=None)
def probe_reference(out_sz):
    """crop_reference of every probe entry at out_sz, computed once and shared (do not modify)."""
    from mmt_amd.train_input import MEAN, STD, crop_reference, jet_lut
    lut = jet_lut()
    return [crop_reference(e["frame"], e["box"], e["factor"], e["out_sz"], lut if e["tir"] else None, MEAN, STD, e["gain"],
                           e["src_flip"], e["src_gray"], e["out_flip"]) for _, e in probe_entries(out_sz)]
