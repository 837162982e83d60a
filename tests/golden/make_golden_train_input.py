"""Golden vectors for the training input, from the REFERENCE's own MixformerProcessing (CPU).

Run here only (the reference tree does not exist on the GPU box; libmmt_hip.so must be built, since the sample
search below imports mmt_amd.train_input):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_train_input.py

The reference's lib/train/data/processing_rgbt.py, transforms_rgbt.py and processing_utils.py are loaded by path
under the stub recipe of make_golden_tracker.py, and MixformerProcessing (mode "sequence") is built with the
transform chain of lib/train/base_functions.py:177-183.  cv2 and torchvision are absent from this image, so
  cv2.copyMakeBorder      the exact numpy constant pad (as make_golden_tracker.py),
  cv2.resize              uint8: oracle/preprocess.py resize_linear_u8; the float64 attention mask: the same taps
                          with float weights (mmt_amd.train_input.resize_linear_f64; the oracle has no float form),
  cv2.applyColorMap       oracle/preprocess.py apply_colormap + jet_lut,
  cv2.cvtColor RGB2GRAY   OpenCV's 8-bit fixed point (R*4899 + G*9617 + B*1868 + 8192) >> 14,
  tvisf.normalize         (x - mean) / std in float32, as torchvision computes it
stay PARITY UNPINNED against cv2 itself, as oracle/preprocess.py says.  Everything else -- the order of the random
draws, the box arithmetic, the jitter, the order of flips / jitter / colour map, the clamps, the validity checks --
is the reference's own code.

Recorded (tests/golden/train_input.npz): the frames, per sample its configuration, annos, seed, the values the
reference drew from each generator, valid, and for valid samples every output box in full, a SHA-256 digest of
every image and attention mask, and the whole image at output sizes <= 32.
Nothing is written under /root/reference (sys.dont_write_bytecode).
"""
import hashlib
import importlib.util
import os
import random
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden  # noqa: E402  (stub recipe; inserts the reference into sys.path)
from oracle import preprocess as opre  # noqa: E402
from mmt_amd import train_input as ti  # noqa: E402

CONFIGS = {  # name: (template size, search size); factors and jitters are the reference's defaults
    "small": ti.TrainInputConfig(template_size=32, search_size=64),
    "real": ti.TrainInputConfig(template_size=128, search_size=320),
}
CONFIG_NAMES = list(CONFIGS)
FRAME_SHAPES = [(72, 96), (64, 80), (72, 96)]  # t0, t1, s0: the group's frames need not agree in size


# ------------------------------------------------------------------------------------------- stubs
def _copy_make_border(img, top, bottom, left, right, border_type, value=None):
    assert border_type == 0
    return np.pad(img, ((top, bottom), (left, right)) + ((0, 0),) * (img.ndim - 2), mode="constant")


def _resize(img, size):
    assert size[0] == size[1] and img.shape[0] == img.shape[1], (img.shape, size)
    if img.dtype == np.uint8:
        return opre.resize_linear_u8(img, size[0])
    assert img.dtype == np.float64 and img.ndim == 2
    return ti.resize_linear_f64(img, size[0])


def _apply_color_map(img, cmap):
    assert cmap == 2 and img.dtype == np.uint8
    return opre.apply_colormap(img, opre.jet_lut())


def _cvt_color(img, code):
    assert code == 7 and img.dtype == np.uint8
    v = img.astype(np.int64)
    return ((v[..., 0] * 4899 + v[..., 1] * 9617 + v[..., 2] * 1868 + (1 << 13)) >> 14).astype(np.uint8)


def _normalize(tensor, mean, std, inplace=False):
    m = torch.as_tensor(mean, dtype=tensor.dtype)[:, None, None]
    s = torch.as_tensor(std, dtype=tensor.dtype)[:, None, None]
    return (tensor - m) / s


def _load(name):
    path = os.path.join(make_golden.REF, *name.split(".")) + ".py"
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def install():
    make_golden.install_stubs()
    cv = types.ModuleType("cv2")
    cv.BORDER_CONSTANT, cv.COLORMAP_JET, cv.COLOR_RGB2GRAY, cv.COLOR_RGB2BGR = 0, 2, 7, 4
    cv.copyMakeBorder, cv.resize, cv.applyColorMap, cv.cvtColor = _copy_make_border, _resize, _apply_color_map, _cvt_color
    sys.modules["cv2"] = cv
    tv = sys.modules["torchvision"]
    tv.transforms = types.ModuleType("torchvision.transforms")
    tv.transforms.ToTensor = type("ToTensor", (), {})
    tv.transforms.functional = types.ModuleType("torchvision.transforms.functional")
    tv.transforms.functional.normalize = _normalize
    sys.modules["torchvision.transforms"] = tv.transforms
    sys.modules["torchvision.transforms.functional"] = tv.transforms.functional
    for pkg in ("lib.train", "lib.train.data"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    _load("lib.train.data.processing_utils")
    tfm = _load("lib.train.data.transforms_rgbt")
    proc = _load("lib.train.data.processing_rgbt")
    return tfm, proc


def build_processing(tfm, proc, cfg):
    """lib/train/base_functions.py:177-205."""
    joint = tfm.Transform(tfm.ToGrayscale(probability=0.05), tfm.RandomHorizontalFlip(probability=0.5))
    train = tfm.Transform(tfm.ToTensorAndJitter(0.2), tfm.RandomHorizontalFlip_Norm(probability=0.5),
                          tfm.Normalize(mean=list(cfg.mean), std=list(cfg.std)))
    return proc.MixformerProcessing(
        search_area_factor={"template": cfg.template_factor, "search": cfg.search_factor},
        output_sz={"template": cfg.template_size, "search": cfg.search_size},
        center_jitter_factor={"template": cfg.template_center_jitter, "search": cfg.search_center_jitter},
        scale_jitter_factor={"template": cfg.template_scale_jitter, "search": cfg.search_scale_jitter},
        mode="sequence", transform=train, joint_transform=joint, settings=None, train_score=False)


class Recorder:
    """Wraps the four draw functions the reference calls and keeps what they returned."""

    def __init__(self):
        self.random, self.uniform, self.randn, self.rand = [], [], [], []
        self._orig = (random.random, np.random.uniform, torch.randn, torch.rand)

    def __enter__(self):
        o_random, o_uniform, o_randn, o_rand = self._orig

        def rec(store, fn, conv):
            def wrapped(*a, **k):
                v = fn(*a, **k)
                store.append(conv(v))
                return v
            return wrapped
        random.random = rec(self.random, o_random, float)
        np.random.uniform = rec(self.uniform, o_uniform, float)
        torch.randn = rec(self.randn, o_randn, lambda t: t.numpy().copy())
        torch.rand = rec(self.rand, o_rand, lambda t: t.numpy().copy())
        return self

    def __exit__(self, *exc):
        random.random, np.random.uniform, torch.randn, torch.rand = self._orig


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def make_frames():
    rng = np.random.default_rng(11)
    return [[rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(2)] for h, w in FRAME_SHAPES]


def split(frames, annos, cfg):
    nt = cfg.n_template
    a = [[np.asarray(b, np.float32) for b in pair] for pair in annos]
    return {"template": frames[:nt], "search": frames[nt:]}, {"template": a[:nt], "search": a[nt:]}


# annos per sample: [t0, t1, s0] x [rgb, tir] x (x, y, w, h); the TIR label differs a little from the RGB one
def _tir(b):
    return [b[0] + 1.5, b[1] - 0.75, b[2] * 0.9375, b[3] * 1.0625]


def _annos(t0, t1, s0):
    return [[b, _tir(b)] for b in (t0, t1, s0)]


SPECS = [
    # (config, annos, what the rolls must show, what the sample must be)
    ("small", _annos([30, 20, 32, 32], [20.5, 18.25, 8, 10], [40, 30, 20, 24]),      # exact 2x, up-scale
     lambda r: not r.gray and not r.joint_flip and not r.crop_flip[2], "valid"),
    ("small", _annos([40.2, 30.7, 25, 20], [30, 30, 12.5, 9], [30.3, 20.9, 18, 22]),  # fractional down-scale
     lambda r: not r.gray and r.joint_flip and not r.crop_flip[2], "valid"),
    ("small", _annos([2, 30, 20, 20], [60, 25, 16, 18], [10, 10, 22, 16]),            # left edge, right edge
     lambda r: not r.gray and not r.joint_flip and r.crop_flip[2], "valid"),
    ("small", _annos([80, 30, 14, 18], [1, 20, 16, 18], [70, 40, 20, 20]),            # right edge, left edge
     lambda r: not r.gray and r.joint_flip and r.crop_flip[2], "valid"),
    ("small", _annos([40, 1, 20, 16], [30, 50, 18, 12], [44, 33, 16, 20]),            # top edge, bottom edge
     lambda r: r.gray, "valid"),
    ("small", _annos([1, 2, 18, 18], [66, 50, 13, 13], [80, 60, 14, 10]),             # two corners
     lambda r: r.crop_flip[0] and not r.crop_flip[1], "valid"),
    ("small", _annos([30, 20, 20, 20], [30, 20, 0, 12], [40, 30, 20, 24]),            # crop_sz < 1
     lambda r: True, "small"),
    ("real", _annos([36, 25, 20, 30], [22, 24, 26, 18], [38, 28, 22, 26]),
     lambda r: not r.gray and r.crop_flip[2], "valid"),
    ("real", _annos([50.5, 30.25, 24, 20], [40, 22, 14, 20], [20, 30, 30, 24]),
     lambda r: not r.gray and r.joint_flip and not r.crop_flip[2], "valid"),
    ("real", _annos([36, 25, 20, 30], [22, 24, 26, 18], [-130, -110, 340, 300]),      # a sliver of frame in the crop
     lambda r: True, "mask"),
]


def main():
    tfm, proc = install()
    frames = make_frames()
    lut = ti.jet_lut()
    assert np.array_equal(lut, opre.jet_lut())
    rec = {"config_names": np.array(CONFIG_NAMES), "sizes": np.array([[c.template_size, c.search_size] for c in CONFIGS.values()]),
           "n_samples": np.int64(len(SPECS))}
    for k, pair in enumerate(frames):
        rec["frame_%d_v" % k], rec["frame_%d_i" % k] = pair
    seen = {"gray": 0, "flips": set(), "edges": set(), "area2": 0, "up": 0, "frac": 0}
    seed = 100
    for i, (cname, annos, want, kind) in enumerate(SPECS):
        cfg = CONFIGS[cname]
        processing = build_processing(tfm, proc, cfg)
        fr, an = split(frames, annos, cfg)
        while True:  # the next seed whose draws show what the sample is meant to cover
            seed += 1
            seed_all(seed)
            rolls = ti.draw_rolls(cfg.n_template, cfg.n_search)
            if not want(rolls):
                continue
            plans, valid = ti.plan_sample(fr, an, rolls, cfg)
            if kind == "valid" and valid:
                break
            if kind == "small" and any(p.crop_sz < 1 for p in plans):
                break
            if kind == "mask" and not valid and all(p.crop_sz >= 1 for p in plans):
                break
        data = {"template_images": [[v.copy(), t.copy()] for v, t in fr["template"]],
                "search_images": [[v.copy(), t.copy()] for v, t in fr["search"]],
                "template_anno": [[torch.from_numpy(b.copy()) for b in pair] for pair in an["template"]],
                "search_anno": [[torch.from_numpy(b.copy()) for b in pair] for pair in an["search"]]}
        seed_all(seed)
        with Recorder() as r:
            out = processing(data)
        pre = "s%d_" % i
        rec[pre + "config"] = np.int64(CONFIG_NAMES.index(cname))
        rec[pre + "annos"] = np.array(annos, dtype=np.float32)
        rec[pre + "seed"] = np.int64(seed)
        rec[pre + "valid"] = np.bool_(out["valid"])
        rec[pre + "ref_random"] = np.array(r.random, np.float64)
        rec[pre + "ref_uniform"] = np.array(r.uniform, np.float64)
        rec[pre + "ref_randn"] = np.array(r.randn, np.float32).reshape(-1, 2)
        rec[pre + "ref_rand"] = np.array(r.rand, np.float32).reshape(-1, 2)
        assert bool(out["valid"]) == (kind == "valid"), (i, kind, out["valid"])
        print("sample %d (%s, seed %d): valid %s, gray %s, joint flip %s, crop flips %s" %
              (i, cname, seed, out["valid"], rolls.gray, rolls.joint_flip, rolls.crop_flip))
        if not out["valid"]:
            continue
        seen["gray"] += rolls.gray
        for p in plans:
            seen["flips"].add((p.group, p.src_flip, p.out_flip))
            x1, y1, c = ti.crop_geometry(p.box, p.factor)
            if p.group == "template":
                seen["edges"] |= {e for e, on in (("left", x1 < 0), ("top", y1 < 0), ("right", x1 + c >= p.W),
                                                  ("bottom", y1 + c >= p.H)) if on}
            seen["area2"] += c == 2 * p.out_sz
            seen["up"] += c < p.out_sz
            seen["frac"] += p.out_sz < c < 2 * p.out_sz
        boxes, k = [], 0
        for g in ("template", "search"):
            for f, (imgs, bxs, atts) in enumerate(zip(out[g + "_images"], out[g + "_anno"], out[g + "_att"])):
                boxes.append([bxs[0].numpy(), bxs[1].numpy()])
                for m in range(2):
                    img = imgs[m].numpy()
                    assert img.dtype == np.float32 and atts[m].dtype == torch.bool
                    rec[pre + "img_sha_%d_%d" % (k, m)] = sha(img)
                    rec[pre + "att_sha_%d_%d" % (k, m)] = sha(atts[m].numpy())
                    if img.shape[-1] <= 32:
                        rec[pre + "img_%d_%d" % (k, m)] = img
                k += 1
        rec[pre + "boxes"] = np.array(boxes, dtype=np.float32)
    assert seen["gray"] >= 1 and seen["area2"] >= 1 and seen["up"] >= 1 and seen["frac"] >= 1, seen
    assert seen["edges"] == {"left", "top", "right", "bottom"}, seen
    for g in ("template", "search"):
        assert {(g, a, b) for a in (False, True) for b in (False, True)} <= seen["flips"], seen
    path = os.path.join(HERE, "train_input.npz")
    np.savez_compressed(path, **rec)
    print("wrote train_input.npz: %d samples, %d bytes" % (len(SPECS), os.path.getsize(path)))


if __name__ == "__main__":
    main()
