"""Host side of the training input (no GPU): mmt_amd.train_input's contract against the fixture recorded from the
reference's own MixformerProcessing (tests/golden/train_input.npz), the closed-form validity against the mask it
abbreviates, the pixel restatements against oracle/preprocess.py, the C ABI (symbols, struct layout, refusals
before any launch), the op's fake kernel and the refusals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT
from train_input_probes import (N_FRAMES, contract, fixture, fixture_config, fixture_rolls, fixture_sample, probe_frame,
                                sha)

HEADER = os.path.join(ROOT, "include", "mmt_hip.h")
EBADARG = -10000
N = int(fixture()["n_samples"])
VALID = [i for i in range(N) if bool(fixture()["s%d_valid" % i])]
KEYS = [("template", 0), ("template", 1), ("search", 0)]  # frame k of the fixture -> (group, index)


# ------------------------------------------------------------------ the contract against the reference
def test_fixture_covers_what_it_must():
    fx = fixture()
    assert os.path.getsize(os.path.join(GOLDEN, "train_input.npz")) <= max(
        os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f != "train_input.npz")
    assert len(VALID) >= 6 and len(VALID) <= N - 2
    rolls = [fixture_rolls(i) for i in VALID]
    assert any(r.gray for r in rolls) and any(not r.gray for r in rolls)
    for k in range(N_FRAMES):
        assert {(r.joint_flip, r.crop_flip[k]) for r in rolls} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {tuple(fx["sizes"][int(fx["s%d_config" % i])]) for i in VALID} == {(32, 64), (128, 320)}


@pytest.mark.parametrize("i", range(N))
def test_draw_rolls_reproduces_the_reference_draws(i):
    """Seeding the three generators with the recorded seed, draw_rolls returns what the reference drew, in its order.
    A sample the reference rejected stopped drawing early: the draws it made are a prefix."""
    fx = fixture()
    r = fixture_rolls(i)
    rnd, uni = fx["s%d_ref_random" % i], fx["s%d_ref_uniform" % i]
    randn, rand = fx["s%d_ref_randn" % i], fx["s%d_ref_rand" % i]
    assert len(rnd) >= 2
    assert r.gray == bool(rnd[0] < 0.05) and r.joint_flip == bool(rnd[1] < 0.5)
    assert [bool(v < 0.5) for v in rnd[2:]] == list(r.crop_flip[:len(rnd) - 2])
    mine = np.array([v for pair in zip(r.bf, r.tf) for v in pair])
    assert np.array_equal(uni, mine[:len(uni)])
    assert np.array_equal(randn, r.randn[:len(randn)]) and np.array_equal(rand, r.rand[:len(rand)])
    if bool(fx["s%d_valid" % i]):
        assert len(rnd) == 2 + N_FRAMES and len(uni) == 2 * N_FRAMES and len(randn) == N_FRAMES == len(rand)


@pytest.mark.parametrize("i", range(N))
def test_contract_equals_the_reference(i):
    fx = fixture()
    out = contract(i)
    assert out["valid"] == bool(fx["s%d_valid" % i])
    if not out["valid"]:
        assert set(out) == {"valid"}
        return
    boxes = fx["s%d_boxes" % i]
    for k, (g, f) in enumerate(KEYS):
        for m, name in enumerate("vi"):
            box = out["%s_anno_%s" % (g, name)][f]
            assert box.dtype == torch.float32
            assert np.array_equal(box.numpy(), boxes[k, m]), (k, name, box, boxes[k, m])  # ==, every box in full
            img = out["%s_images_%s" % (g, name)][f].numpy()
            s = fixture_config(i).group(g)[1]
            assert img.dtype == np.float32 and img.shape == (3, s, s)
            assert np.array_equal(sha(img), fx["s%d_img_sha_%d_%d" % (i, k, m)]), (k, name)
            att = out["%s_att_%s" % (g, name)][f].numpy()
            assert att.dtype == np.bool_ and att.shape == (s, s)
            assert np.array_equal(sha(att), fx["s%d_att_sha_%d_%d" % (i, k, m)]), (k, name)
            key = "s%d_img_%d_%d" % (i, k, m)
            if key in fx:  # the small output sizes: the whole array
                assert np.array_equal(img.view(np.uint32), fx[key].view(np.uint32))
    t, s = fixture_config(i).template_size, fixture_config(i).search_size
    assert tuple(out["template_images_v"].shape) == (2, 3, t, t) and tuple(out["search_images_i"].shape) == (1, 3, s, s)
    assert tuple(out["template_anno_i"].shape) == (2, 4) and tuple(out["search_att_v"].shape) == (1, s, s)


def test_fixture_holds_whole_images_at_the_small_sizes():
    fx = fixture()
    whole = [k for k in fx if "_img_" in k and "sha" not in k]
    assert len(whole) >= 4 * 6 and all(fx[k].shape == (3, 32, 32) for k in whole)


def test_invalid_samples_are_one_of_each_kind():
    from mmt_amd.train_input import plan_sample
    kinds = set()
    for i in range(N):
        if i in VALID:
            continue
        frames, annos = fixture_sample(i)
        plans, valid = plan_sample(frames, annos, fixture_rolls(i), fixture_config(i))
        assert not valid
        kinds.add("small" if any(p.crop_sz < 1 for p in plans) else "mask")
    assert kinds == {"small", "mask"}


# ------------------------------------------------------------------ the closed-form validity
def _mask_valid(box, factor, H, W, out_sz, out_flip):
    """The reference's two mask checks (processing_rgbt.py:206-220), literally, on the attention mask itself."""
    from mmt_amd.train_input import att_mask, crop_geometry
    x1, y1, crop = crop_geometry(box, factor)
    if crop < 1:
        return False
    att = torch.from_numpy(att_mask(x1, y1, crop, H, W, out_sz))
    if out_flip:
        att = att.flip((-1,))
    if (att == 1).all():
        return False
    down = F.interpolate(att[None, None].float(), size=out_sz // 16).to(torch.bool)[0]
    return not bool((down == 1).all())


def test_closed_form_validity_equals_the_mask_checks():
    from mmt_amd.train_input import att_mask, att_rows_cols, crop_geometry, crop_is_valid
    rng = np.random.default_rng(21)
    seen = {True: 0, False: 0}
    for n in range(1500):
        H, W = int(rng.integers(1, 60)), int(rng.integers(1, 80))
        out_sz = int(rng.choice([16, 32, 48, 64]))
        kind = n % 5
        if kind == 0:    # a crop much larger than the frame, anywhere around it
            w, h = rng.uniform(20, 400, 2)
            x, y = rng.uniform(-600, 300, 2)
        elif kind == 1:  # near the frame, any size
            w, h = rng.uniform(0.2, 60, 2)
            x, y = rng.uniform(-40, 80, 2)
        elif kind == 2:  # exact 2x: crop == 2 * out_sz
            w = h = float(out_sz)
            x, y = rng.integers(-2 * out_sz, W + 8), rng.integers(-2 * out_sz, H + 8)
        elif kind == 3:  # the frame a sliver between two picked rows / columns
            w = h = float(rng.uniform(100, 900))
            x, y = -w / 2 + rng.uniform(-30, 30), -h / 2 + rng.uniform(-30, 30)
        else:            # degenerate
            w, h = float(rng.choice([0.0, 1e-3, 0.3])), float(rng.uniform(0, 2))
            x, y = rng.uniform(0, W), rng.uniform(0, H)
        box, factor, flip = [float(x), float(y), float(w), float(h)], float(rng.choice([2.0, 5.0])), bool(n & 1)
        got = crop_is_valid(box, factor, H, W, out_sz, flip)
        assert got == _mask_valid(box, factor, H, W, out_sz, flip), (n, box, factor, H, W, out_sz, flip)
        seen[got] += 1
        x1, y1, crop = crop_geometry(box, factor)
        if crop >= 1 and crop <= 1200:
            rows, cols = att_rows_cols(x1, y1, crop, H, W, out_sz)
            assert np.array_equal(att_mask(x1, y1, crop, H, W, out_sz), rows[:, None] | cols[None, :]), (n, box)
    assert seen[True] > 200 and seen[False] > 200, seen


def test_mask_check_points_are_the_nearest_picks():
    from mmt_amd.train_input import mask_check_points
    for s in (16, 32, 48, 64, 128, 320):
        ramp = torch.arange(s, dtype=torch.float32)[None, None, None, :].expand(1, 1, s, s)
        picked = F.interpolate(ramp, size=s // 16)[0, 0, 0].long().numpy()
        assert np.array_equal(mask_check_points(s), picked) and np.array_equal(picked, 16 * np.arange(s // 16))


# ------------------------------------------------------------------ the pixel restatements
def test_pixel_functions_equal_the_oracle():
    from mmt_amd import train_input as ti
    from oracle import preprocess as opre
    assert np.array_equal(ti.jet_lut(), opre.jet_lut())
    assert np.allclose(ti.MEAN, opre.MEAN) and np.allclose(ti.STD, opre.STD)
    rng = np.random.default_rng(4)
    im = probe_frame(38, 54, 9)
    for n in range(60):
        w, h = rng.uniform(1, 40, 2)
        box = [float(rng.uniform(-20, 50)), float(rng.uniform(-20, 36)), float(w), float(h)]
        out_sz = int(rng.choice([16, 32]))
        if n % 6 == 0:
            box[2] = box[3] = float(out_sz)  # exact 2x
        x1, y1, crop = ti.crop_geometry(box, 2.0)
        assert (x1, y1, crop) == opre.crop_geometry(box, 2.0)
        pad = ti.padded_crop(im, x1, y1, crop)
        assert np.array_equal(pad, opre.padded_crop(im, box, 2.0))
        assert np.array_equal(ti.resize_linear_u8(pad, out_sz), opre.resize_linear_u8(pad, out_sz))
        assert np.array_equal(ti.apply_colormap(pad, ti.jet_lut()), opre.apply_colormap(pad, opre.jet_lut()))


def test_crop_reference_arithmetic_on_literal_values():
    """One constant frame, one pixel value per case: the RGB product with the float32 scalar, the TIR jitter on
    uint8 before the colour map, the true division, both clamps."""
    from mmt_amd.train_input import MEAN, STD, crop_reference, jet_lut
    lut = jet_lut()
    m, s = np.float32(MEAN[0]), np.float32(STD[0])

    def centre(v, **kw):
        frame = np.full((40, 40, 3), v, np.uint8)
        out, att, patch, rec = crop_reference(frame, [10.0, 10.0, 8.0, 8.0], 2.0, 16, **kw)
        assert not att.any() and (patch == v).all() and rec[2] == 16 and rec[3] == 1.0
        return out[:, 8, 8]

    for v, bf in ((200, 1.1), (255, 1.2), (7, 0.8), (0, 1.0)):
        x = min(max(np.float32(v) * np.float32(bf / 255.0), np.float32(0)), np.float32(1))
        assert centre(v, gain=bf / 255.0)[0] == (x - m) / s
    assert centre(255, gain=1.2 / 255.0)[0] == (np.float32(1) - m) / s  # the upper clamp
    for v, tf in ((100, 0.5), (201, 1.2), (255, 1.2), (3, 0.3), (77, 1.0)):
        j = int(min(float(v) * tf, 255.0))  # truncation
        gray = (j * 1868 + j * 9617 + j * 4899 + 8192) >> 14
        want = [(np.float32(lut[gray, c]) / np.float32(255.0) - np.float32(MEAN[c])) / np.float32(STD[c]) for c in range(3)]
        assert list(centre(v, lut=lut, gain=tf)) == want


def test_joint_and_crop_flips_are_the_literal_steps():
    """src_flip / src_gray / out_flip equal flipping and graying whole arrays around an unflagged crop."""
    from mmt_amd.train_input import crop_reference, rgb2gray
    frame = probe_frame(23, 37, 2)
    box = [25.0, 12.0, 9.0, 8.0]
    out, att, patch, rec = crop_reference(frame, box, 2.0, 16, src_flip=True, src_gray=True, out_flip=True)
    out0, att0, patch0, rec0 = crop_reference(np.fliplr(rgb2gray(frame)).copy(), box, 2.0, 16)
    assert np.array_equal(out, out0[:, :, ::-1]) and np.array_equal(att, att0[:, ::-1])
    assert np.array_equal(patch, patch0[:, ::-1]) and np.array_equal(rec, rec0)
    assert att0.any() and not att0.all()  # the crop runs past the right edge of the mirrored frame


def test_box_functions_on_literal_values():
    from mmt_amd.train_input import crop_flip_box, joint_box, jitter_box, label_box
    b = torch.tensor([10.0, 20.0, 30.0, 40.0])
    assert joint_box(b, 100, False).tolist() == [10.0, 20.0, 30.0, 40.0]
    assert joint_box(b, 100, True).tolist() == [59.0, 20.0, 30.0, 40.0]  # (W0 - 1) - (x + w) = 59
    n = torch.tensor([0.25, 0.5, 0.25, 0.25])
    assert crop_flip_box(n, True).tolist() == [0.5, 0.5, 0.25, 0.25]
    # the corner form is not the identity in float32: (x + w) - x
    odd = torch.tensor([0.1, 0.2, 0.3, 0.4])
    assert joint_box(odd, 100, False)[2] == (odd[0] + odd[2]) - odd[0]
    # no jitter: the box itself; the label of a box in its own crop is centred
    j = jitter_box(b, np.zeros(2, np.float32), np.full(2, 0.5, np.float32), 0.5, 4.5)
    assert j.tolist() == b.tolist()
    lab = label_box(b, b, 0.5, 64)
    assert lab.tolist() == [(31.5 - 7.5) / 64, (31.5 - 10.0) / 64, 15.0 / 64, 20.0 / 64]


# ------------------------------------------------------------------ C ABI
def test_symbol_declared_exported_and_bound():
    from mmt_amd import _lib
    src = open(HEADER).read()
    assert "int mmt_train_crops_table(" in src and "} mmt_train_crop_params;" in src
    assert "mmt_train_crops_table" in _lib.EXPORTED
    assert _lib.LIB.mmt_train_crops_table.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                                       ctypes.c_void_p]
    assert open(os.path.join(ROOT, "multi-modal-tracking_amd", "csrc", "train_input.hip")).read().count("crop_common.hpp")
    assert '#include "crop_common.hpp"' in open(os.path.join(ROOT, "multi-modal-tracking_amd", "csrc", "preprocess.hip")).read()


def test_train_crop_params_layout_matches_header(tmp_path):
    from mmt_amd import _lib
    fields = [f for f, _ in _lib.TrainCropParams._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HEADER, "int main(void){",
           'printf("%zu\\n", sizeof(mmt_train_crop_params));']
    src += ['printf("%%zu\\n", offsetof(mmt_train_crop_params, %s));' % f for f in fields]
    src += ["return 0;}"]
    c = tmp_path / "abi.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", str(c), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out[0] == ctypes.sizeof(_lib.TrainCropParams)
    assert out[1:] == [getattr(_lib.TrainCropParams, f).offset for f in fields]


def test_train_crops_table_rejects_bad_args_before_any_launch():
    from mmt_amd._lib import LIB, TrainCropParams
    tab = (TrainCropParams * 2)()
    p = ctypes.addressof(tab)  # never dereferenced: every call below is rejected on the host
    assert LIB.mmt_train_crops_table(None, None, 2, 16, None) == EBADARG
    assert LIB.mmt_train_crops_table(p, None, 0, 16, None) == EBADARG
    assert LIB.mmt_train_crops_table(p, None, -1, 16, None) == EBADARG
    assert LIB.mmt_train_crops_table(p, None, 2, 0, None) == EBADARG
    assert LIB.mmt_train_crops_table(p, None, 2, -16, None) == EBADARG
    assert LIB.mmt_train_crops_table(p, None, 2, 16385, None) == EBADARG
    assert LIB.mmt_train_crops_table(p + 4, None, 1, 16, None) == EBADARG            # misaligned table
    assert LIB.mmt_train_crops_table(p, None, 0x7fffffff, 320, None) == EBADARG      # past the grid limit


def test_torch_op_registered_with_fake_kernel():
    from mmt_amd import ops  # noqa: F401
    from mmt_amd._lib import TrainCropParams
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert hasattr(torch.ops.mmt, "train_crops")
    size = ctypes.sizeof(TrainCropParams)
    with FakeTensorMode():
        img, att = torch.empty(2, 3, 16, 16), torch.empty(2, 16, 16, dtype=torch.uint8)
        got = torch.ops.mmt.train_crops(torch.empty(4 * size, dtype=torch.uint8), None, 16, img, img.clone(), att, att.clone(),
                                        torch.empty(2, 2, 4, dtype=torch.float64))
        assert got is None
    with pytest.raises(RuntimeError):  # no CPU path
        img, att = torch.zeros(2, 3, 16, 16), torch.zeros(2, 16, 16, dtype=torch.uint8)
        torch.ops.mmt.train_crops(torch.zeros(4 * size, dtype=torch.uint8), None, 16, img, img.clone(), att, att.clone(),
                                  torch.zeros(2, 2, 4, dtype=torch.float64))


# ------------------------------------------------------------------ refusals
def test_sample_refusals():
    from mmt_amd.train_input import TrainInputConfig, process_sample_reference
    frames, annos = fixture_sample(0)
    rolls, cfg = fixture_rolls(0), TrainInputConfig(template_size=32, search_size=64)

    def with_frame(x):
        return {"template": [[x, frames["template"][0][1]], frames["template"][1]], "search": frames["search"]}

    with pytest.raises(ValueError, match="uint8"):
        process_sample_reference(with_frame(np.zeros((72, 96, 3), np.float32)), annos, rolls, cfg)
    with pytest.raises(ValueError, match="uint8"):
        process_sample_reference(with_frame(torch.zeros(72, 96, 3, dtype=torch.uint8)), annos, rolls, cfg)
    with pytest.raises(ValueError, match=r"\(H, W, 3\)"):
        process_sample_reference(with_frame(np.zeros((72, 96, 1), np.uint8)), annos, rolls, cfg)
    with pytest.raises(ValueError, match=r"\(H, W, 3\)"):
        process_sample_reference(with_frame(np.zeros((72, 96), np.uint8)), annos, rolls, cfg)
    with pytest.raises(ValueError, match="differ in size"):
        process_sample_reference(with_frame(np.zeros((70, 96, 3), np.uint8)), annos, rolls, cfg)
    with pytest.raises(ValueError, match="frame pairs expected"):
        process_sample_reference({"template": frames["template"][:1], "search": frames["search"]}, annos, rolls, cfg)


def test_processor_refusals_need_no_gpu():
    from mmt_amd.train_input import TrainInputProcessor, check_batch
    sample = fixture_sample(0)
    with pytest.raises(ValueError, match="batch mismatch: the processor was built for 3 samples, got 2"):
        check_batch([sample, sample], None, 3)
    with pytest.raises(ValueError, match="batch mismatch: 2 samples, 1 rolls"):
        check_batch([sample, sample], [fixture_rolls(0)], 2)
    check_batch([sample, sample], [fixture_rolls(0)] * 2, 2)
    with pytest.raises(ValueError, match="runs on the GPU"):
        TrainInputProcessor((32, 64), 2, device="cpu")
    with pytest.raises(ValueError, match="batch"):
        TrainInputProcessor((32, 64), 0, device="cuda")
    with pytest.raises(ValueError, match="multiple of 16"):
        TrainInputProcessor((24, 64), 2, device="cuda")
