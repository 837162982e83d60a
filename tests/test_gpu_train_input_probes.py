"""mmt_train_crops_table (csrc/train_input.hip) on the GPU against mmt_amd.train_input.crop_reference, bit for bit.

Every entry writes out (compared as fp32 bits), att, patch and its crop record into storage of its own that is
filled with NaN / 0xA5 and sits between guards that must stay intact; every pointer is off its 16-byte alignment
(out by 4 bytes, att by 1, patch by 3, crop by 8, the frame by 1).  The entries (tests/train_input_probes.py) are
the smallest that reach every branch: out_sz 16 (one block per entry) and 32 (four), frames of 1x1, 23x37 and
38x54, an exact 2x, an up-scale and a fractional down-scale, crops across every edge and corner and entirely
outside the frame, all eight flag combinations on odd and even widths, and gains that land on both clamps."""
import ctypes

import numpy as np
import pytest
import torch

from train_input_probes import probe_entries, probe_frame, probe_reference

pytestmark = pytest.mark.gpu

GUARD = 256  # bytes
G = 0xA5
NAN32 = 0x7fc00000


def _nan32(n):
    return torch.full((n,), NAN32, dtype=torch.int32, device="cuda")


class _Entry:
    """One entry's device storage."""

    def __init__(self, e, lut):
        from mmt_amd.train_input import MEAN, STD
        self.e, s = e, e["out_sz"]
        self.s = s
        f = np.ascontiguousarray(e["frame"])
        self.H, self.W = f.shape[:2]
        self.image = torch.zeros(1 + f.size, dtype=torch.uint8, device="cuda")
        self.image[1:].copy_(torch.from_numpy(f.reshape(-1)))
        self.box = torch.tensor(e["box"], dtype=torch.float64, device="cuda")
        self.n_out = 3 * s * s
        self.out = _nan32(2 * GUARD // 4 + 1 + self.n_out)
        self.att = torch.full((2 * GUARD + 1 + s * s,), G, dtype=torch.uint8, device="cuda")
        self.patch = torch.full((2 * GUARD + 3 + 3 * s * s,), G, dtype=torch.uint8, device="cuda")
        self.crop = torch.full((2 * GUARD // 8 + 1 + 4,), float("nan"), dtype=torch.float64, device="cuda")
        self.lut = lut if e["tir"] else None
        self.mean, self.std = MEAN, STD

    def params(self, **override):
        from mmt_amd.train_input import crop_params
        e = self.e
        kw = dict(image=self.image.data_ptr() + 1, H=self.H, W=self.W, box=self.box.data_ptr(), factor=e["factor"],
                  out_sz=self.s, lut=self.lut.data_ptr() if self.lut is not None else None, mean=self.mean, std=self.std,
                  gain=e["gain"], src_flip=e["src_flip"], src_gray=e["src_gray"], out_flip=e["out_flip"],
                  out=self.out.data_ptr() + GUARD + 4, att=self.att.data_ptr() + GUARD + 1,
                  patch=self.patch.data_ptr() + GUARD + 3, crop=self.crop.data_ptr() + GUARD + 8)
        kw.update(override)
        return crop_params(**kw)

    def got(self):
        s = self.s
        lo = GUARD // 4 + 1
        out = self.out.cpu()[lo:lo + self.n_out].view(3, s, s).numpy()
        att = self.att.cpu()[GUARD + 1:GUARD + 1 + s * s].view(s, s).numpy()
        patch = self.patch.cpu()[GUARD + 3:GUARD + 3 + 3 * s * s].view(s, s, 3).numpy()
        crop = self.crop.cpu()[GUARD // 8 + 1:GUARD // 8 + 5].numpy()
        return out, att, patch, crop

    def guards_intact(self, written=("out", "att", "patch", "crop")):
        s = self.s
        out, att, patch, crop = self.out.cpu(), self.att.cpu(), self.patch.cpu(), self.crop.cpu().view(torch.int64)
        nan64 = torch.tensor(float("nan"), dtype=torch.float64).view(torch.int64)
        spans = {"out": (out, NAN32, GUARD // 4 + 1, self.n_out), "att": (att, G, GUARD + 1, s * s),
                 "patch": (patch, G, GUARD + 3, 3 * s * s), "crop": (crop, nan64, GUARD // 8 + 1, 4)}
        for name, (t, fill, lo, n) in spans.items():
            if name not in written:
                n = 0
            if not (bool((t[:lo] == fill).all()) and bool((t[lo + n:] == fill).all())):
                return False
        return True

    def untouched(self):
        return self.guards_intact(())

    def check(self, ref, tag, written=("out", "att", "patch", "crop")):
        out, att, patch, crop = self.got()
        r_out, r_att, r_patch, r_crop = ref
        if "out" in written:
            assert np.array_equal(out.view(np.uint32), r_out.view(np.uint32)), tag  # fp32 bits
        if "att" in written:
            assert np.array_equal(att, r_att.astype(np.uint8)), tag
        if "patch" in written:
            assert np.array_equal(patch, r_patch), tag
        if "crop" in written:
            assert np.array_equal(crop, r_crop), (tag, crop, r_crop)
        assert self.guards_intact(written), tag


def _lut():
    from mmt_amd.train_input import jet_lut
    return torch.from_numpy(jet_lut()).cuda()


def _launch(params, out_sz, enable=None, n=None):
    from mmt_amd.train_input import launch_train_crops, table_tensor
    tab = table_tensor(params, "cuda")
    en = torch.tensor(enable, dtype=torch.uint8).cuda() if enable is not None else None
    launch_train_crops(tab, en, len(params) if n is None else n, out_sz)
    torch.cuda.synchronize()
    return tab, en


@pytest.mark.parametrize("out_sz", [16, 32])
def test_every_probe_entry_equals_the_contract(out_sz):
    lut = _lut()
    cases = probe_entries(out_sz)
    refs = probe_reference(out_sz)
    entries = [_Entry(e, lut) for _, e in cases]
    _launch([x.params() for x in entries], out_sz)
    for (name, _), x, ref in zip(cases, entries, refs):
        x.check(ref, name)
    # the probes reach what they are meant to: both clamps, padding and frame in one mask, both resize paths
    outs = np.stack([r[0] for r in refs])
    from mmt_amd.train_input import MEAN, STD
    lo = (np.float32(0) - np.float32(MEAN[0])) / np.float32(STD[0])
    hi = (np.float32(1) - np.float32(MEAN[0])) / np.float32(STD[0])
    assert (outs[:, 0] == lo).any() and (outs[:, 0] == hi).any()
    assert any(r[1].any() and not r[1].all() for r in refs) and any(r[1].all() for r in refs)
    assert any(r[3][2] == 2 * out_sz for r in refs) and any(0 < r[3][2] < out_sz for r in refs)
    assert any(r[3][2] == 0 for r in refs)
    # all eight flag combinations meet the exact-2x path at this out_sz
    assert {(e["src_flip"], e["src_gray"], e["out_flip"]) for (_, e), r in zip(cases, refs) if r[3][2] == 2 * out_sz} == {
        (a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)}


def test_every_skip_rule_leaves_the_guards_intact():
    lut = _lut()
    out_sz = 16
    cases = dict(probe_entries(out_sz))
    refs = dict(zip([n for n, _ in probe_entries(out_sz)], probe_reference(out_sz)))
    base = cases["flags5_23x37_tir_9"]
    skips = [("disabled", {}, 0), ("image", dict(image=None), 1), ("box", dict(box=None), 1),
             ("no_output", dict(out=None, att=None, patch=None), 1), ("H0", dict(H=0), 1), ("Wneg", dict(W=-3), 1),
             ("factor0", dict(factor=0.0), 1), ("factor_neg", dict(factor=-2.0), 1), ("factor_nan", dict(factor=float("nan")), 1),
             ("out_sz", dict(out_sz=32), 1), ("gain_neg", dict(gain=-0.5), 1), ("gain_nan", dict(gain=float("nan")), 1),
             ("gain_inf", dict(gain=float("inf")), 1)]
    entries = [_Entry(base, lut) for _ in skips]
    live = [_Entry(base, lut) for _ in range(4)]  # the first and the last entry, and partial outputs
    partial = [("out", "att", "patch", "crop"), ("att",), ("patch", "crop"), ("out", "att", "patch", "crop")]
    nulls = [{k: None for k in ("out", "att", "patch", "crop") if k not in w} for w in partial]
    params = ([live[0].params(**nulls[0])] + [x.params(**kw) for x, (_, kw, _) in zip(entries, skips)]
              + [live[i].params(**nulls[i]) for i in (1, 2, 3)])
    enable = [1] + [en for _, _, en in skips] + [1, 1, 1]
    _launch(params, out_sz, enable)
    for x, (name, _, _) in zip(entries, skips):
        assert x.untouched(), name
    for x, w in zip(live, partial):
        x.check(refs["flags5_23x37_tir_9"], "live", w)
    # enable NULL: every entry runs
    again = [_Entry(base, lut) for _ in range(2)]
    _launch([x.params() for x in again], out_sz, None)
    for x in again:
        x.check(refs["flags5_23x37_tir_9"], "enable NULL")
    # n smaller than the table: the rest is not reached
    rest = [_Entry(base, lut) for _ in range(3)]
    _launch([x.params() for x in rest], out_sz, None, n=2)
    rest[0].check(refs["flags5_23x37_tir_9"], "n")
    assert rest[2].untouched()


def test_a_repointed_entry_takes_effect_and_a_captured_launch_follows_the_table():
    from mmt_amd.train_input import MEAN, STD, crop_reference, jet_lut, launch_train_crops, table_tensor
    lut = _lut()
    out_sz = 32
    cases = dict(probe_entries(out_sz))
    names = [n for n, _ in probe_entries(out_sz)]
    refs = dict(zip(names, probe_reference(out_sz)))
    a, b = "flags3_38x54_rgb_9", "corner_br_tir"
    xa, xb = _Entry(cases[a], lut), _Entry(cases[b], lut)
    tab = table_tensor([xa.params()], "cuda")
    en = torch.ones(1, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch_train_crops(tab, en, 1, out_sz)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    xa.check(refs[a], "eager")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch_train_crops(tab, en, 1, out_sz)
    graph.replay()
    torch.cuda.synchronize()
    xa.check(refs[a], "replay")
    assert xb.untouched()
    # the entry re-pointed at another frame, size, modality, flags and outputs: the same graph
    tab.copy_(table_tensor([xb.params()], "cuda"))
    graph.replay()
    torch.cuda.synchronize()
    xb.check(refs[b], "replay after the table changed")
    # a new frame behind the same pointer, a new box and a new gain
    frame2 = probe_frame(23, 37, 77)
    xb.image[1:].copy_(torch.from_numpy(frame2.reshape(-1)).cuda())
    xb.box.copy_(torch.tensor([3.0, 2.0, 12.0, 10.0], dtype=torch.float64))
    tab.copy_(table_tensor([xb.params(gain=0.75, out_flip=1)], "cuda"))
    graph.replay()
    torch.cuda.synchronize()
    xb.check(crop_reference(frame2, [3.0, 2.0, 12.0, 10.0], 2.0, out_sz, jet_lut(), MEAN, STD, 0.75, False, False, True),
             "new frame")
    # disabled: the replay writes nothing
    fresh = _Entry(cases[b], lut)
    tab.copy_(table_tensor([fresh.params()], "cuda"))
    en.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert fresh.untouched()


@pytest.mark.parametrize("out_sz", [16, 32])
def test_patch_and_crop_equal_the_tracker_kernel_with_all_flags_off(out_sz):
    """With all flags off, the resized uint8 crop and the crop record are mmt_sample_target_table's on the same
    entries: the two kernels share the geometry and the resize."""
    from mmt_amd._lib import LIB, CropParams, check
    lut = _lut()
    cases = [(n, e) for n, e in probe_entries(out_sz)
             if not (e["src_flip"] or e["src_gray"] or e["out_flip"]) and "gain" not in n]
    assert len(cases) >= 30
    mine = [_Entry(e, lut) for _, e in cases]
    _launch([x.params() for x in mine], out_sz)
    s = out_sz
    patch = torch.full((len(cases), s, s, 3), G, dtype=torch.uint8, device="cuda")
    crop = torch.full((len(cases), 4), float("nan"), dtype=torch.float64, device="cuda")
    arr = (CropParams * len(cases))()
    for i, x in enumerate(mine):
        p = arr[i]
        p.image, p.H, p.W, p.box, p.factor, p.out_sz = x.image.data_ptr() + 1, x.H, x.W, x.box.data_ptr(), x.e["factor"], s
        p.lut, p.out, p.patch, p.crop = None, None, patch[i].data_ptr(), crop[i].data_ptr()
        for c in range(3):
            p.mean[c], p.std[c] = x.mean[c], x.std[c]
    tab = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).cuda()
    check(LIB.mmt_sample_target_table(tab.data_ptr(), None, len(cases), s, torch.cuda.current_stream().cuda_stream),
          "mmt_sample_target_table")
    torch.cuda.synchronize()
    patch, crop = patch.cpu().numpy(), crop.cpu().numpy()
    for i, ((name, _), x) in enumerate(zip(cases, mine)):
        _, _, got_patch, got_crop = x.got()
        assert np.array_equal(got_patch, patch[i]), name
        assert np.array_equal(got_crop.view(np.uint64), crop[i].view(np.uint64)), name  # inf at crop_sz 0 included
