"""The list-indexed crop and box-update kernels of the batched tracker's packed step on the GPU
(csrc/preprocess.hip: mmt_sample_target_packed, mmt_track_update_packed).

Packed crop: every packed row equals, bit for bit, the `out` mmt_sample_target_table writes for the same
entry in a launch of its own, and so does the entry's crop record and patch; the entries' own `out`
buffers, the packed rows of skipped positions and every record of an unlisted slot keep their sentinel
fill.  Packed update: listed live slots equal oracle.preprocess.track_update exactly, every other slot's
state is bitwise unchanged."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import preprocess as pp

pytestmark = pytest.mark.gpu

SENTINEL_F, SENTINEL_U8, SENTINEL_D = -777.25, 0xAB, -3.5
SLOTS, PER = 9, 2
INT32_MAX = 2 ** 31 - 1


def _frame(H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


class _Entries:
    """SLOTS x PER crop descriptors over two frame sizes (LUT on the odd entries) with sentinel-filled
    out / patch / crop buffers, as a device table."""

    def __init__(self, osz, override=None):
        from mmt_amd import tracking
        from mmt_amd._lib import CropParams
        self.osz = osz
        self.ims = [torch.from_numpy(_frame(33, 47, 3)).cuda(), torch.from_numpy(_frame(97, 131, 4)).cuda()]
        self.lut = torch.from_numpy(pp.jet_lut().reshape(-1)).cuda()
        rng = np.random.default_rng(17)
        n = SLOTS * PER
        self.params, self.bufs = [], []
        for e in range(n):
            im = self.ims[(e // PER) % 2]
            H, W = im.shape[:2]
            box = [rng.uniform(-6, W - 4), rng.uniform(-6, H - 4), rng.uniform(2, W / 2), rng.uniform(2, H / 2)]
            if e % 5 == 0:
                box = [round(v) for v in box]
            b = torch.tensor(box, dtype=torch.float64, device="cuda")
            out = torch.full((3 * osz * osz,), SENTINEL_F, device="cuda")
            patch = torch.full((osz * osz * 3,), SENTINEL_U8, dtype=torch.uint8, device="cuda")
            crop = torch.full((4,), SENTINEL_D, dtype=torch.float64, device="cuda")
            p = tracking.crop_params(im, b, 2.0 + (e % 3), osz, out=out, patch=patch, crop=crop,
                                     lut=self.lut if e % 2 else None)
            for k, v in (override or {}).get(e, {}).items():
                setattr(p, k, v)
            self.params.append(p)
            self.bufs.append((b, out, patch, crop))
        arr = (CropParams * n)(*self.params)
        self.table = torch.frombuffer(arr, dtype=torch.uint8).cuda()

    def reset(self):
        for _, out, patch, crop in self.bufs:
            out.fill_(SENTINEL_F)
            patch.fill_(SENTINEL_U8)
            crop.fill_(SENTINEL_D)

    def untouched(self, e):
        _, out, patch, crop = self.bufs[e]
        return bool((out == SENTINEL_F).all() and (patch == SENTINEL_U8).all() and (crop == SENTINEL_D).all())

    def reference(self, enable=None):
        """What mmt_sample_target_table writes for every entry, in a launch of its own: [(out, patch, crop)]."""
        from mmt_amd._lib import LIB, check
        self.reset()
        en = torch.tensor(enable, dtype=torch.uint8).cuda() if enable is not None else None
        check(LIB.mmt_sample_target_table(self.table.data_ptr(), en.data_ptr() if en is not None else None, SLOTS * PER,
                                          self.osz, torch.cuda.current_stream().cuda_stream), "mmt_sample_target_table")
        torch.cuda.synchronize()
        ref = [(out.clone(), patch.clone(), crop.clone()) for _, out, patch, crop in self.bufs]
        self.reset()
        return ref

    def packed(self, lst, enable=None):
        from mmt_amd._lib import LIB, check
        n, row = len(lst), 3 * self.osz * self.osz
        rows = torch.full((PER, n, row), SENTINEL_F, device="cuda")
        lst_dev = torch.tensor(lst, dtype=torch.int32).cuda()
        en = torch.tensor(enable, dtype=torch.uint8).cuda() if enable is not None else None
        check(LIB.mmt_sample_target_packed(self.table.data_ptr(), en.data_ptr() if en is not None else None,
                                           lst_dev.data_ptr(), n, SLOTS, PER, self.osz, rows.data_ptr(), n * row, row,
                                           torch.cuda.current_stream().cuda_stream), "mmt_sample_target_packed")
        torch.cuda.synchronize()
        return rows


def _lists(n):
    """A list of n positions: a permutation of slots (without repeats), -1 padding, an index of SLOTS and an
    index of INT32_MAX."""
    rng = np.random.default_rng(n)
    if n == 1:
        return [[4], [-1], [SLOTS], [INT32_MAX]]
    perm = [int(v) for v in rng.permutation(SLOTS)]
    if n == 5:
        return [[perm[0], -1, SLOTS, perm[1], INT32_MAX]]
    lst = [-1] * n  # 130 positions: 7 of the 9 slots spread over the list, the bad indices between them
    for k, s in enumerate(perm[:7]):
        lst[3 + 19 * k] = s
    lst[0], lst[64], lst[129] = SLOTS, INT32_MAX, perm[7]
    lst[1] = -(2 ** 31)
    return [lst]


def _check(ent, ref, lst, rows, enable=None, skipped_entries=()):
    listed = {s for s in lst if 0 <= s < SLOTS}
    for j, s in enumerate(lst):
        for m in range(PER):
            e = s * PER + m
            live = 0 <= s < SLOTS and (enable is None or enable[e]) and e not in skipped_entries
            if not live:
                assert bool((rows[m, j] == SENTINEL_F).all()), "packed row %d.%d of a skipped position was written" % (j, m)
                continue
            out, patch, crop = ref[e]
            assert torch.equal(rows[m, j].view(torch.int32), out.view(torch.int32)), (j, m, e)
            assert torch.equal(ent.bufs[e][2], patch), (j, m, e)
            assert torch.equal(ent.bufs[e][3].view(torch.int64), crop.view(torch.int64)), (j, m, e)
            assert not bool((crop == SENTINEL_D).any())  # the reference launch did write it
    for e in range(SLOTS * PER):
        _, out, patch, crop = ent.bufs[e]
        assert bool((out == SENTINEL_F).all()), "entry %d's own out was written" % e
        skipped = e // PER not in listed or (enable is not None and not enable[e]) or e in skipped_entries
        if skipped:
            assert ent.untouched(e), "record of unlisted / skipped entry %d was written" % e


@pytest.mark.parametrize("osz", [16, 17, 128])
@pytest.mark.parametrize("n", [1, 5, 130])
def test_sample_target_packed_bit_exact(osz, n):
    """out_sz 16: exactly one 256-pixel tile; 17: a second tile with 33 live pixels; 128: 64 tiles."""
    ent = _Entries(osz)
    ref = ent.reference()
    for lst in _lists(n):
        ent.reset()
        rows = ent.packed(lst)
        _check(ent, ref, lst, rows)


def test_sample_target_packed_skip_rules():
    """The enable byte, a NULL image and a foreign out_sz skip an entry of a listed slot (nothing written for
    it, the slot's other modality still runs), as in mmt_sample_target_table."""
    osz = 16
    over = {2 * 3 + 1: dict(image=None), 2 * 5 + 0: dict(out_sz=64), 2 * 6 + 1: dict(H=0), 2 * 7 + 0: dict(factor=0.0),
            2 * 8 + 1: dict(box=None)}
    ent = _Entries(osz, over)
    enable = [1] * (SLOTS * PER)
    enable[2 * 1 + 0] = 0
    enable[2 * 2 + 0] = enable[2 * 2 + 1] = 0
    ref = ent.reference(enable)
    for e in list(over) + [2, 4, 5]:
        assert bool((ref[e][0] == SENTINEL_F).all())  # the table launch skips them too
    lst = [8, 7, 6, 5, 3, 2, 1, 0, -1]
    ent.reset()
    rows = ent.packed(lst, enable)
    _check(ent, ref, lst, rows, enable, skipped_entries=set(over))
    # a NULL enable pointer enables every entry
    ref = ent.reference(None)
    ent.reset()
    rows = ent.packed(lst, None)
    _check(ent, ref, lst, rows, None, skipped_entries=set(over))


def test_track_update_packed_bit_exact():
    """257 slots, a list of 130 (two full 64-thread blocks and a partial one) drawn without repeats, with -1
    and out-of-range entries, three frame sizes, some listed slots inactive or without a frame size."""
    from mmt_amd._lib import LIB, check
    rng = np.random.default_rng(5)
    slots, n, ss, stride = 257, 130, 320, 8
    sizes = np.array([(360, 480), (240, 320), (97, 131)], dtype=np.int32)
    hw = sizes[rng.integers(0, 3, slots)]
    lst = rng.permutation(slots)[:n].astype(np.int64)
    bad = rng.permutation(n)[:12]
    lst[bad] = [-1, -1, -1, -7, slots, slots + 1, INT32_MAX, -(2 ** 31), 4096, -1, slots, 2 ** 30]
    assert len(set(int(s) for s in lst if 0 <= s < slots)) == n - 12
    pred = rng.uniform(-0.2, 1.2, (n, 4)).astype(np.float32)
    pred[:, 2:] = np.abs(pred[:, 2:])
    state = np.stack([rng.uniform(-50, 480, slots), rng.uniform(-50, 360, slots), rng.uniform(1, 300, slots),
                      rng.uniform(1, 300, slots)], 1)
    rf = rng.uniform(0.2, 6.0, slots)
    crop = rng.uniform(-5, 5, (slots, stride))
    crop[:, 3] = rf
    active = (rng.uniform(size=slots) < 0.7).astype(np.uint8)
    good = [int(s) for s in lst if 0 <= s < slots]
    hw[good[3]] = (0, 480)  # listed, active, no frame size: skipped
    hw[good[4]] = (360, -1)
    active[good[3]] = active[good[4]] = 1
    assert 0 < sum(int(active[s]) for s in good) < len(good)
    st_dev = torch.from_numpy(state.copy()).cuda()
    pred_dev, crop_dev = torch.from_numpy(pred).cuda(), torch.from_numpy(crop).cuda()
    hw_dev, act_dev = torch.from_numpy(hw.copy()).cuda(), torch.from_numpy(active).cuda()
    lst_dev = torch.from_numpy(lst.astype(np.int32)).cuda()
    check(LIB.mmt_track_update_packed(pred_dev.data_ptr(), crop_dev.data_ptr(), stride, st_dev.data_ptr(), hw_dev.data_ptr(),
                                      act_dev.data_ptr(), lst_dev.data_ptr(), n, slots, ss, 10.0,
                                      torch.cuda.current_stream().cuda_stream), "mmt_track_update_packed")
    got = st_dev.cpu().numpy()
    row_of = {int(s): j for j, s in enumerate(lst) if 0 <= s < slots}
    updated = 0
    for s in range(slots):
        j = row_of.get(s)
        if j is not None and active[s] and hw[s, 0] > 0 and hw[s, 1] > 0:
            ref = pp.track_update(pred[j], list(state[s]), float(rf[s]), int(hw[s, 0]), int(hw[s, 1]), ss)
            assert got[s].tolist() == ref, (s, j, got[s].tolist(), ref)
            updated += 1
        else:
            assert np.array_equal(got[s].view(np.uint64), state[s].view(np.uint64)), s
    assert updated > 64
    # a NULL active pointer: every listed slot with a frame size runs
    st_dev = torch.from_numpy(state.copy()).cuda()
    check(LIB.mmt_track_update_packed(pred_dev.data_ptr(), crop_dev.data_ptr(), stride, st_dev.data_ptr(), hw_dev.data_ptr(),
                                      None, lst_dev.data_ptr(), n, slots, ss, 10.0,
                                      torch.cuda.current_stream().cuda_stream), "mmt_track_update_packed")
    got = st_dev.cpu().numpy()
    for s in range(slots):
        j = row_of.get(s)
        if j is not None and hw[s, 0] > 0 and hw[s, 1] > 0:
            assert got[s].tolist() == pp.track_update(pred[j], list(state[s]), float(rf[s]), int(hw[s, 0]), int(hw[s, 1]), ss)
        else:
            assert np.array_equal(got[s].view(np.uint64), state[s].view(np.uint64)), s
