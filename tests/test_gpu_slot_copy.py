"""mmt_slot_copy (csrc/slot_cache.hip) on the GPU: bit-exact against torch indexing, with guard bytes.

Every destination is pre-filled with a position-dependent byte pattern, and the whole buffer -- the gaps
between rows (pitch > row_bytes), between slots (slot stride > rows * pitch), the slots of skipped entries
and the guard bytes before and after -- is compared with a host restatement of the contract, so a byte
written anywhere it should not be fails the test."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64  # bytes before slot 0 and after the last slot, multiples of 16


def _pattern(nbytes):
    return ((torch.arange(nbytes, dtype=torch.int64) * 7 + 3) % 251).to(torch.uint8)


def _random(nbytes, seed):
    return torch.randint(0, 256, (nbytes,), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


class _Seg:
    """One segment with byte buffers of its own: src random, dst the pattern."""

    def __init__(self, rows, row_bytes, spitch, dpitch, sstride, dstride, src_slots, dst_slots, seed):
        assert spitch >= row_bytes and dpitch >= row_bytes and sstride >= rows * spitch and dstride >= rows * dpitch
        self.rows, self.rb, self.sp, self.dp, self.ss, self.ds = rows, row_bytes, spitch, dpitch, sstride, dstride
        self.src = _random(2 * GUARD + src_slots * sstride, seed)
        self.dst0 = _pattern(2 * GUARD + dst_slots * dstride)
        self.src_dev, self.dst_dev = self.src.cuda(), self.dst0.cuda()

    def fill(self, a):
        a.src, a.dst = self.src_dev.data_ptr() + GUARD, self.dst_dev.data_ptr() + GUARD
        a.src_slot_stride, a.dst_slot_stride, a.src_row_pitch, a.dst_row_pitch = self.ss, self.ds, self.sp, self.dp
        a.rows, a.row_bytes = self.rows, self.rb

    def expected(self, src_list, src_slots, dst_list, dst_slots, n):
        out = self.dst0.clone()
        for j in range(n):
            s = j if src_list is None else src_list[j]
            d = j if dst_list is None else dst_list[j]
            if not (0 <= s < src_slots and 0 <= d < dst_slots):
                continue
            for r in range(self.rows):
                so, do = GUARD + s * self.ss + r * self.sp, GUARD + d * self.ds + r * self.dp
                out[do:do + self.rb] = self.src[so:so + self.rb]
        return out


def _launch(table, nseg, src_list, src_slots, dst_list, dst_slots, n, max_bytes, src_off=0, dst_off=0):
    from mmt_amd._lib import LIB, check
    sp = None if src_list is None else src_list.data_ptr() + 4 * src_off
    dp = None if dst_list is None else dst_list.data_ptr() + 4 * dst_off
    check(LIB.mmt_slot_copy(table.data_ptr(), nseg, sp, src_slots, dp, dst_slots, n, max_bytes,
                            torch.cuda.current_stream().cuda_stream), "mmt_slot_copy")


def _table(segs):
    from mmt_amd._lib import SlotCopySeg
    arr = (SlotCopySeg * len(segs))()
    for a, s in zip(arr, segs):
        s.fill(a)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()


def _dev_list(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32).cuda()


# n = 5 entries, 4 source slots, 6 destination slots.  Entry 1 has a -1, entry 2 the out-of-range destination
# 6, entry 3 the out-of-range source 4: those three write nothing.
LISTS = {
    "both": ([2, -1, 0, 4, 3], [5, 1, 6, 2, 0]),
    "neg_dst": ([2, 1, 0, 3, 3], [5, -1, 6, -7, 0]),
    "null_src": (None, [3, -1, 0, 5, 1]),      # entry j reads slot j; entry 4 is past the 4 source slots
    "null_dst": ([1, 3, -1, 0, 4], None),      # entry j writes slot j
}


@pytest.mark.parametrize("case", sorted(LISTS))
def test_two_segments_lists_and_guards(case):
    src_list, dst_list = LISTS[case]
    n, S, D = 5, 4, 6
    segs = [_Seg(3, 16, 32, 48, 3 * 32 + 16, 3 * 48 + 32, S, D, seed=1),
            _Seg(5, 48, 64, 80, 5 * 64 + 32, 5 * 80 + 16, S, D, seed=2)]
    _launch(_table(segs), 2, _dev_list(src_list), S, _dev_list(dst_list), D, n, 5 * 48)
    torch.cuda.synchronize()
    for i, s in enumerate(segs):
        exp = s.expected(src_list, S, dst_list, D, n)
        assert not torch.equal(exp, s.dst0)  # the case copies something
        assert torch.equal(s.dst_dev.cpu(), exp), (case, i)


def test_grid_smaller_than_the_segment():
    """max_seg_bytes below the largest segment: fewer workgroups loop over it, the result is the same."""
    S = D = 3
    seg = _Seg(37, 4096, 4096 + 16, 4096 + 32, 37 * (4096 + 16) + 48, 37 * (4096 + 32), S, D, seed=3)
    src_list = [2, 0, 1]
    _launch(_table([seg]), 1, _dev_list(src_list), S, None, D, 3, 16 * 1024)  # one workgroup per entry
    torch.cuda.synchronize()
    assert torch.equal(seg.dst_dev.cpu(), seg.expected(src_list, S, None, D, 3))


def test_130_entries_equal_single_launches():
    n, S, D = 130, 140, 150
    g = torch.Generator().manual_seed(4)
    src_list = torch.randperm(S, generator=g)[:n].tolist()
    dst_list = torch.randperm(D, generator=g)[:n].tolist()
    for j in (7, 64, 129):
        src_list[j] = -1
    dst_list[100] = D
    mk = lambda: [_Seg(3, 16, 32, 48, 112, 176, S, D, seed=5), _Seg(5, 48, 64, 80, 352, 416, S, D, seed=6)]  # noqa: E731
    one, many = mk(), mk()
    sl, dl = _dev_list(src_list), _dev_list(dst_list)
    _launch(_table(one), 2, sl, S, dl, D, n, 240)
    tab = _table(many)
    for j in range(n):
        _launch(tab, 2, sl, S, dl, D, 1, 240, src_off=j, dst_off=j)
    torch.cuda.synchronize()
    for a, b in zip(one, many):
        exp = a.expected(src_list, S, dst_list, D, n)
        assert torch.equal(a.dst_dev.cpu(), exp)
        assert torch.equal(b.dst_dev.cpu(), exp)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_kv_columns_of_qkv_rows(dtype):
    """The cache's real segment: the K and V columns [C, 3C) of the first 2 rows of each slot's [ntok][3C]
    block, C = 768, 2-byte and 4-byte elements, compact 2-slot side -> 3-slot side by a slot list."""
    from mmt_amd._lib import SlotCopySeg
    C, ntok, rows, Dn, N = 768, 4, 2, 2, 3
    g = torch.Generator().manual_seed(8)
    src = torch.randn(Dn, ntok, 3 * C, generator=g).to(dtype).cuda()
    dst0 = torch.randn(N, ntok, 3 * C, generator=g).to(dtype)
    dst = dst0.cuda()
    es = src.element_size()
    seg = SlotCopySeg()
    seg.src, seg.dst = src.data_ptr() + C * es, dst.data_ptr() + C * es
    seg.src_slot_stride = seg.dst_slot_stride = ntok * 3 * C * es
    seg.src_row_pitch = seg.dst_row_pitch = 3 * C * es
    seg.rows, seg.row_bytes = rows, 2 * C * es
    tab = torch.frombuffer(bytearray(bytes(seg)), dtype=torch.uint8).cuda()
    slots = [2, 0]
    _launch(tab, 1, None, Dn, _dev_list(slots), N, Dn, rows * 2 * C * es)
    torch.cuda.synchronize()
    exp = dst0.clone()
    exp[slots, :rows, C:] = src.cpu()[:, :rows, C:]
    bits = torch.int16 if es == 2 else torch.int32
    assert torch.equal(dst.cpu().view(bits), exp.view(bits))
    assert ctypes.sizeof(SlotCopySeg) == 56
