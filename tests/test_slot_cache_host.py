"""Host side of the per-slot template K/V cache (no GPU): the mmt_slot_copy entry point's export, struct
layout and argument checks, the refresh list chunking, and the batched tracker's kv_cache refusal."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mmt_hip.h")
EBADARG = -10000


def test_slot_copy_exported_and_declared():
    from mmt_amd import _lib
    assert "mmt_slot_copy" in _lib.EXPORTED
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mmt_slot_copy")
    assert "int mmt_slot_copy(" in open(HEADER).read()


def test_slot_copy_seg_layout_matches_header(tmp_path):
    from mmt_amd import _lib
    fields = [f for f, _ in _lib.SlotCopySeg._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HEADER, "int main(void){",
           'printf("%zu\\n", sizeof(mmt_slot_copy_seg));']
    src += ['printf("%%zu\\n", offsetof(mmt_slot_copy_seg, %s));' % f for f in fields]
    src += ["return 0;}"]
    c = tmp_path / "seg.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "seg"
    subprocess.check_call(["gcc", str(c), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out[0] == ctypes.sizeof(_lib.SlotCopySeg) == 56
    assert out[1:] == [getattr(_lib.SlotCopySeg, f).offset for f in fields]


def test_slot_copy_rejects_bad_arguments_before_any_launch():
    from mmt_amd._lib import LIB
    fake = 1 << 20  # 16-B aligned, never dereferenced
    good = dict(segs=fake, nseg=2, src=fake, src_slots=4, dst=fake, dst_slots=6, n=5, max_bytes=240)

    def call(**kw):
        a = dict(good, **kw)
        return LIB.mmt_slot_copy(a["segs"], a["nseg"], a["src"], a["src_slots"], a["dst"], a["dst_slots"], a["n"],
                                 a["max_bytes"], None)
    assert call(segs=None) == EBADARG
    assert call(nseg=0) == EBADARG and call(nseg=-1) == EBADARG
    assert call(n=0) == EBADARG and call(n=-3) == EBADARG
    assert call(src_slots=0) == EBADARG and call(dst_slots=0) == EBADARG
    assert call(src_slots=-1) == EBADARG and call(dst_slots=-2) == EBADARG
    assert call(src=None, dst=None) == EBADARG  # both lists NULL: 4 source slots against 6 destination slots
    # the grid's y / z limits, the size that sizes the grid, misaligned tables
    assert call(n=65536) == EBADARG and call(nseg=65536) == EBADARG
    assert call(max_bytes=0) == EBADARG and call(max_bytes=24) == EBADARG
    assert call(segs=fake + 4) == EBADARG and call(src=fake + 2) == EBADARG and call(dst=fake + 1) == EBADARG


def test_slot_chunks():
    from mmt_amd.runtime import slot_chunks
    assert slot_chunks([], 2) == []
    assert slot_chunks([4, 0, 3, 1, 2], 2) == [[4, 0], [3, 1], [2, -1]]  # order kept, the last list padded
    assert slot_chunks([2, 0], 2) == [[2, 0]]
    assert slot_chunks([1], 3) == [[1, -1, -1]]
    assert slot_chunks(range(64), 8) == [list(range(i, i + 8)) for i in range(0, 64, 8)]
    with pytest.raises(ValueError):
        slot_chunks([0], 0)


def test_batch_tracker_still_refuses_kv_cache():
    """kv_cache names the whole-batch template pass and stays refused; slot_cache is a keyword of its own."""
    import inspect

    from mmt_amd.tracking import RGBTBatchTrackerCore
    with pytest.raises(NotImplementedError, match="slot_cache"):
        RGBTBatchTrackerCore(None, 2.0, 128, 5.0, 320, [3], multimodal=False, kv_cache=True, slots=2)
    sig = inspect.signature(RGBTBatchTrackerCore.__init__).parameters
    assert sig["slot_cache"].default is False and sig["refresh_slots"].default is None


def test_cache_refusal_for_candidate_elimination():
    from mmt_amd.runtime import refuse_cache_with_ce
    refuse_cache_with_ce("asym")
    with pytest.raises(NotImplementedError):
        refuse_cache_with_ce("asym_ce")
