"""Host side of the batched tracker's packed step (no GPU): the rung ladder and choice, the padded slot
list, and the two list-indexed C-ABI entry points (mmt_sample_target_packed, mmt_track_update_packed):
exported, declared, and rejecting every host-checkable bad argument before any launch."""
import ctypes
import os

import pytest

EBADARG = -10000
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmt_hip.h")


# ------------------------------------------------------------------ rungs
def test_auto_ladder():
    from mmt_amd.tracking import pack_rungs
    assert pack_rungs("auto", 64) == (1, 2, 4, 8, 16, 32)
    assert pack_rungs("auto", 6) == (1, 3)  # 6 // 2, 6 // 4
    assert pack_rungs("auto", 1) == ()  # nothing below one slot: off
    assert pack_rungs(None, 64) == () and pack_rungs((), 64) == ()
    assert pack_rungs((8, 1, 32), 64) == (1, 8, 32)
    assert pack_rungs([63], 64) == (63,)


def test_rung_choice():
    from mmt_amd.tracking import choose_rung, pack_rungs
    rungs = pack_rungs((2, 8, 32), 64)
    assert [choose_rung(rungs, n) for n in (1, 2, 3, 8, 9, 32)] == [2, 2, 8, 8, 32, 32]
    assert choose_rung(rungs, 33) is None and choose_rung(rungs, 64) is None  # past the largest: the full step
    assert choose_rung((), 1) is None
    assert choose_rung(pack_rungs((2, 1), 4), 3) is None
    assert choose_rung(pack_rungs("auto", 64), 5) == 8


@pytest.mark.parametrize("bad", [(4,), (5,), (0,), (-1,), (2, 2), "full", "", (1.5,), 3, (True,)])
def test_bad_pack_raises(bad):
    from mmt_amd.tracking import RGBTBatchTrackerCore, pack_rungs
    with pytest.raises(ValueError):
        pack_rungs(bad, 4)
    with pytest.raises(ValueError):  # at construction, before anything touches the GPU
        RGBTBatchTrackerCore(None, 2.0, 128, 5.0, 320, [3], multimodal=False, slots=4, pack=bad)


def test_list_is_padded_with_minus_one():
    from mmt_amd.tracking import pack_list
    assert pack_list([5, 1], 4) == [1, 5, -1, -1]
    assert pack_list([3], 1) == [3]
    assert pack_list([], 2) == [-1, -1]
    assert pack_list([0, 1, 2], 3) == [0, 1, 2]
    with pytest.raises(ValueError):
        pack_list([0, 1, 2], 2)


# ------------------------------------------------------------------ C ABI
def test_symbols_exported_and_declared():
    from mmt_amd import _lib
    text = open(HEADER).read()
    for name in ("mmt_sample_target_packed", "mmt_track_update_packed"):
        assert name in _lib.EXPORTED
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
        assert "int %s(" % name in text


def test_sample_target_packed_rejects_bad_args():
    from mmt_amd._lib import LIB, CropParams
    tab = (CropParams * 4)()  # non-NULL pointers; a rejected call never reads them
    buf = (ctypes.c_float * 16)()
    lst = (ctypes.c_int32 * 4)()
    ok = dict(tab=ctypes.addressof(tab), en=None, lst=ctypes.addressof(lst), n=2, slots=2, per=2, osz=16,
              out=ctypes.addressof(buf), ms=2 * 768, rs=768)

    def call(**kw):
        a = dict(ok, **kw)
        return LIB.mmt_sample_target_packed(a["tab"], a["en"], a["lst"], a["n"], a["slots"], a["per"], a["osz"], a["out"],
                                            a["ms"], a["rs"], None)

    for kw in (dict(tab=None), dict(lst=None), dict(out=None), dict(n=0), dict(n=-2), dict(slots=0), dict(slots=-1),
               dict(per=0), dict(per=-1), dict(per=5), dict(osz=0), dict(osz=-16), dict(ms=-1), dict(rs=-768),
               dict(n=2 ** 31 - 1, per=1, osz=17),  # 2 tiles per crop: the grid passes 2^31 - 1 blocks
               dict(n=2 ** 30, per=2, osz=16)):  # 2^31 blocks
        assert call(**kw) == EBADARG, kw


def test_track_update_packed_rejects_bad_args():
    from mmt_amd._lib import LIB
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ok = dict(pred=p, crop=p, stride=8, state=p, hw=p, active=None, lst=p, n=2, slots=4, ss=320)

    def call(**kw):
        a = dict(ok, **kw)
        return LIB.mmt_track_update_packed(a["pred"], a["crop"], a["stride"], a["state"], a["hw"], a["active"], a["lst"],
                                           a["n"], a["slots"], a["ss"], 10.0, None)

    for kw in (dict(pred=None), dict(crop=None), dict(state=None), dict(hw=None), dict(lst=None), dict(n=0), dict(n=-1),
               dict(slots=0), dict(slots=-3), dict(ss=0), dict(stride=3), dict(stride=0)):
        assert call(**kw) == EBADARG, kw
