"""Host side of the batched multi-sequence tracker (no GPU): the two C-ABI entry points exist and
reject every host-checkable bad argument before any launch, track_sequences' slot bookkeeping against
a stand-in core that records its calls, and the per-slot template schedule against the rule of
RGBTTrackerCore.track (restated here as the single tracker's loop over host counters)."""
import ctypes

import pytest

EBADARG = -10000


# ------------------------------------------------------------------ C ABI
def test_symbols_exported():
    from mmt_amd import _lib
    for name in ("mmt_sample_target_table", "mmt_track_update_slots"):
        assert name in _lib.EXPORTED
        assert getattr(_lib.LIB, name) is not None


def test_sample_target_table_rejects_bad_args():
    from mmt_amd._lib import LIB, CropParams
    tab = (CropParams * 2)()  # a non-NULL pointer; a rejected call never reads it
    p = ctypes.addressof(tab)
    assert LIB.mmt_sample_target_table(None, None, 2, 320, None) == EBADARG
    assert LIB.mmt_sample_target_table(p, None, 0, 320, None) == EBADARG
    assert LIB.mmt_sample_target_table(p, None, -3, 320, None) == EBADARG
    assert LIB.mmt_sample_target_table(p, None, 2, 0, None) == EBADARG
    assert LIB.mmt_sample_target_table(p, None, 2, -128, None) == EBADARG


def test_track_update_slots_rejects_bad_args():
    from mmt_amd._lib import LIB
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ok = dict(pred=p, crop=p, stride=8, state=p, hw=p, active=None, n=2, ss=320)

    def call(**kw):
        a = dict(ok, **kw)
        return LIB.mmt_track_update_slots(a["pred"], a["crop"], a["stride"], a["state"], a["hw"], a["active"], a["n"],
                                          a["ss"], 10.0, None)

    assert call(state=None) == EBADARG
    assert call(pred=None) == EBADARG
    assert call(crop=None) == EBADARG
    assert call(hw=None) == EBADARG
    assert call(n=0) == EBADARG
    assert call(n=-1) == EBADARG
    assert call(ss=0) == EBADARG
    assert call(stride=3) == EBADARG
    assert call(stride=0) == EBADARG


# ------------------------------------------------------------------ track_sequences
class StandInCore:
    """Records assign / release / track; a frame is the tuple (name, index); a box is [slot, index, 0, 0].
    fail_at: {(name, index)}: track reports a failure for that frame and releases the slot, as the
    real core does."""

    def __init__(self, slots, fail_at=()):
        self.slots = slots
        self.active = {}  # slot -> name
        self.log = []
        self.fed = {}  # name -> [(slot, frame)]
        self.fail_at = set(fail_at)

    def assign(self, slot, image, init_bbox):
        assert 0 <= slot < self.slots
        assert slot not in self.active, "slot %d reused before release" % slot
        self.log.append(("assign", slot, image))
        self.active[slot] = image[0]
        self.fed.setdefault(image[0], []).append((slot, image))

    def release(self, slot):
        self.log.append(("release", slot))
        self.active.pop(slot, None)

    def track(self, images):
        assert set(images) == set(self.active), "track must name exactly the active slots"
        self.log.append(("track", dict(images)))
        out = {}
        for slot, frame in images.items():
            assert frame[0] == self.active[slot]
            self.fed[frame[0]].append((slot, frame))
            if frame in self.fail_at:
                self.release(slot)
                out[slot] = Exception("Too small bounding box.")
            else:
                out[slot] = [float(slot), float(frame[1]), 0.0, 0.0]
        return out


LENGTHS = {"a": 1, "b": 2, "c": 4, "d": 4, "e": 7}


def _sequences():
    return [(name, iter([(name, i) for i in range(n)]), [1.0, 2.0, 3.0, 4.0]) for name, n in LENGTHS.items()]


def test_track_sequences_keeps_slots_full():
    from mmt_amd.tracking import track_sequences
    core = StandInCore(2)
    res = track_sequences(core, _sequences())
    assert sorted(res) == sorted(LENGTHS)
    for name, n in LENGTHS.items():
        fed = core.fed[name]
        assert [f for _, f in fed] == [(name, i) for i in range(n)]  # exactly its frames, in order
        assert len({s for s, _ in fed}) == 1  # in one slot
        slot = fed[0][0]
        assert res[name].error is None
        assert list(res[name]) == [[1.0, 2.0, 3.0, 4.0]] + [[float(slot), float(i), 0.0, 0.0] for i in range(1, n)]
    assert not core.active  # every slot released at the end
    # both slots are busy for as long as a sequence is waiting: every step before the last assign has two
    last_assign = max(i for i, e in enumerate(core.log) if e[0] == "assign")
    tracks = [(i, e[1]) for i, e in enumerate(core.log) if e[0] == "track"]
    assert tracks and all(len(im) == 2 for i, im in tracks if i < last_assign)


def test_track_sequences_failure_is_isolated():
    from mmt_amd.tracking import track_sequences
    core = StandInCore(2, fail_at={("c", 2)})
    res = track_sequences(core, _sequences())
    assert isinstance(res["c"].error, Exception) and "Too small" in str(res["c"].error)
    assert len(res["c"]) == 2  # the init box and frame 1
    assert [f for _, f in core.fed["c"]] == [("c", 0), ("c", 1), ("c", 2)]  # nothing fed after the failure
    for name, n in LENGTHS.items():
        if name != "c":
            assert res[name].error is None and len(res[name]) == n
    assert not core.active


def test_track_sequences_assign_failure_and_empty_sequence():
    from mmt_amd.tracking import track_sequences

    class Core(StandInCore):
        def assign(self, slot, image, init_bbox):
            if image[0] == "b":
                raise Exception("Too small bounding box.")
            super().assign(slot, image, init_bbox)

    core = Core(2)
    seqs = _sequences() + [("empty", iter([]), [0.0, 0.0, 1.0, 1.0])]
    res = track_sequences(core, seqs)
    assert res["b"].error is not None and list(res["b"]) == []
    assert list(res["empty"]) == [] and res["empty"].error is None
    for name in "acde":
        assert len(res[name]) == LENGTHS[name] and res[name].error is None


# ------------------------------------------------------------------ template schedule
def _single_core_rule(online_score, intervals, scores):
    """RGBTTrackerCore.track's decisions over host counters: per frame (cropped, promoted, max_pred_score)."""
    out, max_pred, frame_id = [], -1.0, 0
    for p in scores:
        frame_id += 1
        cropped = promoted = 0
        if online_score:
            if p > 0.5 and p > max_pred:
                cropped, max_pred = 1, p
            for i in intervals:
                if frame_id % i == 0:
                    promoted += 1
                    max_pred = -1
        else:
            for i in intervals:
                if frame_id % i == 0:
                    cropped = 1
        out.append((bool(cropped), promoted, max_pred))
    return out


@pytest.mark.parametrize("online_score,intervals,scores", [
    (False, [3], [None] * 7),
    (True, [3], [0.4, 0.6, 0.55, 0.7, 0.3, 0.9]),
    (True, [2, 3], [0.4, 0.6, 0.55, 0.7, 0.3, 0.9]),  # both intervals on frame 6
])
def test_template_schedule_matches_single_core(online_score, intervals, scores):
    from mmt_amd.tracking import template_schedule
    ref = _single_core_rule(online_score, intervals, scores)
    max_pred, got = -1.0, []
    for f, p in enumerate(scores, 1):
        c, pr, max_pred = template_schedule(online_score, f, intervals, p, max_pred)
        got.append((c, pr, max_pred))
    assert got == ref
    if online_score and intervals == [3]:
        # frame 2 opens the gate, 3 does not beat it and promotes, 4 opens again, 6 opens and promotes
        assert [g[0] for g in got] == [False, True, False, True, False, True]
        assert [g[1] for g in got] == [0, 0, 1, 0, 0, 1]
    if not online_score:
        assert [g[0] for g in got] == [False, False, True, False, False, True, False]
