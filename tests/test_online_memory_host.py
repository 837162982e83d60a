"""Host side of the online template memory (no GPU): the schedule function against a transliteration of
upstream lib/test/tracker/mixformer_vit_online.py:107-129, and the refusals of the runtime, the modules and
the trackers."""
import random
from types import SimpleNamespace

import pytest
import torch


def _upstream(scores, interval_list, online_size, decay):
    """Upstream's track() bookkeeping, statement for statement, with the online templates as a list of labels
    ("T" the template, ("C", frame) the crop of that frame); one list of intervals is upstream's one interval
    applied once per entry, as the RGB-T trackers' loops do.  Yields (cropped, online templates) per frame."""
    online_template = ["T"]  # :68 self.online_template = template
    max_pred_score, online_max_template, online_forget_id = -1.0, "T", 0
    for frame_id, pred_score in enumerate(scores, 1):
        max_pred_score = max_pred_score * decay
        cropped = False
        if pred_score > 0.5 and pred_score > max_pred_score:
            online_max_template = ("C", frame_id)
            max_pred_score = pred_score
            cropped = True
        for update_interval in interval_list:
            if frame_id % update_interval == 0:
                if online_size == 1:
                    online_template = [online_max_template]
                elif len(online_template) < online_size:
                    online_template = online_template + [online_max_template]
                else:
                    online_template[online_forget_id:online_forget_id + 1] = [online_max_template]
                    online_forget_id = (online_forget_id + 1) % online_size
                max_pred_score = -1
                online_max_template = "T"
        yield cropped, list(online_template)


@pytest.mark.parametrize("decay", [1.0, 0.98, 0.5])
@pytest.mark.parametrize("intervals", [[2], [3], [1], [2, 3], [4, 2], [200]])
@pytest.mark.parametrize("K", [1, 2, 3, 5])
def test_schedule_matches_upstream(K, intervals, decay):
    from mmt_amd.tracking import online_memory_schedule
    rng = random.Random(17 * K + 5 * len(intervals) + intervals[0])
    for stream in range(6):
        lo = (0.0, 0.3, 0.45)[stream % 3]  # mostly under the gate, around it, mostly over it
        scores = [min(1.0, lo + rng.random() * 0.7) for _ in range(40)]
        memory, online, cand = (1, 0, -1.0), ["T"], "T"
        for frame_id, (score, (want_crop, want_online)) in enumerate(zip(scores, _upstream(scores, intervals, K, decay)), 1):
            crop, writes, memory = online_memory_schedule(frame_id, intervals, score, memory, K, decay)
            assert crop == want_crop, (stream, frame_id)
            if crop:
                cand = ("C", frame_id)
            for j, slot in enumerate(writes):  # what both cores do with the result
                assert slot <= len(online) and slot < K
                img = cand if j == 0 else "T"
                if slot == len(online):
                    online.append(img)
                else:
                    online[slot] = img
            if writes:
                cand = "T"
            assert online == want_online and memory[0] == len(online), (stream, frame_id)
            assert len(writes) == sum(frame_id % i == 0 for i in intervals)


@pytest.mark.parametrize("intervals", [[2], [3, 6], [5]])
def test_size_one_without_decay_is_template_schedule(intervals):
    from mmt_amd.tracking import online_memory_schedule, template_schedule
    rng = random.Random(3)
    memory, best = (1, 0, -1.0), -1.0
    for frame_id in range(1, 60):
        score = rng.random()
        crop, writes, memory = online_memory_schedule(frame_id, intervals, score, memory, 1)
        c, p, best = template_schedule(True, frame_id, intervals, score, best)
        assert (bool(crop), writes, memory) == (bool(c), [0] * p, (1, 0, best))


def test_tracker_arguments():
    from lib.test.tracker._rgbt import _online_memory
    from mmt_amd.tracking import RGBTBatchTrackerCore, RGBTTrackerCore, check_online_memory
    assert check_online_memory(1, 1.0, False) == (1, 1.0) and check_online_memory(3, 0.98, True) == (3, 0.98)
    assert _online_memory(SimpleNamespace(), False) == {"online_size": 1, "max_score_decay": 1.0}
    assert _online_memory(SimpleNamespace(online_size=3, max_score_decay=0.9), True) == {"online_size": 3, "max_score_decay": 0.9}
    for bad in (dict(online_size=3), dict(max_score_decay=0.9)):  # the plain trackers have no ring
        with pytest.raises(ValueError, match="plain trackers"):
            _online_memory(SimpleNamespace(**bad), False)
    for K, decay in ((0, 1.0), (2.5, 1.0), (3, 0.0), (3, 1.5)):
        with pytest.raises(ValueError):
            check_online_memory(K, decay, True)
    net1, net3 = SimpleNamespace(online_size=1), SimpleNamespace(online_size=3, variant="asym_online")
    args = (2.0, 128, 5.0, 320, [2], True)
    with pytest.raises(ValueError, match="set_online_size"):  # the network must be built for the same size
        RGBTTrackerCore(net1, *args, online_score=True, online_size=3)
    with pytest.raises(ValueError, match="plain trackers"):
        RGBTTrackerCore(net3, *args, online_score=False, online_size=3)
    with pytest.raises(ValueError, match="plain trackers"):
        RGBTBatchTrackerCore(net3, *args, online_score=False, slots=2, online_size=3)
    with pytest.raises(ValueError, match="pack"):
        RGBTBatchTrackerCore(net3, *args, online_score=True, slots=4, pack="auto", online_size=3)


@pytest.mark.parametrize("variant", ["asym_ce", "rgb"])
def test_runtime_refuses_the_variants_without_a_memory(variant):
    from mmt_amd.runtime import MixFormerRGBTRuntime
    with pytest.raises(NotImplementedError, match="online_size"):
        MixFormerRGBTRuntime({}, variant, dtype=torch.float16, online_size=3)


@pytest.mark.parametrize("bad", [0, -1, 1.5])
def test_runtime_refuses_a_bad_size(bad):
    from mmt_amd.runtime import MixFormerRGBTRuntime
    with pytest.raises(ValueError, match="online_size"):
        MixFormerRGBTRuntime({}, "asym_online", online_size=bad)


def test_dims_follow_online_size():
    from mmt_amd.runtime import Dims
    import json
    from conftest import GOLDEN
    shapes = dict(json.load(open(GOLDEN + "/state_dict_asym_online.json")))
    sd = {k: torch.empty(tuple(v), device="meta") for k, v in shapes.items()}
    d1, d3 = Dims(sd, "asym_online"), Dims(sd, "asym_online", 3)
    assert (d1.n_t, d1.ntok, d1.n_kv1) == (2 * d1.nt1, 2 * d1.nt1 + d1.ns, 2 * d1.nt1)
    assert (d3.n_t, d3.ntok, d3.n_kv1) == (4 * d3.nt1, 4 * d3.nt1 + d3.ns, 2 * d3.nt1)


def test_modules_refuse_what_is_not_implemented():
    from mmt_amd.model import build_asymmetric_shared_ce, build_asymmetric_shared_online_score, hot_path_cfg
    ce = build_asymmetric_shared_ce(hot_path_cfg(), train=False)
    with pytest.raises(NotImplementedError, match="online_size"):
        ce.set_online_size(3)
    assert ce.set_online_size(1).online_size == 1
    model = build_asymmetric_shared_online_score(hot_path_cfg(), train=False)
    with pytest.raises(ValueError):
        model.set_online_size(0)
    x = [torch.zeros(1, 3, 8, 8)] * 2
    with pytest.raises(ValueError, match="online_count"):  # belongs to online_size > 1
        model.eval()._online_kw([1])
    model.set_online_size(3).train()
    with pytest.raises(NotImplementedError, match="training"):
        model(x, x, x)
