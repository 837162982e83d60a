"""The batched tracker with the per-slot template K/V cache (RGBTBatchTrackerCore(slot_cache=True)), fp32
HIP path: the loop of tests/test_gpu_batch_tracker.py -- same sequences, same oracle slots, same bars (crops
and the box update bit-exact, boxes within 1e-3 * 320 / resize_factor px of the oracle's teacher-forced host
loop, scores within 1e-3) -- with the search-only pass per step and a template pass over the dirty slots only.

Dirty rules, counted through core.refresh_replays: `assign` dirties its slot, a plain tracker's online
template re-crop and the online-score tracker's promotion dirty theirs, a candidate crop alone does not,
`release` clears the mark; a step refreshes ceil(dirty / refresh_slots) times before its graph, a step with
no dirty slot not at all."""
import math

import pytest
import torch

from test_gpu_batch_tracker import THREE, _batch_tracker, _OracleSlot, _seq, _start, _step, _synth_sd

pytestmark = pytest.mark.gpu


def _template_rows(core):
    """Every layer's template rows of the N-slot cache, [mod][slot][n_t][3C] (and KV1 [slot][n_t][2C])."""
    rt, ws, N = core._rt, core._sc["ws"], core.slots
    d = rt.d
    rows = [q.view(d.nmod, N, d.ntok, 3 * d.C)[:, :, :d.n_t].clone() for q in ws["QKVL"]]
    if "KV1" in ws:
        rows.append(ws["KV1"].view(1, N, d.n_t, 2 * d.C).clone())
    return rows


@pytest.mark.parametrize("variant,multimodal", [("shared", False), ("asym", True)])
def test_cached_tracking_loop_matches_oracle(variant, multimodal):
    """3 slots, interval [3], 5 frames: three assigns cost one refresh (capacity min(8, 3) = 3), frames 2 and 3
    none, the frame after the update one; one step graph throughout."""
    trk, sd = _batch_tracker(variant, 3, slot_cache=True)
    core = trk.core
    assert core.slot_cache and core.refresh_slots == 3
    slots = _start(trk, sd, variant, multimodal, THREE, 5)
    assert core.refresh_replays == 0  # lazily: nothing runs before the first track
    graph, counts = None, []
    for _ in range(4):
        _step(trk, slots)
        graph = graph or core._graph
        assert graph is not None and core._graph is graph
        counts.append(core.refresh_replays)
    assert counts == [1, 1, 1, 2]  # frames 1-3 on the assigned templates; frame 3 re-cropped every online template
    assert all(s.updates == 1 for s in slots.values())


@pytest.mark.parametrize("lift", [0.25, 0.0])
def test_cached_online_score_staggered(lift):
    """asymmetric_shared_online, 2 slots one step apart (tests/test_gpu_batch_tracker.py's staggered start):
    promotions dirty a slot, candidate crops do not."""
    sd = _synth_sd("asym_online")
    key = "score_branch.score_head.layers.2.bias"
    sd[key] = sd[key] + lift
    trk, sd = _batch_tracker("asym_online", 2, sd=sd, slot_cache=True)
    core = trk.core
    D = core.refresh_slots
    assert D == 2
    specs = [dict(seed=0), dict(seed=5, x0=180, y0=140)]
    seqs = [_seq(7, **kw) for kw in specs]
    slots, live, dirty, expected = {}, {}, set(), 0
    crop_only_steps = 0
    for step in range(7):
        if step < 2:
            frames, init = seqs[step]
            trk.initialize(step, frames[0], {"init_bbox": [init, init]})
            slots[step] = live[step] = _OracleSlot(sd, "asym_online", True, frames, init, score=True)
            slots[step].check_templates(core, step)
            dirty.add(step)
        for b in [b for b, s in live.items() if s.f + 1 == len(s.frames)]:
            trk.release(b)
            del live[b]
            dirty.discard(b)
        expected += math.ceil(len(dirty) / D)
        dirty.clear()
        took = {b: s.took for b, s in live.items()}
        _step(trk, live)
        assert core.refresh_replays == expected, (step, core.refresh_replays, expected)
        for b, s in live.items():
            if s.f % 3 == 0:  # the schedule promoted the slot's candidate
                dirty.add(b)
        # a candidate crop on a frame without a promotion leaves every slot clean
        if any(s.took > took[b] and s.f % 3 for b, s in live.items()) and not any(s.f % 3 == 0 for s in live.values()):
            assert not core._dirty
            crop_only_steps += 1
    assert all(s.f == 6 for s in slots.values()) and all(s.updates >= 1 for s in slots.values())
    if lift:
        assert all(s.took > 0 for s in slots.values()) and crop_only_steps > 0
    else:
        assert not any(s.took for s in slots.values())
    assert 0 < core.refresh_replays < 7 + 6  # fewer refreshes than slot-steps


def test_refresh_capacity_one_chunks_the_dirty_slots():
    """refresh_slots = 1: two assigns before the first track are two replays, the two slots re-cropped on frame
    3 two more; the steps between launch no refresh."""
    trk, sd = _batch_tracker("shared", 2, slot_cache=True, refresh_slots=1)
    core = trk.core
    slots = _start(trk, sd, "shared", False, THREE[:2], 5)
    counts = []
    for _ in range(4):
        _step(trk, slots)
        counts.append(core.refresh_replays)
    assert counts == [2, 2, 2, 4]
    assert core._sc["slots"].tolist() == [1]  # the last chunk held the higher slot: ascending order


def test_slot_reuse_refreshes_only_that_slot():
    """Slot 1 is released and takes a 97x131 sequence: one refresh with the list [1, -1]; the other slots' cache
    rows are bitwise unchanged and the step graph and the refresh graph are the same objects."""
    trk, sd = _batch_tracker("shared", 3, slot_cache=True, refresh_slots=2)
    core = trk.core
    slots = _start(trk, sd, "shared", False, THREE, 4)
    _step(trk, slots)
    assert core.refresh_replays == 2  # ceil(3 assigns / 2)
    graph, rgraph = core._graph, core._sc["graph"]
    assert graph is not None and rgraph is not None
    before = _template_rows(core)
    trk.release(1)
    frames, init = _seq(2, H=97, W=131, x0=40, y0=30, side=24, seed=3)
    trk.initialize(1, frames[0], {"init_bbox": [init, init]})
    slots[1] = _OracleSlot(sd, "shared", False, frames, init)
    slots[1].check_templates(core, 1)
    _step(trk, slots)
    assert core.refresh_replays == 3 and core._sc["slots"].tolist() == [1, -1]
    after = _template_rows(core)
    for a, b in zip(after, before):
        assert torch.equal(a[:, [0, 2]].view(torch.uint8), b[:, [0, 2]].view(torch.uint8))
    assert any(not torch.equal(a[:, 1], b[:, 1]) for a, b in zip(after, before))
    assert core._graph is graph and core._sc["graph"] is rgraph
    # a slot released while dirty is not refreshed: release, assign, release, step
    trk.release(1)
    trk.initialize(1, frames[0], {"init_bbox": [init, init]})
    trk.release(1)
    del slots[1]
    _step(trk, slots)
    assert core.refresh_replays == 3


def test_cached_boxes_match_uncached_and_reload_marks_all_dirty():
    """Two batched trackers, same weights and frames, with and without the cache: boxes within the oracle bar
    1e-3 * 320 / resize_factor px at every step (not bitwise: the compact passes' GEMMs may tile differently).
    A weight reload re-plans and refreshes every active slot."""
    trk_c, sd = _batch_tracker("asym", 3, slot_cache=True, refresh_slots=2)
    trk_u, _ = _batch_tracker("asym", 3, sd=sd)
    seqs = [_seq(6, **kw) for kw in THREE]
    for b, (frames, init) in enumerate(seqs):
        for trk in (trk_c, trk_u):
            trk.initialize(b, frames[0], {"init_bbox": [init, init]})
    for f in range(1, 6):
        if f == 5:  # the network drops its runtime, as after load_state_dict: new weights buffers, new cache
            trk_c.network.refresh_kernels()
            trk_u.network.refresh_kernels()  # the uncached core re-plans too, and refreshes nothing
            before = trk_c.core.refresh_replays
        images = {b: seqs[b][0][f] for b in range(3)}
        out_c, out_u = trk_c.track(images), trk_u.track(images)
        rf = trk_u.core.search_crop[:, 0, 3].tolist()
        for b in range(3):
            tol = 1e-3 * 320 / rf[b]
            err = max(abs(x - y) for x, y in zip(out_c[b]["target_bbox"], out_u[b]["target_bbox"]))
            print("frame %d slot %d cached vs uncached %.3g px (tol %.3g)" % (f, b, err, tol))
            assert err <= tol, (f, b)
    assert trk_c.core.refresh_replays == before + 2  # three active slots, capacity 2
    assert trk_u.core.refresh_replays == 0 and not trk_u.core.slot_cache


def test_slot_cache_refuses_candidate_elimination():
    from lib.test.tracker import asymmetric_shared_ce
    from test_gpu_batch_tracker import _params
    params = _params()
    params.slot_cache = True
    with pytest.raises(NotImplementedError):
        asymmetric_shared_ce.get_batch_tracker_class()(params, "synth", 2)
