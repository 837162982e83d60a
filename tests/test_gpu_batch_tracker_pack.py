"""The batched tracker's packed step (RGBTBatchTrackerCore(pack=...)), fp32 HIP path, on the setup of
tests/test_gpu_batch_tracker.py: synthetic weights, small frames of differing sizes, the oracle's host loop
teacher-forced per slot at the same bars (crops and the box update bit-exact, boxes within
1e-3 * 320 / resize_factor px, scores within 1e-3).

A core of 4 slots with pack=(2, 1) on sequences of 6, 5, 3 and 2 frames: the steps run at batch 4, 4 (three
active: no rung), 2, 2 and 1.  Variants: `shared` plain, `shared` with the slot cache (refresh capacity 2; the
update interval 3 puts a refresh inside the packed phase) and `asym_online` (score gate and promotions)."""
import math

import pytest
import torch

from oracle import preprocess as pp
from test_gpu_batch_tracker import _batch_tracker, _OracleSlot, _seq, _synth_sd

pytestmark = pytest.mark.gpu

LENGTHS = [6, 5, 3, 2]
SPECS = [dict(H=120, W=160, x0=50, y0=40, side=24, seed=0), dict(H=97, W=131, x0=40, y0=30, side=24, seed=1),
         dict(H=120, W=160, x0=30, y0=50, side=28, seed=2), dict(H=144, W=176, x0=60, y0=50, side=24, seed=3)]
BATCHES = [4, 4, 2, 2, 1]
COUNTS = {4: 2, 2: 2, 1: 1}
CASES = {"shared": dict(variant="shared", multimodal=False), "shared-slot-cache": dict(variant="shared", multimodal=False,
                                                                                       slot_cache=True, refresh_slots=2),
         "asym_online": dict(variant="asym_online", multimodal=True, score=True)}


def _tracker(case, slots=4, pack=(2, 1), sd=None):
    c = CASES[case]
    if sd is None:
        sd = _synth_sd(c["variant"])
        if c.get("score"):  # the lift that opens the score gate (tests/test_gpu_batch_tracker.py)
            key = "score_branch.score_head.layers.2.bias"
            sd[key] = sd[key] + 0.25
    over = {k: min(v, slots) if k == "refresh_slots" else v for k, v in c.items() if k in ("slot_cache", "refresh_slots")}
    if pack is not None:
        over["pack_slots"] = pack
    return _batch_tracker(c["variant"], slots, sd=sd, **over)


class _Rows:
    """A rung's batch-R rows addressed by slot, as the oracle slot's checks address the batch-N buffers."""

    def __init__(self, t, row_of):
        self.t, self.row_of = t, row_of

    def __getitem__(self, k):
        if isinstance(k, slice):
            j = self.row_of[k.start]
            return self.t[j:j + 1]
        return self.t[self.row_of[k]]


class _PackedView:
    """The core as _OracleSlot.check_step reads it, after a packed step: search crops and BOX rows are the rung's."""

    def __init__(self, core, pk):
        row_of = {b: j for j, b in enumerate(pk["members"])}
        self.search = [_Rows(pk["search"][m], row_of) for m in range(2)]
        self._ws = {"BOX": _Rows(pk["ws"]["BOX"], row_of)}
        self._core = core

    def __getattr__(self, name):
        return getattr(self._core, name)


def _view(core, n_active):
    from mmt_amd.tracking import choose_rung
    R = choose_rung(core.pack, n_active)
    return core if R is None else _PackedView(core, core._packs[R])


@pytest.mark.parametrize("case", list(CASES))
def test_packed_loop_matches_oracle(case):
    c = CASES[case]
    trk, sd = _tracker(case)
    core = trk.core
    assert core.pack == (1, 2)
    live = {}
    for b, (n, kw) in enumerate(zip(LENGTHS, SPECS)):
        frames, init = _seq(n, **kw)
        trk.initialize(b, frames[0], {"init_bbox": [init, init]})
        live[b] = _OracleSlot(sd, c["variant"], c["multimodal"], frames, init, c.get("score", False))
        live[b].check_templates(core, b)
    slots = dict(live)
    batches, refreshes = [], []
    while live:
        n = len(live)
        before = core.refresh_replays
        out = trk.track({b: s.next_frame() for b, s in live.items()})
        assert sorted(out) == sorted(live)
        view = _view(core, n)
        batches.append(core.slots if view is core else view._ws["BOX"].t.shape[0])
        refreshes.append(core.refresh_replays - before)
        for b, s in live.items():
            s.check_step(view, b, out[b]["target_bbox"])
        if c.get("score") and view is not core:  # a packed step: NaN for the slots that did not run
            assert all(math.isnan(core.last_scores[b]) for b in range(4) if b not in live)
        for b in [b for b, s in live.items() if s.f + 1 == len(s.frames)]:
            trk.release(b)
            del live[b]
    assert batches == BATCHES
    assert core.step_counts == COUNTS
    assert sorted(core._packs) == [1, 2] and all(pk["graph"] is not None for pk in core._packs.values())
    assert slots[0].updates == 1 and slots[1].updates == 1  # frame 3: inside the packed phase
    if c.get("slot_cache"):
        # 4 assigns at capacity 2; frame 3 re-cropped the online templates of slots 0 and 1: one refresh before
        # the second step at batch 2
        assert refreshes == [2, 0, 0, 1, 0]
    if c.get("score"):
        # the two slots that reach the packed phase open the gate on frame 1 and, after the promotion of frame 3
        # reset their best score, again on frame 4: candidate crops and promotions inside packed steps
        assert slots[0].took >= 2 and slots[1].took >= 2


def _twin_step(case, sd, core, images, twins, make=None):
    """One packed step of `core` and the same step on a core of slots = R whose slot j is listed slot list[j]:
    same state, template buffers, frame and counters (slot cache: marked dirty).  Returns both results."""
    from mmt_amd.tracking import choose_rung
    act = core.active_slots()
    R = choose_rung(core.pack, len(act))
    if R not in twins:
        twins[R] = make(R) if make else _tracker(case, slots=R, pack=None, sd=sd)[0]
        twins[R].core.net = core.net  # one network: one runtime, one set of weight buffers, the same kernels
    twin = twins[R].core
    for j, b in enumerate(act):
        twin._load_frames(j, images[b])
        twin.state[j].copy_(core.state[b])
        for name in ("template", "online_template", "online_max_template"):
            for m in range(2):
                getattr(twin, name)[m][j].copy_(getattr(core, name)[m][b])
        twin.frame_id[j], twin.max_pred_score[j] = core.frame_id[b], core.max_pred_score[b]
        twin._set_active(j, True)
        if twin.slot_cache:
            twin._dirty.add(j)
    out = core.track(images)
    ref = twin.track({j: images[b] for j, b in enumerate(act)})
    return R, act, out, ref, twin


@pytest.mark.parametrize("case", list(CASES))
def test_packed_step_is_bitwise_the_small_core(case):
    """Same launches, same bits: a packed step at rung R and a core of slots = R run the same plan at batch R
    on the same inputs.  Plain and online score: bitwise.  Slot cache: bitwise as well, the twin refreshing its
    slots at the same capacity (at R = 1 the capacity is 1: min(refresh_slots, R))."""
    trk, sd = _tracker(case)
    core = trk.core
    seqs = [_seq(n, **kw) for n, kw in zip(LENGTHS, SPECS)]
    for b, (frames, init) in enumerate(seqs):
        trk.initialize(b, frames[0], {"init_bbox": [init, init]})
    twins, checked = {}, []
    for f in range(1, 6):
        for b in core.active_slots():
            if f >= LENGTHS[b]:
                trk.release(b)
        images = {b: seqs[b][0][f] for b in core.active_slots()}
        if len(images) > 2:
            core.track(images)
            continue
        R, act, out, ref, twin = _twin_step(case, sd, core, images, twins)
        for j, b in enumerate(act):
            assert out[b] == ref[j], (f, R, b, out[b], ref[j])  # lists of fp64: equal means the same bits
            assert torch.equal(core.state[b].view(torch.int64), twin.state[j].view(torch.int64))
            if core.online_score:
                assert core.last_scores[b] == twin.last_scores[j], (f, R, b)
        checked.append(R)
    assert checked == [2, 2, 1]


@pytest.mark.parametrize("case", list(CASES))
def test_padded_row_is_isolated(case):
    """1 slot active on rung 2: NaN in the padded row of the rung's inputs, in every activation of the rung's
    workspace and (slot cache) in the rung's cache rows leaves the active slot's box bitwise the same, and no
    inactive slot's state moves."""
    trk, sd = _tracker(case, pack=(2,))
    core = trk.core
    frames, init = _seq(3, **SPECS[1])
    trk.initialize(2, frames[0], {"init_bbox": [init, init]})
    for b in (0, 1, 3):  # inactive slots with a state worth watching
        core.state[b].copy_(torch.tensor([10.0 + b, 20.0, 30.0, 40.0], dtype=torch.float64))
    start = core.state.clone()

    def step():
        core.state.copy_(start)
        core.frame_id[2], core.max_pred_score[2] = 0, -1.0
        out = core.track({2: frames[1]})
        return out[2], core.state.clone()

    box, after = step()
    assert core.step_counts == {2: 1}
    pk = core._packs[2]
    assert pk["list"].tolist() == [2, -1]
    nan = float("nan")
    pk["search"][:, 1].fill_(nan)
    for name in ("template", "online_template"):
        for t in pk.get(name, ()):
            t[1].fill_(nan)
    poisoned = 0
    for k, v in pk["ws"].items():
        for t in (v if isinstance(v, (list, tuple)) else [v]):
            if isinstance(t, torch.Tensor) and t.is_floating_point():
                if k in ("in_t", "in_o", "in_s"):
                    continue  # the rung reads its own inputs, not the workspace's
                t.fill_(nan)  # row 0's cache rows are gathered again by the step, everything else is recomputed
                poisoned += 1
    assert poisoned > 20
    box2, after2 = step()
    assert box2 == box and not any(math.isnan(v) for v in box2)
    assert torch.equal(after.view(torch.int64), after2.view(torch.int64))
    for b in (0, 1, 3):
        assert torch.equal(after2[b].view(torch.int64), start[b].view(torch.int64)), b
    assert not torch.equal(after2[2], start[2])


def test_candidate_elimination_packs_without_the_slot_cache():
    """asymmetric_shared_ce (no slot cache: that stays refused): 2 of 4 slots active run at rung 2, bitwise a
    2-slot core on the same states, templates and frames; the pruning is per sample, the padded rows do not exist."""
    from lib.test.tracker import asymmetric_shared_ce
    from test_gpu_batch_tracker import _params
    sd = _synth_sd("asym_ce")

    def make(slots, pack=None):
        params = _params()
        if pack:
            params.pack_slots = pack
        trk = asymmetric_shared_ce.get_batch_tracker_class()(params, "synth", slots)
        trk.network.load_state_dict(sd, strict=True)
        trk.network.set_compute_dtype(torch.float32)
        return trk

    trk = make(4, (2,))
    core = trk.core
    seqs = [_seq(3, **kw) for kw in SPECS[:2]]
    for b, (frames, init) in zip((1, 3), seqs):
        trk.initialize(b, frames[0], {"init_bbox": [init, init]})
    twins = {}
    for f in (1, 2):
        images = {b: frames[f] for b, (frames, _) in zip((1, 3), seqs)}
        R, act, out, ref, twin = _twin_step(None, sd, core, images, twins, make)
        assert R == 2 and act == [1, 3]
        for j, b in enumerate(act):
            assert out[b] == ref[j] and not any(math.isnan(v) for v in out[b]), (f, b, out[b], ref[j])
    assert core.step_counts == {2: 2}
    params = _params()
    params.pack_slots, params.slot_cache = (2,), True
    with pytest.raises(NotImplementedError):  # the existing refusal stays
        asymmetric_shared_ce.get_batch_tracker_class()(params, "synth", 4)


def test_weight_reload_drops_the_rung_plans():
    """The network drops its runtime (as after load_state_dict): the next packed step builds the rung anew on
    the new runtime, refreshes the active slot's cache rows there, and gives the same bits as before."""
    trk, sd = _tracker("shared-slot-cache", pack=(2,))
    core = trk.core
    frames, init = _seq(3, **SPECS[0])
    trk.initialize(1, frames[0], {"init_bbox": [init, init]})
    start = core.state.clone()
    box = core.track({1: frames[1]})[1]
    pk, rt, replays = core._packs[2], core._rt, core.refresh_replays
    assert replays == 1
    trk.network.refresh_kernels()
    core.state.copy_(start)
    core.frame_id[1] = 0
    box2 = core.track({1: frames[1]})[1]
    assert core._rt is not rt and core._packs[2] is not pk and core._plan is None
    assert core.refresh_replays == replays + 1
    assert box2 == box
    assert core.step_counts == {2: 2}


def test_off_is_off():
    """pack=None: the launch names of a core built without the keyword, in order, the same boxes bit for bit,
    every step counted at batch 4; params without pack_slots leave the option off."""
    from mmt_amd.tracking import RGBTBatchTrackerCore
    trk_a, sd = _batch_tracker("shared", 4)  # _params() has no pack_slots
    trk_b, _ = _batch_tracker("shared", 4, sd=sd, pack_slots=None)
    net = trk_a.network
    core_c = RGBTBatchTrackerCore(net, 2.0, 128, 5.0, 320, [3], multimodal=False, slots=4)  # no keyword at all
    cores = [trk_a.core, trk_b.core, core_c]
    trk_b.core.net = net
    assert all(c.pack == () for c in cores)
    seqs = [_seq(3, **kw) for kw in SPECS[:2]]
    outs = []
    for c in cores:
        for b, (frames, init) in enumerate(seqs):
            c.assign(b + 1, frames[0], init)
        outs.append([c.track({b + 1: seqs[b][0][f] for b in range(2)}) for f in (1, 2)])
        assert c.step_counts == {4: 2} and c._packs == {}
    names = [[e[2] for e in c._plan] for c in cores]
    assert names[0] == names[1] == names[2]
    assert names[0][0] == "track_sample_target_table" and names[0][-1] == "track_update_slots"
    assert not any("pack" in n for n in names[0])
    assert outs[0] == outs[1] == outs[2]


def _oracle_check(sd, frames, boxes):
    """The `shared` plain tracker's host loop (update interval 3), teacher-forced from `boxes`."""
    from oracle.forward import forward as oracle_forward

    def prep(pair, box, factor, sz):
        t = [pp.preprocess(pair[m], box, factor, sz, lut=None) for m in range(2)]
        return [torch.from_numpy(x[0])[None] for x in t], t[0][2]

    H, W = frames[0][0].shape[:2]
    state = list(boxes[0])
    tmpl, _ = prep(frames[0], state, 2.0, 128)
    online = list(tmpl)
    assert len(boxes) == len(frames)
    for f in range(1, len(frames)):
        srch, rf = prep(frames[f], state, 5.0, 320)
        out, _ = oracle_forward(sd, "shared", tmpl, online, srch, run_score_head=False)
        ref = pp.track_update(out["pred_boxes"].view(4).numpy(), state, rf, H, W, 320)
        tol = 1e-3 * 320 / rf
        err = max(abs(a - c) for a, c in zip(boxes[f], ref))
        print("frame %d err %.3g px (tol %.3g)" % (f, err, tol))
        assert err <= tol, (f, boxes[f], ref)
        state = list(boxes[f])
        if f % 3 == 0:
            online, _ = prep(frames[f], state, 2.0, 128)


def test_track_sequences_on_the_packing_core():
    """The four sequences plus two pending ones of 2 frames each.  Slots 3 and 2 take the pending ones after
    steps 1 and 2, so the active counts are 4, 4, 3, 2, 1: batches 4, 4, 4, 2, 1."""
    from mmt_amd.tracking import choose_rung, track_sequences
    trk, sd = _tracker("shared")
    core = trk.core
    lengths = LENGTHS + [2, 2]
    specs = SPECS + [dict(SPECS[1], seed=7), dict(SPECS[0], seed=8)]
    seqs = {"s%d" % i: _seq(n, **kw) for i, (n, kw) in enumerate(zip(lengths, specs))}
    res = track_sequences(core, [(name, frames, init) for name, (frames, init) in seqs.items()])
    # the schedule from the lengths alone: a slot whose sequence ends takes the next pending one
    left, pending, counts = [n - 1 for n in lengths[:4]], [n - 1 for n in lengths[4:]], {}
    while any(left):
        n = sum(1 for v in left if v)
        B = choose_rung((1, 2), n) or 4
        counts[B] = counts.get(B, 0) + 1
        left = [v - 1 if v else 0 for v in left]
        left = [v if v else (pending.pop(0) if pending else 0) for v in left]
    assert counts == {4: 3, 2: 1, 1: 1}
    assert core.step_counts == counts
    assert core.active_slots() == []
    for name, (frames, init) in seqs.items():
        assert res[name].error is None and len(res[name]) == len(frames), name
        _oracle_check(sd, frames, list(res[name]))
