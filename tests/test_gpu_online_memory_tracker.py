"""The online-score trackers with a memory of K = 3 online templates (params.online_size; upstream
lib/test/tracker/mixformer_vit_online.py:107-129), interval 2, 8 synthetic frames.

Every step of RGBTTrackerCore and RGBTBatchTrackerCore is compared with the same schedule driven by hand: a
second runtime gets the templates, the memory and the counts the core held before the step through set_template,
and the core's own search crops through forward_search (the batched core without slot_cache runs the full forward:
forward), at the same batch size; boxes and scores compare ==.  The
memory itself is compared with a list-based transliteration of upstream's rule in this file, fed with the core's
scores and crops made by the core's own crop kernel.  A promotion writes one slot and the length: the plan and
the graphs stay the same objects."""
import json
import math
from types import SimpleNamespace

import pytest
import torch

from test_gpu_batch_tracker import _seq

pytestmark = pytest.mark.gpu

K, INTERVAL, FRAMES = 3, 2, 9  # the first frame initialises: 8 tracked frames


@pytest.fixture(scope="module")
def sd():
    from conftest import GOLDEN
    from mmt_amd import synthetic
    keys = json.load(open(GOLDEN + "/state_dict_asym_online.json"))
    sd = {k: torch.from_numpy(v) for k, v in synthetic.synth_state_dict(keys).items()}
    key = "score_branch.score_head.layers.2.bias"  # lifts the scores over the gate's 0.5 on some frames
    sd[key] = sd[key] + 0.25
    return sd


@pytest.fixture(scope="module")
def hand_rt(sd):
    from mmt_amd.runtime import MixFormerRGBTRuntime
    return MixFormerRGBTRuntime(sd, "asym_online", online_size=K)


def _params(**over):
    from mmt_amd.model import hot_path_cfg
    cfg = hot_path_cfg()
    cfg.TEST.UPDATE_INTERVALS = {"SYNTH": [INTERVAL]}
    p = SimpleNamespace(cfg=cfg, template_factor=2.0, template_size=128, search_factor=5.0, search_size=320,
                        checkpoint=None, save_all_boxes=False, online_size=K)
    for k, v in over.items():
        setattr(p, k, v)
    return p


class _Memory:
    """Upstream's rule on lists (mixformer_vit_online.py:68, :107-129), one sequence."""

    def __init__(self, template):
        self.template = template
        self.online = [template]
        self.cand, self.best, self.forget = template, -1.0, 0
        self.crops = self.writes = 0

    def frame(self, frame_id, score, crop):
        if score > 0.5 and score > self.best:
            self.cand, self.best = crop(), score
            self.crops += 1
        if frame_id % INTERVAL == 0:
            if len(self.online) < K:
                self.online.append(self.cand)
            else:
                self.online[self.forget] = self.cand
                self.forget = (self.forget + 1) % K
            self.best, self.cand = -1, self.template
            self.writes += 1


def _crop(core, frames, state):
    """A template crop by the core's own kernel, into fresh buffers: [rgb, tir] (3, ts, ts)."""
    from mmt_amd import tracking
    out = [torch.empty(1, 3, core.ts, core.ts, device="cuda") for _ in range(2)]
    tmp = torch.empty(2, 4, dtype=torch.float64, device="cuda")
    tracking.sample_target([tracking.crop_params(frames[m], state, core.tf, core.ts, out=out[m].view(-1), crop=tmp[m],
                                                 lut=core.lut if m == 1 else None) for m in range(2)])
    torch.cuda.synchronize()
    return [x[0].clone() for x in out]


def _check_memory(core_online, count, mem, b=0):
    assert count == len(mem.online)
    for k, img in enumerate(mem.online):
        for m in range(2):
            assert torch.equal(core_online[m][b, k], img[m]), (b, k, m)


def test_single_core_matches_the_hand_driven_schedule(sd, hand_rt):
    from lib.test.tracker import asymmetric_shared_online
    trk = asymmetric_shared_online.get_tracker_class()(_params(), "synth")
    trk.network.load_state_dict(sd, strict=True)
    core = trk.core
    assert core.online_size == K and core.kv_cache and trk.network.online_size == K
    frames, init = _seq(FRAMES)
    trk.initialize(frames[0], {"init_bbox": [init, init]})
    mem = _Memory([core.template[m][0].clone() for m in range(2)])
    _check_memory(core.online_template, core.online_count, mem)
    objs = None
    for f in range(1, FRAMES):
        online = [x.clone() for x in core.online_template]
        count = core.online_count
        trk.track(frames[f])
        ws = core._ws
        box, score = ws["BOX"].clone(), ws["SC"].view(-1).clone()
        hand_rt.set_template(core.template, online, online_count=[count])
        hbox, hsc = hand_rt.forward_search(core.search, run_score_head=True)
        torch.cuda.synchronize()
        assert bool((box == hbox).all()) and bool((score == hsc).all()), f
        mem.frame(f, torch.sigmoid(score).item(), lambda: _crop(core, core.frames, core.state))
        _check_memory(core.online_template, core.online_count, mem)
        assert ws["TL"].tolist() == [(1 + count) * core._rt.d.nt1] * 2
        now = (core._plan, core._graph, core._tmpl_plan, core._tmpl_graph, core._rt)
        assert all(x is not None for x in now)
        objs = objs or now
        assert all(a is b for a, b in zip(objs, now)), f  # promotions re-plan and re-capture nothing
    assert mem.writes == (FRAMES - 1) // INTERVAL and core.online_count == K and mem.crops > 0
    assert core.forget_id == mem.forget == 2  # two appends filled the memory, two writes went round the ring


@pytest.mark.parametrize("slot_cache", [False, True])
def test_batched_core_matches_the_hand_driven_schedule(sd, hand_rt, slot_cache):
    """Three slots assigned on steps 0, 2 and 4: on step 5 they hold 3, 2 and 1 online templates in one replay."""
    from lib.test.tracker import asymmetric_shared_online
    N = 3
    trk = asymmetric_shared_online.get_batch_tracker_class()(_params(slot_cache=slot_cache, refresh_slots=N), "synth", N)
    trk.network.load_state_dict(sd, strict=True)
    core = trk.core
    seqs = [_seq(FRAMES, seed=0), _seq(FRAMES, x0=180, y0=140, seed=5), _seq(FRAMES, H=240, W=320, x0=90, y0=60, seed=7)]
    start = {0: 0, 2: 1, 4: 2}  # step -> slot
    live, mems, fid, spread, graph = [], {}, {}, set(), None
    for step in range(FRAMES - 1):
        if step in start:
            b = start[step]
            frames, init = seqs[b]
            trk.initialize(b, frames[0], {"init_bbox": [init, init]})
            mems[b], fid[b] = _Memory([core.template[m][b].clone() for m in range(2)]), 0
            _check_memory(core.online_template, core.online_count[b], mems[b], b)
            live.append(b)
        online = [x.clone() for x in core.online_template]
        counts = list(core.online_count)
        for b in live:
            fid[b] += 1
        trk.track({b: seqs[b][0][fid[b]] for b in live})
        ws = core._ws
        box, score = ws["BOX"].clone(), ws["SC"].view(-1).clone()
        assert ws["TL"].tolist() == [(1 + c) * core._rt.d.nt1 for c in counts] * 2
        if slot_cache:  # the step is the search pass over the slots' cached template rows
            hand_rt.set_template(core.template, online, online_count=counts)
            hbox, hsc = hand_rt.forward_search(core.search, run_score_head=True)
        else:  # the step is the full forward
            hbox, hsc = hand_rt.forward(core.template, online, core.search, run_score_head=True, online_count=counts)
        torch.cuda.synchronize()
        for b in live:
            assert bool((box[b] == hbox[b]).all()) and bool(score[b] == hsc[b]), (step, b)
        spread.add(tuple(counts[b] for b in live))
        for b in live:
            mems[b].frame(fid[b], torch.sigmoid(score[b]).item(),
                          lambda b=b: _crop(core, core._fview[b], core.state[b]))
            _check_memory(core.online_template, core.online_count[b], mems[b], b)
        graph = graph or core._graph
        assert graph is not None and core._graph is graph, step
    assert (3, 2, 1) in spread  # different fill levels in one step
    assert sum(m.crops for m in mems.values()) > 0


def test_slot_cache_refreshes_once_per_promotion(sd):
    """refresh_slots = 1: one refresh replay per assign and per promotion, none for a candidate crop."""
    from lib.test.tracker import asymmetric_shared_online
    trk = asymmetric_shared_online.get_batch_tracker_class()(_params(slot_cache=True, refresh_slots=1), "synth", 2)
    trk.network.load_state_dict(sd, strict=True)
    core = trk.core
    seqs = [_seq(6, seed=0), _seq(6, x0=180, y0=140, seed=5)]
    for b, (frames, init) in enumerate(seqs):
        trk.initialize(b, frames[0], {"init_bbox": [init, init]})
    promotions, rgraph = 0, None
    for f in range(1, 6):
        trk.track({b: seqs[b][0][f] for b in range(2)})
        # the refresh runs at the start of a step: it has seen the assigns and the promotions of earlier frames
        assert core.refresh_replays == 2 + promotions, f
        promotions += 2 * (f % INTERVAL == 0)
        rgraph = rgraph or core._sc["graph"]
        assert core._sc["graph"] is rgraph
    assert promotions == 4 and core.online_count == [K, K]


def test_default_is_todays_tracker(sd):
    """online_size 1 and decay 1.0: no ring state is consulted, the runtime has no length buffer."""
    from lib.test.tracker import asymmetric_shared_online
    trk = asymmetric_shared_online.get_tracker_class()(_params(online_size=1), "synth")
    trk.network.load_state_dict(sd, strict=True)
    core = trk.core
    assert not core._ring and not core.kv_cache and core.online_template[0].dim() == 4
    frames, init = _seq(4)
    trk.initialize(frames[0], {"init_bbox": [init, init]})
    for f in range(1, 4):
        out = trk.track(frames[f])
        assert all(math.isfinite(v) for v in out["target_bbox"])
    assert "TL" not in core._ws
