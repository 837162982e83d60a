"""RGB-D input through the trackers (aux_format="depth16"): a core fed raw uint16 depth frames against the same
core fed the host preparation of those frames (mmt_amd.depth.depth_to_3xd) as ordinary uint8 frames, which is the
path every tracker had before.  The device preparation is bit-exact and everything behind it is unchanged, so the
boxes compare ==.  The depth cores keep their step graph across frame sizes, and an inactive slot's frame buffer
is not touched by a step."""
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_gpu_batch_tracker import _frame, _seq

pytestmark = pytest.mark.gpu

INTERVAL = 2


def _depth_seq(n, H=360, W=480, x0=200, y0=150, side=48, seed=0):
    """_seq's RGB frames with a raw depth frame as the second modality: a smooth background at 1.5-7 m, the object
    nearer, 10 % holes at 0, a few far readings above the 10 000 limit.  Returns (raw pairs, prepared pairs, box)."""
    from mmt_amd.depth import depth_to_3xd
    frames, init = _seq(n, H=H, W=W, x0=x0, y0=y0, side=side, seed=seed)
    rng = np.random.default_rng(101 + seed)
    bg = _frame(H, W, 33 + seed)[:, :, 0].astype(np.uint16) * 21 + 1500
    obj = rng.integers(700, 900, (side, side)).astype(np.uint16)
    raw, prepared = [], []
    for f, (fv, _) in enumerate(frames):
        d = bg.copy()
        x, y = x0 + 4 * f, y0 + 3 * f
        d[y:y + side, x:x + side] = obj
        d[rng.random((H, W)) < 0.1] = 0
        d[rng.random((H, W)) < 0.01] = 40000
        raw.append([fv, d])
        prepared.append([fv, depth_to_3xd(d)])
    return raw, prepared, init


@pytest.fixture(scope="module")
def sds():
    from conftest import GOLDEN
    from mmt_amd import synthetic
    out = {}
    for variant in ("asym", "shared", "asym_online"):
        keys = json.load(open(GOLDEN + "/state_dict_%s.json" % variant))
        out[variant] = {k: torch.from_numpy(v) for k, v in synthetic.synth_state_dict(keys).items()}
    key = "score_branch.score_head.layers.2.bias"  # lifts the scores over the gate's 0.5 on some frames
    out["asym_online"][key] = out["asym_online"][key] + 0.25
    return out


def _params(**over):
    from mmt_amd.model import hot_path_cfg
    cfg = hot_path_cfg()
    cfg.TEST.UPDATE_INTERVALS = {"SYNTH": [INTERVAL]}
    p = SimpleNamespace(cfg=cfg, template_factor=2.0, template_size=128, search_factor=5.0, search_size=320,
                        checkpoint=None, save_all_boxes=False)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _module(variant):
    """asym / asym_online: the shipped modules (JET look-up on the second modality's crops); shared: the shared
    backbone without the look-up, as tests/test_gpu_batch_tracker.py builds it."""
    from lib.models.mixformer_vit_rgbt import build_mixformer_vit_rgbt_shared
    from lib.test.tracker import asymmetric_shared, asymmetric_shared_online
    from lib.test.tracker._rgbt import make_batch_tracker_class, make_tracker_class
    plain = SimpleNamespace(
        get_tracker_class=lambda: make_tracker_class(build_mixformer_vit_rgbt_shared, multimodal=False),
        get_batch_tracker_class=lambda: make_batch_tracker_class(build_mixformer_vit_rgbt_shared, multimodal=False))
    return {"asym": asymmetric_shared, "shared": plain, "asym_online": asymmetric_shared_online}[variant]


def _pair(variant, sd, slots=None, **over):
    """The variant's tracker twice on the same weights: fed raw depth, and fed prepared uint8 frames."""
    out = []
    for aux in ("depth16", "rgb8"):
        mod = _module(variant)
        p = _params(aux_format=aux, **over)
        trk = mod.get_tracker_class()(p, "synth") if slots is None else mod.get_batch_tracker_class()(p, "synth", slots)
        trk.network.load_state_dict(sd, strict=True)
        assert trk.core.aux_format == aux
        out.append(trk)
    return out


@pytest.mark.parametrize("variant", ["asym", "shared"])
def test_single_core_depth16_equals_prepared_frames(sds, variant):
    """Two sequences of different frame sizes, the second larger (the device buffers grow): four frames each,
    update interval 2.  The depth core's step graph is one object throughout."""
    dt, rt = _pair(variant, sds[variant])
    assert (dt.core.lut is not None) == (variant == "asym")  # asym: the JET look-up reads the prepared frame
    graph = None
    for k, (H, W) in enumerate([(240, 320), (360, 480)]):
        raw, prepared, init = _depth_seq(4, H=H, W=W, x0=90 + 60 * k, y0=60 + 40 * k, seed=k)
        dt.initialize(raw[0], {"init_bbox": [init, init]})
        rt.initialize(prepared[0], {"init_bbox": [init, init]})
        assert torch.equal(dt.core.frames[1].cpu(), torch.from_numpy(prepared[0][1]))
        for f in range(1, 4):
            inputs = raw[f] if f != 2 else [torch.from_numpy(raw[f][0]).cuda(), torch.from_numpy(raw[f][1].view(np.int16)).cuda()]
            a, b = dt.track(inputs)["target_bbox"], rt.track(prepared[f])["target_bbox"]
            assert a == b, (k, f, a, b)
            assert torch.equal(dt.core.frames[1].cpu(), torch.from_numpy(prepared[f][1])), (k, f)
            graph = graph or dt.core._graph
            assert graph is not None and dt.core._graph is graph, (k, f)
    assert tuple(dt.core.frames[1].shape) == (360, 480, 3)


def test_single_core_depth16_refusals(sds):
    dt, _ = _pair("shared", sds["shared"])
    raw, _, init = _depth_seq(1, H=97, W=131, x0=20, y0=20, side=24)
    with pytest.raises(ValueError, match=r"\(97, 131\)"):
        dt.initialize([raw[0][0], raw[0][1][:, :-1]], {"init_bbox": [init, init]})
    with pytest.raises(ValueError, match="must be uint16"):
        dt.initialize([raw[0][0], raw[0][0]], {"init_bbox": [init, init]})


SIZES = [(360, 480), (240, 320), (97, 131)]
STARTS = [(200, 150, 48), (90, 60, 48), (30, 25, 24)]


def _seqs(n):
    return [_depth_seq(n, H=H, W=W, x0=x0, y0=y0, side=side, seed=3 + i)
            for i, ((H, W), (x0, y0, side)) in enumerate(zip(SIZES, STARTS))]


@pytest.mark.parametrize("over", [{}, {"slot_cache": True}, {"pack_slots": (2, 1)}], ids=["plain", "slot_cache", "pack"])
def test_batched_core_depth16_equals_prepared_frames(sds, over):
    """3 slots with three frame sizes; slot 1 is released after two steps, runs two steps empty (with pack: the
    two-slot rung) and takes slot 2's sequence shape with another start; boxes == the core fed prepared frames."""
    N = 3
    dt, rt = _pair("asym", sds["asym"], slots=N, **over)
    seqs = _seqs(7)
    extra = _depth_seq(3, H=240, W=400, x0=120, y0=80, seed=9)  # slot 1's second sequence: another size again
    for b in range(N):
        for trk, k in ((dt, 0), (rt, 1)):
            trk.initialize(b, seqs[b][k][0], {"init_bbox": [seqs[b][2]] * 2})
    graph = None
    live = {0: (seqs[0], 0), 1: (seqs[1], 0), 2: (seqs[2], 0)}  # slot -> (sequence, frames fed)
    for step in range(6):
        if step == 2:
            dt.release(1), rt.release(1)
            del live[1]
            idle = [dt.core.frames[1][m].clone() for m in range(2)], dt.core._dbuf[1].clone()
        if step == 4:
            for trk, k in ((dt, 0), (rt, 1)):
                trk.initialize(1, extra[k][0], {"init_bbox": [extra[2]] * 2})
            live[1] = (extra, 0)
        live = {b: (s, f + 1) for b, (s, f) in live.items()}
        a = dt.track({b: s[0][f] for b, (s, f) in live.items()})
        r = rt.track({b: s[1][f] for b, (s, f) in live.items()})
        assert sorted(a) == sorted(live)
        for b, (s, f) in live.items():
            assert a[b]["target_bbox"] == r[b]["target_bbox"], (step, b)
            assert torch.equal(dt.core._fview[b][1].cpu(), torch.from_numpy(s[1][f][1])), (step, b)
        if 2 <= step < 4:  # the released slot: nothing of it is written by a step
            assert all(torch.equal(x, y) for x, y in zip(idle[0], dt.core.frames[1]))
            assert torch.equal(idle[1], dt.core._dbuf[1])
        if "pack_slots" not in over:
            graph = graph or dt.core._graph
            assert graph is not None and dt.core._graph is graph, step
    if "pack_slots" in over:
        assert dt.core.step_counts == rt.core.step_counts == {3: 4, 2: 2}
    if "slot_cache" in over:
        assert dt.core.refresh_replays == rt.core.refresh_replays > 0


@pytest.mark.parametrize("batched", [False, True], ids=["single", "batched"])
def test_online_memory_depth16_equals_prepared_frames(sds, batched):
    """asym_online with a memory of two online templates, interval 2, four tracked frames: the promotion on frame
    2 fills the second slot from a candidate cropped out of the prepared depth frame."""
    dt, rt = _pair("asym_online", sds["asym_online"], slots=2 if batched else None, online_size=2)
    seqs = _seqs(5)[:2]
    if batched:
        for b in range(2):
            for trk, k in ((dt, 0), (rt, 1)):
                trk.initialize(b, seqs[b][k][0], {"init_bbox": [seqs[b][2]] * 2})
    else:
        dt.initialize(seqs[0][0][0], {"init_bbox": [seqs[0][2]] * 2})
        rt.initialize(seqs[0][1][0], {"init_bbox": [seqs[0][2]] * 2})
    for f in range(1, 5):
        if batched:
            a = dt.track({b: seqs[b][0][f] for b in range(2)})
            r = rt.track({b: seqs[b][1][f] for b in range(2)})
            assert all(a[b]["target_bbox"] == r[b]["target_bbox"] for b in range(2)), f
            assert dt.core.last_scores == rt.core.last_scores
        else:
            assert dt.track(seqs[0][0][f])["target_bbox"] == rt.track(seqs[0][1][f])["target_bbox"], f
        for m in range(2):
            assert torch.equal(dt.core.online_template[m], rt.core.online_template[m]), (f, m)
    counts = dt.core.online_count
    assert counts == rt.core.online_count and counts == ([2, 2] if batched else 2)  # the promotion happened
