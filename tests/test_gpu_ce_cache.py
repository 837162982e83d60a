"""Candidate elimination in the template-cached passes (runtime.set_template / forward_search, the module's
set_online / forward_test, the tracker's params.kv_cache) on the synthetic weights and the reference-made
goldens of tests/test_gpu_ce.py.

* fp32: the cached pass's boxes within 1e-3 of the golden and of forward() on the same inputs, every
  stage's kept indices identical to the reference's and its attention means within 1e-5 relative.
* bf16: as test_gpu_ce.py::test_ce_model_matches_reference -- kept-set overlap with the reference >= 0.9
  per stage and modality, boxes within 1e-2 of the oracle replaying the cached pass's own selections.  The
  cached and the full bf16 selections are not required to be equal (the compact GEMMs may associate
  differently).
* One template pass, three search frames, with every cache search row and every activation stream filled
  with NaN before each frame: boxes finite and within 1e-3 of forward(), template rows of the cache
  untouched.
* Module and tracker API; the full-forward plan is the same before and after the cache plans are built."""
import importlib
import json

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
_RT = {}


def _state_dict():
    from mmt_amd import synthetic
    keys = json.load(open(GOLDEN + "/state_dict_asym_ce.json"))
    return {k: torch.from_numpy(v) for k, v in synthetic.synth_state_dict(keys).items()}


def _runtime(dtype, mask_count=None):
    key = (dtype, mask_count)
    if key not in _RT:
        from mmt_amd.runtime import MixFormerRGBTRuntime
        _RT[key] = MixFormerRGBTRuntime(_state_dict(), "asym_ce", dtype=dtype, ce_mask_count=mask_count)
    return _RT[key]


def _inputs(B, seed=None):
    from mmt_amd import synthetic
    t, o, s = synthetic.synth_inputs(B) if seed is None else synthetic.synth_inputs(B, seed=seed)
    return [x.cuda() for x in t], [x.cuda() for x in o], [x.cuda() for x in s]


def _gold(B, masked):
    return np.load(GOLDEN + "/model_asym_ce_%sb%d.npz" % ("mask_" if masked else "", B))


def _scrub_selection(ws, gold):
    """Forget what an earlier pass selected: the slots a stage writes (the rest of a CEG row stays -1) and
    the attention means."""
    for k in range(3):
        ws["CEG"][k][:, :gold["ce%d_keep_v" % k].shape[1]] = -2
        ws["CEM"][k].fill_(float("nan"))


def cached_selection(ws, gold, B):
    """(identical per stage+modality, overlap per stage+modality, the selections as ce_forced takes them)."""
    same, overlap, forced = [], [], []
    for k in range(3):
        pair = []
        for m, nm in enumerate(("v", "i")):
            ref = gold["ce%d_keep_%s" % (k, nm)]
            got = ws["CEG"][k].view(2, B, -1)[m, :, :ref.shape[1]].cpu().numpy()
            same.append(bool(np.array_equal(got, ref)))
            overlap.append(min(len(set(got[b]) & set(ref[b])) / ref.shape[1] for b in range(B)))
            pair.append(got)
        forced.append(tuple(pair))
    return same, overlap, forced


def oracle_replay_error(box, inputs, forced, mask):
    from oracle.forward import forward as oracle_forward, state_dict_to_torch
    from mmt_amd import synthetic
    sd = state_dict_to_torch(synthetic.synth_state_dict(json.load(open(GOLDEN + "/state_dict_asym_ce.json"))))
    out, _ = oracle_forward(sd, "asym_ce", *[[x.cpu() for x in grp] for grp in inputs], ce_forced=forced,
                            ce_template_mask=mask)
    B = box.shape[0]
    return np.abs(box.cpu().numpy() - out["pred_boxes"].reshape(B, 4).numpy()).max()


@pytest.mark.parametrize("B,masked", [(1, False), (2, False), (2, True)])
def test_cached_ce_fp32_matches_reference_and_full(B, masked):
    gold = _gold(B, masked)
    mask = torch.from_numpy(gold["ce_template_mask"]).cuda() if masked else None
    rt = _runtime(torch.float32, 4 if masked else None)
    t, o, s = _inputs(B)
    box_full = rt.forward(t, o, s, ce_template_mask=mask)[0].clone()
    ws = rt.cache_workspace(B)
    _scrub_selection(ws, gold)
    rt.set_template(t, o)
    box, _ = rt.forward_search(s, ce_template_mask=mask)
    torch.cuda.synchronize()
    err_g = np.abs(box.cpu().numpy() - gold["pred_boxes"].reshape(B, 4)).max()
    err_f = (box - box_full).abs().max().item()
    same, overlap, _ = cached_selection(ws, gold, B)
    print("asym_ce cached B=%d masked=%s f32: vs golden %.3g, vs full %.3g, stages identical %s" % (B, masked, err_g,
                                                                                                 err_f, same))
    assert err_g <= 1e-3 and err_f <= 1e-3, (err_g, err_f)
    assert all(same), same
    for k in range(3):
        ref = gold["ce%d_attn_mean" % k]
        n = ref.shape[1]
        am = ws["CEM"][k].view(-1)[:B * n].view(B, n).cpu().numpy()
        aerr = np.abs(am - ref).max() / np.abs(ref).max()
        assert aerr <= 1e-5, (k, aerr)
        assert bool((ws["CEG"][k][:, gold["ce%d_keep_v" % k].shape[1]:] == -1).all())  # the rest of a row stays -1
    with pytest.raises(ValueError):  # forward()'s mask contract
        rt.forward_search(s, ce_template_mask=None if masked else torch.ones(B, 256, dtype=torch.bool, device="cuda"))


@pytest.mark.parametrize("B", [1, 2])
def test_cached_ce_bf16_matches_reference(B):
    gold = _gold(B, False)
    rt = _runtime(torch.bfloat16)
    inputs = _inputs(B)
    ws = rt.cache_workspace(B)
    rt.set_template(inputs[0], inputs[1])
    box, _ = rt.forward_search(inputs[2])
    torch.cuda.synchronize()
    err_g = np.abs(box.cpu().numpy() - gold["pred_boxes"].reshape(B, 4)).max()
    same, overlap, forced = cached_selection(ws, gold, B)
    rerr = oracle_replay_error(box, inputs, forced, None)
    print("asym_ce cached B=%d bf16: box err vs golden %.3g, vs the oracle replaying its selections %.3g, kept-set "
          "overlap %s" % (B, err_g, rerr, ["%.3f" % x for x in overlap]))
    assert rerr <= 1e-2, rerr
    assert min(overlap) >= 0.9, overlap


def test_cache_reused_across_frames_with_stale_rows_poisoned():
    rt = _runtime(torch.float32)
    d = rt.d
    t, o, _ = _inputs(1)
    ws = rt.cache_workspace(1)
    rt.set_template(t, o)
    torch.cuda.synchronize()
    rows = lambda q: q.view(2, d.ntok, 3 * d.C)  # noqa: E731
    snap = [rows(q)[:, :d.n_t].clone() for q in ws["QKVL"]]
    for seed in (11, 12, 13):
        _, _, s = _inputs(1, seed=seed)
        for q in ws["QKVL"]:
            rows(q)[:, d.n_t:] = float("nan")
        for name in ("X", "XC", "XN", "AO", "HID", "XT"):
            ws[name].fill_(float("nan"))
        box = rt.forward_search(s)[0].clone()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(box).all()), box
        for q, ref in zip(ws["QKVL"], snap):
            assert torch.equal(rows(q)[:, :d.n_t], ref)
        full, _ = rt.forward(t, o, s)  # its own qkv buffer: the cache's template rows stay
        err = (box - full).abs().max().item()
        print("seed %d: cached vs full %.3g" % (seed, err))
        assert err <= 1e-3, err


def test_full_forward_plan_untouched_by_the_cache_plans():
    from mmt_amd.runtime import MixFormerRGBTRuntime
    rt = MixFormerRGBTRuntime(_state_dict(), "asym_ce", dtype=torch.bfloat16)
    t, o, s = _inputs(1)
    ws = rt.workspace(1)
    names = [p[2] for p in ws["plan"]]
    box0 = rt.forward(t, o, s)[0].clone()
    assert rt.cache_workspace(1) is ws
    assert [p[2] for p in ws["plan"]] == names
    assert not any(p[2].startswith("ce_") for p in ws["plan_t"])
    cached = [p[2] for p in ws["plan_s"] if p[2].startswith("ce_")]
    assert cached == ["ce_t2s", "ce_select", "ce_rows_gather_cast"] * 3 + ["ce_index_invert", "ce_recover_rows"]
    rt.set_template(t, o)
    rt.forward_search(s)
    box1 = rt.forward(t, o, s)[0]
    torch.cuda.synchronize()
    assert torch.equal(box0, box1)


def test_module_set_online_forward_test():
    from mmt_amd import model as M
    from mmt_amd import synthetic
    net = M.build_asymmetric_shared_ce(M.hot_path_cfg(), train=False)
    keys = [(k, list(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.synth_state_dict(keys).items()}, strict=True)
    net = net.cuda().eval().set_compute_dtype(torch.float32)
    assert M.MixFormer_RGBT_CE.set_online is M._HipTracker.set_online
    assert M.MixFormer_RGBT_CE.forward_test is M._HipTracker.forward_test
    t, o, s = _inputs(2)
    with torch.no_grad():
        full, _ = net(t, o, s)
        net.set_online(t, o)
        out, _ = net.forward_test(s)
    err = (out["pred_boxes"] - full["pred_boxes"]).abs().max().item()
    gold = _gold(2, False)
    assert err <= 1e-3, err
    assert np.abs(out["pred_boxes"].cpu().numpy().reshape(2, 4) - gold["pred_boxes"].reshape(2, 4)).max() <= 1e-3


def _ce_tracker(kv_cache, use_graph):
    from test_gpu_tracker import _params
    mod = importlib.import_module("lib.test.tracker.asymmetric_shared_ce")
    params = _params("asym_ce")
    params.cfg.TEST.UPDATE_INTERVALS = {"SYNTH": [3]}
    if kv_cache is not None:
        params.kv_cache = kv_cache
    trk = mod.get_tracker_class()(params, "synth")
    sd = _state_dict()
    trk.network.load_state_dict(sd, strict=True)
    trk.network.set_compute_dtype(torch.float32)
    trk.core.use_graph = use_graph
    trk.core._plan = trk.core._graph = None
    return trk, sd


def test_tracker_kv_cache_matches_oracle():
    """test_gpu_tracker.py::test_tracking_loop_matches_oracle's loop (teacher-forced oracle steps, tolerance
    1e-3 * 320 / rf px) for the CE tracker with params.kv_cache = True, replaying captured graphs; the eager
    tracker then runs the same launches on the same frames and must give the same boxes."""
    from oracle import preprocess as pp
    from oracle.forward import forward as oracle_forward
    from test_gpu_tracker import _seq
    assert _ce_tracker(None, True)[0].core.kv_cache is False  # the default stays off
    trk, sd = _ce_tracker(True, True)
    assert trk.core.kv_cache is True
    frames, init = _seq(5)
    lut = pp.jet_lut()
    trk.initialize(frames[0], {"init_bbox": [init, init]})
    H, W = frames[0][0].shape[:2]

    def prep(im_pair, box, factor, sz):
        t = [pp.preprocess(im_pair[m], box, factor, sz, lut=lut if m == 1 else None) for m in range(2)]
        return [torch.from_numpy(x[0])[None] for x in t], t[0][2]

    tmpl, _ = prep(frames[0], init, 2.0, 128)
    online = list(tmpl)
    state, boxes = list(init), []
    for f in range(1, len(frames)):
        srch, rf = prep(frames[f], state, 5.0, 320)
        out, _ = oracle_forward(sd, "asym_ce", tmpl, online, srch)
        ref = pp.track_update(out["pred_boxes"].view(4).numpy(), state, rf, H, W, 320)
        got = trk.track(frames[f], {})["target_bbox"]
        tol = 1e-3 * 320 / rf
        err = max(abs(a - b) for a, b in zip(got, ref))
        print("frame %d err %.3g px (tol %.3g)" % (f, err, tol))
        assert err <= tol, (f, got, ref)
        state = got
        boxes.append(got)
        if f % 3 == 0:
            online, _ = prep(frames[f], state, 2.0, 128)
            for m in range(2):
                assert torch.equal(trk.core.online_template[m].cpu(), online[m])
    assert trk.core._graph is not None and trk.core._tmpl_graph is not None
    eager, _ = _ce_tracker(True, False)
    eager.initialize(frames[0], {"init_bbox": [init, init]})
    for f in range(1, len(frames)):
        got = eager.track(frames[f], {})["target_bbox"]
        assert max(abs(a - b) for a, b in zip(got, boxes[f - 1])) <= 1e-6, (f, got, boxes[f - 1])
    assert eager.core._graph is None
