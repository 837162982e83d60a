"""Candidate elimination in fp16 (MMT_F16): the full forward and the template-cached pass.

The scheme is the 16-bit branch of tests/test_gpu_ce.py::test_ce_model_matches_reference: the selection is
a discrete function of attention means whose cut gaps are below the 16-bit types' resolution, so the kept
sets may differ slightly from the reference's (overlap >= 0.9 per stage and modality required); the fp16
arithmetic is checked on its own choices -- the oracle replays them (ce_forced) and the boxes must agree
within 1e-2.  The box error against the golden and the overlaps are printed next to bf16's from the same run
(whether fp16's wider significand keeps more of the reference's tokens than bf16 is measured, not assumed).
The CE tracker under set_compute_dtype(torch.float16) tracks five frames to finite boxes inside the frame."""
import numpy as np
import pytest
import torch

from test_gpu_ce_cache import _ce_tracker, _gold, _inputs, _runtime, cached_selection, oracle_replay_error

pytestmark = pytest.mark.gpu


def _run(rt, inputs, mask, cached):
    if cached:
        rt.set_template(inputs[0], inputs[1])
        box, _ = rt.forward_search(inputs[2], ce_template_mask=mask)
    else:
        box, _ = rt.forward(*inputs, ce_template_mask=mask)
    torch.cuda.synchronize()
    return box


@pytest.mark.parametrize("cached", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B", [1, 2])
def test_ce_fp16_matches_reference(B, masked, cached):
    gold = _gold(B, masked)
    mask = torch.from_numpy(gold["ce_template_mask"]) if masked else None
    inputs = _inputs(B)
    dmask = None if mask is None else mask.cuda()
    res = {}
    for name, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):  # bf16: the same run, for the printed comparison
        rt = _runtime(dt, 4 if masked else None)
        ws = rt.cache_workspace(B) if cached else rt.workspace(B)
        box = _run(rt, inputs, dmask, cached)
        err = np.abs(box.cpu().numpy() - gold["pred_boxes"].reshape(B, 4)).max()
        _, overlap, forced = cached_selection(ws, gold, B)
        res[name] = (box.clone(), err, overlap, forced)
        print("asym_ce %s B=%d masked=%s %s: box err vs golden %.3g, kept-set overlap %s"
              % ("cached" if cached else "full", B, masked, name, err, ["%.3f" % x for x in overlap]))
    box, err, overlap, forced = res["f16"]
    rerr = oracle_replay_error(box, inputs, forced, mask)
    print("f16 box err vs the oracle replaying the f16 selections %.3g" % rerr)
    assert rerr <= 1e-2, rerr
    assert min(overlap) >= 0.9, overlap


def test_ce_tracker_fp16_tracks():
    from test_gpu_tracker import _seq
    trk, _ = _ce_tracker(None, True)
    trk.network.set_compute_dtype(torch.float16)
    trk.core._plan = trk.core._graph = None
    frames, init = _seq(6)
    trk.initialize(frames[0], {"init_bbox": [init, init]})
    H, W = frames[0][0].shape[:2]
    for f in range(1, 6):
        x, y, w, h = trk.track(frames[f], {})["target_bbox"]
        assert all(np.isfinite(v) for v in (x, y, w, h)), (f, x, y, w, h)
        assert w > 0 and h > 0 and x >= 0 and y >= 0 and x + w <= W and y + h <= H, (f, x, y, w, h)
    assert trk.network._rt.dtype == torch.float16 and trk.network._rt.ce
