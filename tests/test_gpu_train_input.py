"""TrainInputProcessor on the GPU, end to end, on the fixture's samples at the real 128 / 320 sizes: every field
equals the host contract (which tests/test_train_input_host.py pins against the reference's own output), an
invalid sample's rows keep their fill, the outputs are persistent buffers, and a training forward / backward runs
on them in place."""
import random

import numpy as np
import pytest
import torch

from train_input_probes import contract, fixture, fixture_config, fixture_rolls, fixture_sample, samples_of

pytestmark = pytest.mark.gpu

KEYS = [("template", 0), ("template", 1), ("search", 0)]


def _real():
    ids = samples_of("real")
    valid = [i for i in ids if bool(fixture()["s%d_valid" % i])]
    invalid = [i for i in ids if i not in valid]
    assert len(valid) >= 2 and len(invalid) >= 1
    return valid, invalid


def test_process_batch_equals_the_contract_and_skips_the_invalid_sample():
    from mmt_amd.train_input import TrainInputProcessor
    valid, invalid = _real()
    order = [valid[0], invalid[0], valid[1]]  # the invalid sample in the middle
    cfg = fixture_config(order[0])
    assert (cfg.template_size, cfg.search_size) == (128, 320)
    proc = TrainInputProcessor(cfg, 3, "cuda", frame_hw=(8, 8))  # too small on purpose: the staging grows
    ptrs = {k: v.data_ptr() for k, v in proc.out.items()}
    out = proc.process_batch([fixture_sample(i) for i in order], [fixture_rolls(i) for i in order])
    torch.cuda.synchronize()
    assert {k: v.data_ptr() for k, v in out.items()} == ptrs
    assert out["valid"].cpu().tolist() == [True, False, True]
    for g, n, s in (("template", 2, 128), ("search", 1, 320)):
        for m in "vi":
            assert tuple(out["%s_images_%s" % (g, m)].shape) == (n, 3, 3, s, s)
            assert tuple(out["%s_anno_%s" % (g, m)].shape) == (n, 3, 4)
            assert tuple(out["%s_att_%s" % (g, m)].shape) == (n, 3, s, s) and out["%s_att_%s" % (g, m)].dtype == torch.bool
    host = {k: v.cpu() for k, v in out.items()}
    for b, i in enumerate(order):
        ref = contract(i)
        for g, f in KEYS:
            for m in "vi":
                img, box, att = (host["%s_%s_%s" % (g, k, m)][f, b] for k in ("images", "anno", "att"))
                if not ref["valid"]:
                    assert bool(torch.isnan(img).all()) and bool(torch.isnan(box).all()) and bool(att.all()), (i, g, f, m)
                    continue
                want = ref["%s_images_%s" % (g, m)][f]
                assert np.array_equal(img.numpy().view(np.uint32), want.numpy().view(np.uint32)), (i, g, f, m)
                assert torch.equal(box, ref["%s_anno_%s" % (g, m)][f]), (i, g, f, m)
                assert torch.equal(att, ref["%s_att_%s" % (g, m)][f]), (i, g, f, m)
    # a second batch into the same buffers: the rows of a sample that turned invalid keep the previous contents
    before = {k: v.clone() for k, v in host.items()}
    order2 = [invalid[0], valid[1], valid[0]]
    out2 = proc.process_batch([fixture_sample(i) for i in order2], [fixture_rolls(i) for i in order2])
    torch.cuda.synchronize()
    assert out2["valid"].cpu().tolist() == [False, True, True]
    img = out2["search_images_v"].cpu()
    assert np.array_equal(img[0, 0].numpy().view(np.uint32), before["search_images_v"][0, 0].numpy().view(np.uint32))
    assert torch.equal(img[0, 1], contract(valid[1])["search_images_v"][0])
    assert torch.equal(img[0, 2], contract(valid[0])["search_images_v"][0])
    assert torch.equal(out2["template_anno_i"].cpu()[1, 2], contract(valid[0])["template_anno_i"][1])


def test_drawn_rolls_and_batch_mismatch():
    from mmt_amd.train_input import TrainInputProcessor
    valid, _ = _real()
    proc = TrainInputProcessor((32, 64), 2, "cuda")
    with pytest.raises(ValueError, match="batch mismatch"):
        proc.process_batch([fixture_sample(valid[0])])
    random.seed(3), np.random.seed(3), torch.manual_seed(3)
    out = proc.process_batch([fixture_sample(valid[0]), fixture_sample(valid[1])])  # rolls drawn inside
    torch.cuda.synchronize()
    ok = out["valid"]
    assert bool(ok.any())
    for k, v in out.items():
        if k != "valid" and "_att_" not in k:
            assert bool(torch.isfinite(v[:, ok]).all()), k


def test_training_forward_backward_on_the_output_buffers():
    import mmt_amd.model as M
    import mmt_amd.train as T
    from mmt_amd.train_input import TrainInputProcessor
    valid, _ = _real()
    proc = TrainInputProcessor(fixture_config(valid[0]), 2, "cuda")
    out = proc.process_batch([fixture_sample(i) for i in valid[:2]], [fixture_rolls(i) for i in valid[:2]])
    assert out["valid"].cpu().tolist() == [True, True]
    torch.manual_seed(0)
    net = M.build_asymmetric_shared(M.hot_path_cfg(), train=False)
    net.drop_path_rate = 0.0
    net = net.cuda().train()
    tv, ti, sv, si = (out[k] for k in ("template_images_v", "template_images_i", "search_images_v", "search_images_i"))
    pred, _ = T.module_forward(net, [tv[0], ti[0]], [tv[1], ti[1]], [sv[0], si[0]], T.HipOps)  # views of the buffers
    loss, _ = T.box_loss(pred["pred_boxes"], out["search_anno_v"][0])
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)), loss
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert len(grads) > 100 and all(bool(torch.isfinite(g).all()) for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)
