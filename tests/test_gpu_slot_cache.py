"""Per-slot template K/V cache at the runtime level (runtime.slot_cache_workspace /
refresh_template_slots): N = 3 slots, staging capacity D = 2, synthetic weights as tests/test_gpu_cache.py.

The cache is filled for templates A on all three slots by the batch-3 set_template, then slots [2, 0] are
refreshed with templates B, then slot [1] alone (a list padded with -1).  Checked bit for bit: a slot not
listed keeps every cache row (all 3C columns) and its KV1 rows; a listed slot holds the K / V columns of the
staging pass's rows in list order and keeps its Q columns.  Checked within tests/test_gpu_cache.py's bars
(1e-3 fp32, 1e-2 bf16; boxes, and scores for asym_online): the search pass after the refresh against the
full forward on the mixed templates.

Negative control: before the refresh the same search pass must differ from that full forward on slots 0 and
2 by at least ten times the bar, i.e. the templates matter to the boxes.  The template seeds were picked on
the CPU with oracle.forward at batch 3.  Among plain N(0, 1) templates no pair of seeds 1..6 over search seeds
1..12 moved both slots' boxes by more than 0.053 in both variants, so templates B are drawn at 4 times the
amplitude: search seed 7, templates A = seed 5, templates B = 4 x seed 6, for which the oracle's own boxes for
A and B differ on slots (0, 2) by (0.141, 0.167) for shared and (0.161, 0.136) for asym_online -- past
10 x 1e-2, the larger of the two bars."""
import json

import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SEED_S, SEED_A, SEED_B, AMP_B = 7, 5, 6, 4.0
N, D = 3, 2
CASES = [(v, d) for v in ("shared", "asym_online") for d in ("f32", "bf16")]
TOL = {"f32": 1e-3, "bf16": 1e-2}


def _runtime(variant, dtype):
    from mmt_amd import synthetic
    from mmt_amd.runtime import MixFormerRGBTRuntime
    keys = json.load(open(GOLDEN + "/state_dict_%s.json" % variant))
    sd = {k: torch.from_numpy(v) for k, v in synthetic.synth_state_dict(keys).items()}
    return MixFormerRGBTRuntime(sd, variant, dtype=dtype)


def _inputs(seed, amp=1.0):
    from mmt_amd import synthetic
    t, o, s = synthetic.synth_inputs(N, seed=seed)
    return [(x * amp).cuda() for x in t], [(x * amp).cuda() for x in o], [x.cuda() for x in s]


def _snapshot(rt, ws, B):
    """Per layer the template rows of the cache as [mod][B][n_t][3C], and KV1 as [B][n_t][2C]."""
    d = rt.d
    rows = [q.view(d.nmod, B, d.ntok, 3 * d.C)[:, :, :d.n_t].clone() for q in ws["QKVL"]]
    kv1 = ws["KV1"].view(B, d.n_t, 2 * d.C).clone() if "KV1" in ws else None
    return rows, kv1


@pytest.fixture(scope="module", params=CASES, ids=["%s-%s" % c for c in CASES])
def run(request):
    """One pass of the whole scenario per (variant, dtype); the tests below read its record."""
    variant, dname = request.param
    rt = _runtime(variant, torch.float32 if dname == "f32" else torch.bfloat16)
    score = variant == "asym_online"
    tA, oA, _ = _inputs(SEED_A)
    tB, oB, _ = _inputs(SEED_B, AMP_B)
    _, _, s = _inputs(SEED_S)
    sc = rt.slot_cache_workspace(N, D)
    ws, st = sc["ws"], sc["stage"]
    r = dict(variant=variant, tol=TOL[dname], score=score, C=rt.d.C, sc=sc)
    r["zeroed"] = all(bool((q == 0).all()) for q in ws["QKVL"])
    rt.set_template(tA, oA)  # batch-3 template pass: templates A on every slot
    r["snap0"] = _snapshot(rt, ws, N)
    box, scr = rt.forward_search(s, run_score_head=score)
    r["before"] = (box.clone(), scr.clone() if score else None)
    for dst, src in zip(ws["in_t"] + ws["in_o"], tB + oB):  # templates B into slots 2 and 0 of the N-slot buffers
        dst[[2, 0]] = src[[2, 0]]
    r["replays_20"] = rt.refresh_template_slots(sc, [2, 0])
    r["snap1"] = _snapshot(rt, ws, N)
    r["stage1"] = _snapshot(rt, st, D)
    r["list1"] = sc["slots"].tolist()
    r["replays_1"] = rt.refresh_template_slots(sc, [1])
    r["snap2"] = _snapshot(rt, ws, N)
    r["list2"] = sc["slots"].tolist()
    box, scr = rt.forward_search(s, run_score_head=score)
    r["after"] = (box.clone(), scr.clone() if score else None)
    mixed = lambda A, B: [torch.stack([b[0], a[1], b[2]]) for a, b in zip(A, B)]  # noqa: E731
    box, scr = rt.forward(mixed(tA, tB), mixed(oA, oB), s, run_score_head=score)
    r["full"] = (box.clone(), scr.clone() if score else None)
    torch.cuda.synchronize()
    return r


def _same(a, b):
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_cache_rows_start_zeroed(run):
    assert run["zeroed"]


def test_unlisted_slot_is_bitwise_unchanged(run):
    (q0, k0), (q1, k1), (q2, k2) = run["snap0"], run["snap1"], run["snap2"]
    assert run["replays_20"] == 1 and run["replays_1"] == 1
    assert run["list1"] == [2, 0] and run["list2"] == [1, -1]  # the second list padded with -1
    for i in range(len(q0)):
        assert _same(q1[i][:, 1], q0[i][:, 1]), i            # refresh [2, 0]: slot 1, all 3C columns
        assert _same(q2[i][:, [0, 2]], q1[i][:, [0, 2]]), i  # refresh [1, -1]: slots 0 and 2
    if k0 is not None:
        assert _same(k1[1], k0[1]) and _same(k2[[0, 2]], k1[[0, 2]])


def test_listed_slots_hold_the_staging_rows_in_list_order(run):
    (q0, _), (q1, k1), (qs, ks) = run["snap0"], run["snap1"], run["stage1"]
    C = run["C"]
    changed = False
    for i in range(len(q1)):
        for j, slot in enumerate((2, 0)):
            assert _same(q1[i][:, slot, :, C:], qs[i][:, j, :, C:]), (i, slot)  # K and V columns
            assert _same(q1[i][:, slot, :, :C], q0[i][:, slot, :, :C]), (i, slot)  # Q columns are not copied
            changed = changed or not _same(q1[i][:, slot, :, C:], q0[i][:, slot, :, C:])
    assert changed  # templates B are not templates A
    if k1 is not None:
        assert _same(k1[2], ks[0]) and _same(k1[0], ks[1])


def test_search_pass_after_refresh_matches_full_forward(run):
    tol = run["tol"]
    err = (run["after"][0] - run["full"][0]).abs().amax(1)
    print("%s: box err per slot %s (tol %.0e)" % (run["variant"], err.tolist(), tol))
    assert err.max().item() <= tol
    if run["score"]:
        serr = (run["after"][1] - run["full"][1]).abs()
        print("score err per slot %s" % serr.tolist())
        assert serr.max().item() <= tol


def test_negative_control_stale_cache_differs(run):
    tol = run["tol"]
    diff = (run["before"][0] - run["full"][0]).abs().amax(1)
    print("%s: stale-cache box difference per slot %s (10 x tol = %.0e)" % (run["variant"], diff.tolist(), 10 * tol))
    assert diff[0].item() >= 10 * tol and diff[2].item() >= 10 * tol
    assert diff[1].item() <= tol  # slot 1 kept templates A


def test_refresh_rejects_slots_out_of_range(run):
    from mmt_amd.runtime import MixFormerRGBTRuntime
    with pytest.raises(IndexError):
        MixFormerRGBTRuntime.refresh_template_slots(None, run["sc"], [N])
