"""The training-glue probes themselves (tests/train_glue_probes.py), on the CPU: the constants are the sources', the
case tables reach every class they claim (computed from the shapes), the operands the bitwise families call exact are
exact, the restatements meet their own bars, every planted defect fails the comparison the GPU test uses, and the C
ABI rejects every host-checkable bad argument before any launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gemm_probes as P
import head_probes as H
import train_glue_probes as A
from conftest import ROOT

F64, F32, BF16 = A.F64, A.F32, A.BF16
CSRC = os.path.join(ROOT, "multi-modal-tracking_amd", "csrc")


def test_constants_match_the_library_sources():
    hdr = open(os.path.join(ROOT, "include", "mmt_hip.h")).read()
    assert "#define MMT_EBADARG (%d)" % A.EBADARG in hdr
    assert "#define MMT_ADAMW_MAX_GROUPS %d" % A.ADAMW_MAX_GROUPS in hdr and A.ADAMW_MAX_GROUPS == 8
    ft = open(os.path.join(CSRC, "fusion_train.hip")).read()
    for mul in (A.MIX_A, A.MIX_B, A.CTR_MUL, A.WORD_MUL):
        assert "0x%Xull" % mul in ft, hex(mul)
    assert ft.count("__launch_bounds__(%d)" % A.WG) == 8 and ft.count("blockIdx.x * %d + threadIdx.x" % A.WG) == 8
    assert "(chunks + %d) / %d" % (A.WG - 1, A.WG) in ft and A.WG == 256
    assert "d.thr = (uint32_t)(keep * 65536.0 + 0.5);" in ft and "d.scale = d.on ? (float)(1.0 / keep) : 1.f;" in ft
    assert "(2 * c + h) * 0x%Xull" % A.WORD_MUL in ft and "(r >> (16 * j)) & 0xffffu) < d.thr" in ft
    assert "ft_mix(seed ^ ft_mix(ctr * 0x%Xull + d.salt))" % A.CTR_MUL in ft
    opt = open(os.path.join(CSRC, "optim.hip")).read()
    assert "constexpr int CHUNK = 1 << 16;" in opt and A.CHUNK == 1 << 16
    loss = open(os.path.join(CSRC, "loss.hip")).read()
    assert "constexpr int BL_T = %d;" % A.BL_T in loss and A.BL_T == 256
    assert "for (int b = threadIdx.x; b < B; b += BL_T)" in loss and "dim3((unsigned)((B + BL_T - 1) / BL_T))" in loss
    from mmt_amd import _lib, optim
    assert optim.MAX_GROUPS == A.ADAMW_MAX_GROUPS and int(_lib.LIB.mmt_adamw_chunk_elems()) == A.CHUNK
    assert optim.TENSOR_DTYPE.itemsize == 56 and optim.CHUNK_DTYPE.itemsize == 16


# ------------------------------------------------------------------------------------------------ coverage
WANTED = {"below", "exact", "ragged"}


def test_fusion_case_tables_reach_every_class():
    reach = {
        "query_prep": {A.chunk_class(A.qp_items(*s)) for s in A.QP_SHAPES},
        "query_prep_bwd": {A.chunk_class(A.qpb_items(*s)) for s in A.QPB_SHAPES},
        "relu_drop": {A.chunk_class(n // 8) for n in A.RD_NS},
        "rows_cast": {A.chunk_class(A.rc_items(c, False)) for c in A.RC_CASES},
        "rows_cast_bwd": {A.chunk_class(A.rc_items(c, True)) for c in A.RC_CASES},
    }
    for dup in (0, 1):
        for bwd in (False, True):
            reach["drop_residual%s dup%d" % ("_bwd" if bwd else "", dup)] = {
                A.chunk_class(A.dr_items(s, dup, bwd)) for s, d, _ in A.DR_CASES if d == dup}
    for name, classes in reach.items():
        assert classes >= WANTED, (name, classes)
    assert A.chunk_class(255) == "below" and A.chunk_class(256) == "exact" and A.chunk_class(512) == "multiple"
    assert A.chunk_class(257) == "ragged" and A.chunk_class(1110) == "ragged"
    for shapes in (A.QP_SHAPES, A.QPB_SHAPES, [s for s, _, _ in A.DR_CASES]):
        d8 = {s[2] // 8 for s in shapes}
        assert 1 in d8 and {3, 5} <= d8 and any(v & (v - 1) for v in d8) and 96 in d8
        assert all(s[2] % 8 == 0 for s in shapes)
    assert {s[1] for s in A.QP_SHAPES} >= {1, 5, 37, 400} and {s[0] for s in A.QP_SHAPES} >= {1, 3}
    assert {s[0] for s in A.QPB_SHAPES} == {1, 2, 3, 16} and (2, 400, 768) in A.QP_SHAPES and (2, 400, 768) in A.QPB_SHAPES
    assert all(s[1] % 2 == 0 for s, dup, _ in A.DR_CASES if dup) and any(s[1] % 2 for s, dup, _ in A.DR_CASES if not dup)
    assert {(s, dup) for s, dup, _ in A.DR_CASES} >= {(A.DR_BIG, 0), (A.DR_BIG, 1)}
    for dup in (0, 1):  # every drop form at every small shape
        for s in A.DR_SHAPES:
            if s != A.DR_BIG:
                assert {dr for s2, d2, dr in A.DR_CASES if (s2, d2) == (s, dup)} >= set(A.DROPS)
    assert {c[:4] for c in A.RC_CASES} >= set(A.RC_WINDOWS) and {c[4] for c in A.RC_CASES} >= set(A.RC_CS)
    assert {(w, C) for w in A.RC_WINDOWS for C in A.RC_CS} <= {(c[:4], c[4]) for c in A.RC_CASES}
    assert all(c[2] + c[3] <= c[1] for c in A.RC_CASES)
    assert any(c[2] == 0 and c[3] == c[1] for c in A.RC_CASES) and any(c[2] > 0 and c[2] + c[3] < c[1] for c in A.RC_CASES)
    assert any(c[2] + c[3] == c[1] and c[2] > 0 for c in A.RC_CASES)


def test_drop_forms_are_what_they_claim():
    assert A.drop_params(0.5) == (True, 32768, 2.0)
    on, thr, scale = A.drop_params(0.1)
    assert on and thr == round((1.0 - A.f32(0.1)) * 65536) == 58982 and scale == A.f32(1.0 / (1.0 - A.f32(0.1)))
    assert A.drop_params(0.0)[0] is False and A.drop_params(0.5, rng=False) == (False, 32768, 1.0)
    assert A.drop_params(A.P_THR_FULL) == (True, 65536, 1.0 + 2.0 ** -17)
    assert A.drop_params(A.P_THR_ONE) == (True, 1, 65536.0)
    for p in (A.P_THR_FULL, A.P_THR_ONE, A.P_THR_ROUND):
        assert A.f32(p) == p  # the float argument carries them exactly
    assert (1.0 - A.P_THR_ROUND) * 65536 == 32768.75 and A.drop_params(A.P_THR_ROUND)[1] == 32769
    # the frame's geometry draws 32768 somewhere, so a truncated threshold changes a bit there; and it draws a 0
    r = A.draws(A.ft_key(A.Drop(0.5).seed, 0, 1), int(np.prod(A.DR_BIG)))
    assert int((r == 32768).sum()) > 0 and int((r == 0).sum()) > 0 and r.min() >= 0 and r.max() <= 0xFFFF
    assert abs(float((r < 58982).mean()) - 0.9) < 2e-3
    assert {dr.p for dr in A.RD_DROPS} == {0.5, 0.1, A.P_THR_FULL, A.P_THR_ONE}
    assert [A.drop_params(dr.p, dr.rng)[0] for dr in A.RDB_DROPS] == [True] * 4 + [False, False]
    # the keys differ from the first in exactly one component, and every mask differs from every other
    base = A.KEYS[0]
    for k in A.KEYS[1:]:
        assert sum((k.seed != base.seed, k.counter != base.counter, k.salt != base.salt)) == 1
    assert {k.seed for k in A.KEYS} == {base.seed, (1 << 61) + 12345} and {k.counter for k in A.KEYS} == {0, 1, (1 << 32) + 5}
    assert {k.salt for k in A.KEYS} == {8 * li + j for li in (0, 1) for j in (1, 2, 3)}
    masks = [A.keep_factors((3, 74, 40), k) for k in A.KEYS]
    for i in range(len(masks)):
        for j in range(i):
            assert float((masks[i] != masks[j]).float().mean()) > 0.4, (i, j)
    for s in {s for s, _, _ in A.DR_CASES}:
        assert A.keep_factors(s, A.Drop(0.5)).shape == s


def test_loss_batches_reach_every_category_and_workgroup():
    assert A.LOSS_EXACT_BS == (1, 256, 512) and all(B & (B - 1) == 0 for B in A.LOSS_EXACT_BS)
    assert max(A.LOSS_EXACT_BS) > A.BL_T and A.LOSS_BAR_BS == (3, 257, 300) and 257 > A.BL_T > 3
    assert A.LOSS_W != (2.0, 5.0) and A.LOSS_DLOSS != 1.0
    pred, gt, cats = A.loss_exact_batch(512)
    assert set(cats.tolist()) == set(range(7)) and bool((cats[1:] != cats[:-1]).all())
    for t in (pred, gt):
        assert bool((t * 32 == (t * 32).round()).all())
    b1, b2 = A.loss_boxes(pred, gt)
    assert bool((b1 * 16 == (b1 * 16).round()).all()) and bool((b2 * 16 == (b2 * 16).round()).all())
    wh1, wh2 = b1[:, 2:] - b1[:, :2], b2[:, 2:] - b2[:, :2]
    assert torch.equal(wh1[:, 0] / wh1[:, 1], wh2[:, 0] / wh2[:, 1])      # both atan terms cancel
    mi = torch.min(b1[:, 2:], b2[:, 2:]) - torch.max(b1[:, :2], b2[:, :2])
    iou = A.loss_iou(pred, gt)
    raw = torch.cat([gt[:, :2], gt[:, :2] + gt[:, 2:]], 1)
    is_ = {n: cats == i for i, n in enumerate(A.LOSS_CAT_NAMES)}
    assert bool((mi[is_["disjoint2"]] < 0).all())
    d1 = mi[is_["disjoint1"]]
    assert bool(((d1 < 0).sum(1) == 1).all()) and bool(((d1 > 0).sum(1) == 1).all())
    assert bool((mi[is_["touching"]] == 0).any(1).all()) and bool((iou[is_["touching"]] == 0).all())
    assert bool((b1[is_["shared"]] == b2[is_["shared"]]).any(1).all()) and bool((iou[is_["shared"]] > 0).all())
    assert bool(((raw[is_["clamped"]] < 0) | (raw[is_["clamped"]] > 1)).any(1).all())
    con = is_["contained"]
    assert torch.equal(b1[con, :2] + b1[con, 2:], b2[con, :2] + b2[con, 2:])  # concentric
    assert set(iou[con].tolist()) == {0.25, 0.0625}
    assert bool((iou[is_["iou_high"]] > 0.5).all()) and set(iou[is_["iou_high"]].tolist()) == {0.5625, 0.75}
    assert bool((iou != 1).all())
    for B in A.LOSS_BAR_BS:
        pred, gt = A.loss_random_batch(B)
        assert bool(A.loss_separated(pred, gt).all()) and torch.equal(pred, pred.float().double())
        if B > 100:
            assert 0.4 <= float((A.loss_iou(pred, gt) > 0.5).double().mean()) <= 0.6


def test_adamw_tables_reach_every_path():
    assert A.AW_SIZES == (1, 3, 4, 7, 65535, 65536, 65537, 2 * 65536 + 5) and set(A.AW_GROUPS) == {0, 1, 2}
    chunks = A.aw_chunks()
    assert len(chunks) == 11 and sum(n for _, _, n in chunks) == A.AW_TOTAL == 327700
    kinds = {(n >= 4, n % 4 != 0) for _, _, n in chunks}          # (has whole float4s, has a scalar tail)
    assert kinds == {(False, True), (True, False), (True, True)}
    assert {n for _, _, n in chunks} >= {A.CHUNK, A.CHUNK - 1, 1, 5}
    tails = {i for i, _, n in chunks if n % 4}
    assert tails - set(A.AW_NO_SHADOW) == tails and len(tails) >= 5    # every tensor with a tail has a shadow
    assert {A.AW_SIZES[i] for i in A.AW_NO_SHADOW} == {4, A.CHUNK}
    for g in range(3):  # every group has a tensor of several chunks or a tail, and a tiny one
        assert len([i for i in range(8) if A.AW_GROUPS[i] == g]) >= 2
    assert set(A.AW_LAYOUTS) == {"aligned", "g1", "g2", "g3", "p1", "m1", "v1", "all", "sh1", "sh3"}
    for layout, mis in A.AW_LAYOUTS.items():
        for name, a in A.AW_ALIGN.items():
            starts, total = A.aw_starts(layout, name)
            assert all(s % a == mis.get(name, 0) for s in starts) and total % a == 0
            ends = [s + n for s, n in zip(starts, A.AW_SIZES)]
            assert starts[0] >= A.GUARD and total - ends[-1] >= A.GUARD
            assert all(b - a_ >= A.GUARD for a_, b in zip(ends[:-1], starts[1:]))
    assert set(A.AW_LAYOUTS["all"]) == {"p", "g", "m", "v"} and A.AW_LAYOUTS["sh3"] == {"shadow": 3}
    hp = A.AW_CENSUS_HP
    assert tuple(1.0 - A.f32(l) * A.f32(w) for l, w in zip(hp.lr, hp.wd)) == A.AW_CENSUS_FACTORS == (0.5, 0.25, 1.0)
    for hp in A.AW_UPDATE_HPS.values():
        assert 0.0 in hp.wd and hp.max_norm > 0
    g = A.aw_problem("update")["g"].double()
    norm = float(g.pow(2).sum().sqrt())
    assert A.AW_UPDATE_HPS["clip"].max_norm < norm < A.AW_UPDATE_HPS["noclip"].max_norm and A.AW_UPDATE_STEPS == 3


# ------------------------------------------------------------------------------------------------ exact operands
def test_exact_operands_are_exact():
    for shape in A.QP_SHAPES:
        pr = A.qp_problem(shape, "int")
        assert H.bf16_exact(pr["src"].double() + pr["lpos"].double()) and H.bf16_exact(pr["src"].double())
        assert bool((pr["src"] != 0).all())
    for shape in A.QPB_SHAPES:
        pr = A.qpb_problem(shape, "int")
        tot = pr["dthrough"].double().abs() + pr["dqbi"].double().abs().permute(0, 2, 1, 3) + pr["dsrcb"].double().abs()
        assert H.bf16_exact(tot) and H.f32_exact(pr["dqbi"].double().abs().sum(0))
        dsrc, dlpos = A.qpb_expected(pr, True)
        assert torch.equal(dlpos.double(), pr["dqbi"].double().permute(0, 2, 1, 3).sum(0))
    h = A.rd_problem(2048)["h"].float()
    assert bool((h >= 0).all()) and float(h[h > 0].min()) == A.BF16_MIN_NORMAL == float(torch.finfo(BF16).smallest_normal)
    assert int((h == 0).sum()) >= 512 and float(h.max()) == A.RD_LARGE and A.RD_LARGE * 65536 < float(torch.finfo(BF16).max)
    for steps in (1, 2):
        p, sh = A.aw_census_expected(steps)
        assert torch.equal(sh.float(), p) and torch.equal(p.double(), A.aw_problem("census")["p"].double() *
                                                          A.aw_per_element(A.AW_CENSUS_FACTORS) ** steps)
    pr = A.aw_problem("census")
    assert bool(torch.signbit(pr["g"]).all()) and bool((pr["g"] == 0).all()) and float(pr["p"].abs().max()) <= 100
    # moments: every product and both sums are fp32 numbers, so fused and unfused multiply-adds agree
    pr = A.aw_problem("moments")
    m, v, g = pr["m"].double(), pr["v"].double(), pr["g"].double()
    for steps in (1, 2):
        for t in (0.5 * m, 0.5 * g, 0.75 * v, 0.25 * g, 0.25 * g * g, 0.5 * m + 0.5 * g, 0.75 * v + 0.25 * g * g):
            assert torch.equal(t.float().double(), t)
        m, v = 0.5 * m + 0.5 * g, 0.75 * v + 0.25 * g * g
        want_m, want_v = A.aw_moments_expected(steps)
        assert torch.equal(want_m.double(), m) and torch.equal(want_v.double(), v)
    hp = A.AW_MOMENTS_HP
    assert (A.f32(hp.b1), A.f32(1 - hp.b1), A.f32(hp.b2), A.f32(1 - hp.b2)) == (0.5, 0.5, 0.75, 0.25)
    # one step of the op-by-op restatement gives exactly these moments
    _, m1, v1 = A.adamw_f32(pr["p"], pr["g"], pr["m"], pr["v"], hp, (1.0, 0.5, 0.5))
    assert torch.equal(m1, A.aw_moments_expected(1)[0]) and torch.equal(v1, A.aw_moments_expected(1)[1])
    assert A.CHUNK < 2 ** 24 and A.f32(float(A.AW_TOTAL) ** 0.5) > 0


@pytest.mark.parametrize("cat", A.LOSS_CAT_NAMES)
def test_loss_exact_category_is_the_same_in_fp32_and_fp64(cat):
    """Per category (every variant, at several positions): float32 and float64 autograd agree bit for bit, per sample
    and as a batch.  No category had to move to the bar family."""
    n = 16   # a power of two (the means divide exactly), every variant at least three times
    assert n >= 3 * len(A.LOSS_CATEGORIES[cat])
    pred, gt, _ = A.loss_exact_batch(n, cat)
    for lo, hi in [(0, n)] + [(i, i + 1) for i in range(n)]:
        o64, d64 = A.loss_oracle(pred[lo:hi], gt[lo:hi], F64)
        o32, d32 = A.loss_oracle(pred[lo:hi], gt[lo:hi], F32)
        assert o32.dtype == F32 and d32.dtype == F32
        assert torch.equal(o32.double(), o64) and torch.equal(d32.double(), d64), (lo, hi)
        assert bool(torch.isfinite(d64).all()) and bool((d64.abs().max(1).values > 0).all())


@pytest.mark.parametrize("B", A.LOSS_EXACT_BS)
def test_loss_exact_batches_are_the_same_in_fp32_and_fp64(B):
    pred, gt, ref_out, ref_d = A.loss_reference("exact", B)
    o32, d32 = A.loss_oracle(pred, gt, F32)
    assert torch.equal(o32.double(), ref_out) and torch.equal(d32.double(), ref_d)
    if B > 1:  # neighbours differ
        assert bool((ref_d[1:] != ref_d[:-1]).any(1).all())


# ------------------------------------------------------------------------------------------------ bars
def test_loss_bars_are_four_times_the_float32_composition():
    row = sc = 0.0
    for B in A.LOSS_BAR_BS:
        pred, gt, ref_out, ref_d = A.loss_reference("random", B)
        o32, d32 = A.loss_oracle(pred, gt, F32)
        row, sc = max(row, A.loss_row_err(d32, ref_d)), max(sc, A.loss_scalar_err(o32, ref_out))
    print("train-glue box_loss float32 on the CPU: worst row %.4g, worst scalar %.4g" % (row, sc))
    assert abs(row - A.LOSS_ROW_EMUL) <= 0.05 * A.LOSS_ROW_EMUL and abs(sc - A.LOSS_SCALAR_EMUL) <= 0.05 * A.LOSS_SCALAR_EMUL
    assert A.LOSS_ROW_BAR == 4 * A.LOSS_ROW_EMUL and A.LOSS_SCALAR_BAR == 4 * A.LOSS_SCALAR_EMUL


@pytest.mark.parametrize("clip", sorted(A.AW_UPDATE_HPS))
def test_adamw_float32_restatement_lies_under_the_bars(clip):
    hp = A.AW_UPDATE_HPS[clip]
    pr = A.aw_problem("update")
    norm = A.f32(float(pr["g"].double().pow(2).sum().sqrt()))
    cur = {k: pr[k] for k in "pmv"}
    worst = dict(p=0.0, m=0.0, v=0.0)
    for t in range(1, A.AW_UPDATE_STEPS + 1):
        state = [A.f32(s) for s in A.aw_state_ref(hp, t, norm)]
        assert (state[0] < 1.0) == (clip == "clip")
        p64, m64, v64, bars = A.adamw_ref64(cur["p"], pr["g"], cur["m"], cur["v"], hp, state)
        got = dict(zip("pmv", A.adamw_f32(cur["p"], pr["g"], cur["m"], cur["v"], hp, state)))
        for k, ref in (("p", p64), ("m", m64), ("v", v64)):
            assert got[k].dtype == F32 and bool((bars[k] > 0).all())
            worst[k] = max(worst[k], float(((got[k].double() - ref).abs() / bars[k]).max()))
        cur = got
    print("train-glue adamw float32 restatement (%s): worst error / bar p %.3f m %.3f v %.3f" %
          (clip, worst["p"], worst["m"], worst["v"]))
    assert max(worst.values()) <= 1.0 and min(worst.values()) > 0.02, worst   # met, and not by a wide margin
    assert (A.AW_N_M, A.AW_N_V, A.AW_N_P) == (4, 6, 21)


# ------------------------------------------------------------------------------------------------ planted defects
def _differs(a, b, width):
    """The GPU test's comparison (gemm_probes.same on storage images) tells the two apart."""
    dt = a.dtype
    return not P.same(H.image(a.numel() // width, width, a, dt), H.image(b.numel() // width, width, b, dt))


def test_planted_defects_of_the_fusion_kernels_fail():
    for shape in A.QP_SHAPES:
        for family in A.QP_FAMILIES:
            pr = A.qp_problem(shape, family)
            assert _differs(A.qp_expected(pr, "halves_swapped")[0], A.qp_expected(pr)[0], 2 * shape[2]), shape
            assert not _differs(A.qp_expected(pr, "halves_swapped")[1], A.qp_expected(pr)[1], shape[2])
    for shape in A.QPB_SHAPES:
        for family in A.QP_FAMILIES:
            pr = A.qpb_problem(shape, family)
            assert _differs(A.qpb_expected(pr, True, "no_last_sample")[1], A.qpb_expected(pr, True)[1], shape[2]), shape
            assert _differs(A.qpb_expected(pr, False)[0], A.qpb_expected(pr, True)[0], shape[2])
    seen = set()
    for shape, dup, dr in A.DR_CASES:
        on, thr, _ = A.drop_params(dr.p, dr.rng)
        if not on or thr in (1, 65536) or int(np.prod(shape)) < 64:
            continue   # no draws, or a threshold that every draw (or almost none) passes whatever its position
        pr = A.dr_problem(shape, dup)
        d = shape[2]
        for mut in ("salt_ignored", "fields_reversed"):
            assert _differs(A.dr_expected(pr, dup, dr, mut), A.dr_expected(pr, dup, dr), d), (shape, dup, dr, mut)
            assert _differs(A.drb_expected(pr, dup, dr, mut), A.drb_expected(pr, dup, dr), d), (shape, dup, dr, mut)
        if dup:
            assert _differs(A.drb_expected(pr, dup, dr, "mask_at_dy"), A.drb_expected(pr, dup, dr), d), (shape, dr)
        seen.add((shape, dup))
    assert len(seen) >= 12 and (A.DR_BIG, 1) in seen
    # dup backward: the halves carry different gradients, so reading a half with the other's mask shows as well
    pr = A.dr_problem((3, 74, 40), 1)
    assert float((pr["dout"][:, :37] != pr["dout"][:, 37:]).float().mean()) == 1.0
    # the two edge thresholds at the frame's geometry: thr 1 keeps the draws of 0 alone, thr 32769 one draw more than 32768
    pr = A.dr_problem(A.DR_BIG, 0)
    kept = A.keep_factors(A.DR_BIG, A.Drop(A.P_THR_ONE))
    assert 0 < int((kept != 0).sum()) < 100 and float(kept.max()) == 65536.0
    a, b = A.keep_factors(A.DR_BIG, A.Drop(A.P_THR_ROUND)), A.keep_factors(A.DR_BIG, A.Drop(0.5))
    assert int(((a != 0) != (b != 0)).sum()) == int((A.draws(A.ft_key(A.Drop(0.5).seed, 0, 1), a.numel()) == 32768).sum()) > 0
    assert bool((A.keep_factors((3, 74, 40), A.Drop(A.P_THR_FULL)) == 1.0 + 2.0 ** -17).all())
    for n in A.RD_NS[1:]:
        pr = A.rd_problem(n)
        for dr in A.RD_DROPS[:2]:
            for mut in ("salt_ignored", "fields_reversed"):
                assert _differs(A.rd_expected(pr, dr, mut), A.rd_expected(pr, dr), 8), (n, dr, mut)
                assert _differs(A.rdb_expected(pr, dr, mut), A.rdb_expected(pr, dr), 8), (n, dr, mut)
    for case in A.RC_CASES:
        pr = A.rc_problem(case)
        if case[3] < case[1]:
            assert _differs(A.rc_expected(case, pr, "window_unwritten")[1], A.rc_expected(case, pr)[1], case[4]), case


def test_planted_defects_of_the_loss_fail():
    pred, gt, ref_out, ref_d = A.loss_reference("exact", 256)
    cats = A.loss_exact_batch(256)[2]
    out, d = A.loss_oracle(pred, gt, F64, "sample_dropped")
    assert bool((out.float() != ref_out.float()).all()) and bool((d.float() != ref_d.float()).any(1).all())
    out, d = A.loss_oracle(pred, gt, F64, "tie_one_zero")
    moved = (d.float() != ref_d.float()).any(1)
    tied = (A.loss_boxes(pred, gt)[0] == A.loss_boxes(pred, gt)[1]).any(1)
    assert bool(moved[cats == A.LOSS_CAT_NAMES.index("shared")].all()) and torch.equal(moved, tied)
    for B in A.LOSS_BAR_BS:
        pred, gt, ref_out, ref_d = A.loss_reference("random", B)
        out, d = A.loss_oracle(pred, gt, F64, "sample_dropped")
        assert A.loss_row_err(d, ref_d) > 100 * A.LOSS_ROW_BAR and A.loss_scalar_err(out, ref_out) > 100 * A.LOSS_SCALAR_BAR


def test_planted_defects_of_adamw_fail():
    for layout in A.AW_LAYOUTS:
        for steps in (1, 2):
            want_p, want_sh = A.aw_census_expected(steps)
            good = A.aw_image(want_p, layout, "p", F32)
            for mut in ("chunk_last_skipped", "group_zero"):
                bad_p, bad_sh = A.aw_census_expected(steps, mut)
                assert not P.same(A.aw_image(bad_p, layout, "p", F32), good), (layout, mut)
                assert not P.same(A.aw_shadow_image(bad_sh, layout), A.aw_shadow_image(want_sh, layout)) or mut == "chunk_last_skipped"
            assert not P.same(A.aw_shadow_image(want_sh, layout, "tail_unwritten"), A.aw_shadow_image(want_sh, layout)), layout
            # a second touch of one element in a step shows
            twice = want_p.clone()
            twice[70000] *= A.AW_CENSUS_FACTORS[A.AW_GROUPS[4]]
            assert not P.same(A.aw_image(twice, layout, "p", F32), good)
    want_p, _ = A.aw_census_expected(1)
    bad_p, _ = A.aw_census_expected(1, "group_zero")
    wrong = {A.AW_GROUPS[i] for i, (s, n) in enumerate(zip(np.cumsum((0,) + A.AW_SIZES[:-1]), A.AW_SIZES))
             if not torch.equal(want_p[s:s + n], bad_p[s:s + n])}
    assert wrong == {1, 2}


# ------------------------------------------------------------------------------------------------ host rejections
FAKE = 1 << 20  # 16-byte aligned, never dereferenced: every call below fails validation before a launch


def _lib():
    from mmt_amd import _lib
    return _lib


def test_fusion_entry_points_reject_bad_arguments_on_the_host():
    L = _lib().LIB
    E = A.EBADARG

    def qp(src=FAKE, lpos=FAKE, qbi=FAKE, srcb=FAKE, B=2, nq=4, d=16):
        return L.mmt_ft_query_prep(src, lpos, qbi, srcb, B, nq, d, None)

    def qpb(dqbi=FAKE, dsrcb=FAKE, dthrough=FAKE, dsrc=FAKE, dlpos=FAKE, B=2, nq=4, d=16):
        return L.mmt_ft_query_prep_bwd(dqbi, dsrcb, dthrough, dsrc, dlpos, B, nq, d, None)

    for f, ptrs, nullable in ((qp, ("src", "lpos", "qbi", "srcb"), ()), (qpb, ("dqbi", "dsrcb", "dthrough", "dsrc", "dlpos"), ("dthrough",))):
        for name in ptrs:
            if name not in nullable:
                assert f(**{name: None}) == E, name
            for off in (2, 4, 8):
                assert f(**{name: FAKE + off}) == E, (name, off)
        for d in (0, -8, 4, 12, 17):
            assert f(d=d) == E, d
        assert f(B=0) == E and f(B=-1) == E and f(nq=0) == E and f(nq=-3) == E

    def dr(x=FAKE, y=FAKE, out=FAKE, rng=FAKE, p=0.5, B=2, rows=4, d=16, dup=0):
        return L.mmt_ft_drop_residual(x, y, out, rng, 1, p, B, rows, d, dup, None)

    def drb(dout=FAKE, dy=FAKE, rng=FAKE, p=0.5, B=2, rows=4, d=16, dup=0):
        return L.mmt_ft_drop_residual_bwd(dout, dy, rng, 1, p, B, rows, d, dup, None)

    for f, ptrs in ((dr, ("x", "y", "out")), (drb, ("dout", "dy"))):
        for name in ptrs:
            assert f(**{name: None}) == E, name
            for off in (2, 4, 8):
                assert f(**{name: FAKE + off}) == E, (name, off)
        for d in (0, -8, 4, 12):
            assert f(d=d) == E, d
        assert f(B=0) == E and f(B=-2) == E and f(rows=0) == E and f(rows=-4) == E
        for rows in (1, 3, 5):
            assert f(rows=rows, dup=1) == E, rows
        for p in (-0.1, -1e-9, 1.0, 1.5):
            assert f(p=p) == E and f(p=p, rng=None) == E, p

    def rd(h=FAKE, out=FAKE, rng=FAKE, p=0.5, n=64):
        return L.mmt_ft_relu_drop(h, out, rng, 1, p, n, None)

    def rdb(dy=FAKE, h=FAKE, dh=FAKE, rng=FAKE, p=0.5, n=64):
        return L.mmt_ft_relu_drop_bwd(dy, h, dh, rng, 1, p, n, None)

    for f, ptrs in ((rd, ("h", "out", "rng")), (rdb, ("dy", "h", "dh"))):
        for name in ptrs:
            assert f(**{name: None}) == E, name
            if name != "rng":
                for off in (2, 4, 8):
                    assert f(**{name: FAKE + off}) == E, (name, off)
        for n in (0, -8, 1, 4, 12, 63, 65):
            assert f(n=n) == E, n
        for p in (-0.1, 1.0, 1.5):
            assert f(p=p) == E, p
    assert rd(p=0.0) == E and rd(rng=None, p=0.5) == E   # the forward is not a copy: without dropout it is not called

    def rc(x=FAKE, out=FAKE, S=2, rows=8, row0=2, nrows=4, C=16):
        return L.mmt_ft_rows_cast(x, out, S, rows, row0, nrows, C, None)

    def rcb(dout=FAKE, dx=FAKE, S=2, rows=8, row0=2, nrows=4, C=16):
        return L.mmt_ft_rows_cast_bwd(dout, dx, S, rows, row0, nrows, C, None)

    for f, ptrs in ((rc, ("x", "out")), (rcb, ("dout", "dx"))):
        for name in ptrs:
            assert f(**{name: None}) == E, name
            for off in (2, 4, 8):
                assert f(**{name: FAKE + off}) == E, (name, off)
        for C in (0, -8, 4, 12, 17):
            assert f(C=C) == E, C
        assert f(S=0) == E and f(S=-1) == E and f(rows=0) == E and f(nrows=0) == E and f(nrows=-1) == E and f(row0=-1) == E
        for row0, nrows in ((5, 4), (8, 1), (0, 9), (7, 2)):
            assert f(row0=row0, nrows=nrows) == E, (row0, nrows)


def test_loss_and_adamw_reject_bad_arguments_on_the_host():
    L = _lib().LIB
    E = A.EBADARG

    def bl(pred=FAKE, gt=FAKE, out=FAKE, B=4):
        return L.mmt_box_loss(pred, gt, out, B, 2.0, 5.0, None)

    def blb(pred=FAKE, gt=FAKE, dloss=FAKE, dpred=FAKE, B=4):
        return L.mmt_box_loss_bwd(pred, gt, dloss, dpred, B, 2.0, 5.0, None)

    for f, ptrs in ((bl, ("pred", "gt", "out")), (blb, ("pred", "gt", "dloss", "dpred"))):
        for name in ptrs:
            assert f(**{name: None}) == E, name
        assert f(B=0) == E and f(B=-1) == E

    lr, wd = (ctypes.c_float * 9)(*([1e-3] * 9)), (ctypes.c_float * 9)(*([1e-2] * 9))
    lrp, wdp = ctypes.cast(lr, ctypes.c_void_p), ctypes.cast(wd, ctypes.c_void_p)

    def aw(tensors=FAKE, chunks=FAKE, nchunks=3, partial=FAKE, state=FAKE, lr=lrp, wd=wdp, ngroups=3):
        return L.mmt_adamw_step(tensors, chunks, nchunks, partial, state, lr, wd, ngroups, 0.9, 0.999, 1e-8, 1.0, 1, None)

    for name in ("tensors", "chunks", "partial", "state", "lr", "wd"):
        assert aw(**{name: None}) == E, name
    for nchunks in (0, -1):
        assert aw(nchunks=nchunks) == E
    for ngroups in (0, -1, A.ADAMW_MAX_GROUPS + 1):
        assert aw(ngroups=ngroups) == E, ngroups
