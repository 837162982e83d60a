"""The normalisation probes themselves (tests/norm_probes.py), on the CPU: the constants are the sources', the case
tables reach every value, pair and path class they claim, the operands the bitwise families call exact are exact, a
plain fp32 restatement of each kernel's arithmetic lies within every bar (so a correct fp32 kernel can meet them), one
planted defect moves the named output past its bar, and the C ABI rejects every host-checkable bad argument before
any launch."""
import os

import pytest
import torch

import norm_probes as N
from conftest import ROOT

F64, F32, BF16, F16 = N.F64, N.F32, N.BF16, N.F16


def test_constants_match_the_library_sources():
    hdr = open(os.path.join(ROOT, "include", "mmt_hip.h")).read()
    assert "#define MMT_EBADARG (%d)" % N.EBADARG in hdr
    src = open(os.path.join(ROOT, "multi-modal-tracking_amd", "csrc", "norm.hip")).read()
    assert "constexpr int LNB_RPW = %d;" % N.LNB_RPW in src and N.LNB_RPW == 32
    assert "constexpr int GN_THREADS = %d, GN_VMAX = %d;" % (N.GN_THREADS, N.GN_VMAX) in src
    assert (N.GN_THREADS, N.GN_VMAX) == (512, 12)
    assert "constexpr int GNB_LDS = 2 * 9600;" in src and N.GNB_LDS == 2 * 9600
    assert "for (; b + %d <= b1; b += %d)" % (N.RED_UNROLL, N.RED_UNROLL) in src and N.RED_UNROLL == 16
    assert "(int64_t)(run + 1) * nwg / %d" % N.RED_RUNS in src and "__shared__ float red[%d][64];" % N.RED_RUNS in src
    assert N.RED_RUNS == 4
    assert "const int PC = GNB_LDS / (2 * cg);" in src
    assert "const bool second = g1 && ((row / rpg) & 1);" in src and "const bool second = g1 && inst >= inst_per_set;" in src


# ------------------------------------------------------------------------------------------------ coverage
def test_layernorm_cases_reach_every_value_and_pair():
    cs = N.LN_CASES
    assert {c.C for c in cs} == {256, 512, 768, 1024} and {c.dtype for c in cs} == {"f32", "bf16", "fp16"}
    assert {c.rows for c in cs} == {1, 3, 4, 5, 50} and {c.rows % 4 for c in cs} == {0, 1, 2, 3}
    assert {c.variant for c in cs} == set(N.VARIANTS) and {(c.C, c.variant) for c in cs} >= {(C, v) for C in N.LN_CS for v in N.VARIANTS}
    forms = {(c.sets, c.rpg if c.sets == "two" else 0) for c in cs if c.rows == 50}
    assert forms == {("none0", 0), ("none_rows", 0), ("two", 1), ("two", 7), ("two", 25)}
    assert {c.add_rows for c in cs if c.rows == 50} == {0, 1, 7, 25, 50}
    assert {c.out for c in cs} == set(N.LN_OUTS)
    pairs = {(c.sets, c.rpg if c.sets == "two" else 0, c.add_rows) for c in cs if c.rows == 50}
    assert len(pairs) == 25
    assert {(c.out, c.dtype) for c in cs} == {(o, d) for o in N.LN_OUTS for d in N.DTYPES}
    assert {c.add_rows > 0 for c in cs if c.out.startswith("inplace")} == {False, True}  # in place with and without add
    returns = {}
    for c in cs:
        if c.sets == "two" and c.rows == 50:  # the alternation returns to set 0 at least twice (rows_per_group 1, 7) ...
            sel = N.ln_problem(c)["sel"]
            assert bool(sel.any()) and not bool(sel[0])
            returns[c.rpg] = int((sel[:-1] & ~sel[1:]).sum())
    assert returns == {1: 24, 7: 3, 25: 0}
    # ... and a set boundary falls inside a 4-row workgroup; 7 pins row % add_rows against every rows_per_group
    assert any(c.sets == "two" and c.rpg % 4 for c in cs) and 50 % 7 and 7 not in (1, 25)
    assert {c.eps for c in cs} == {1e-5, 1e-6}


def test_layernorm_backward_cases_reach_every_reduce_path():
    cs = N.LNB_CASES
    assert {c.dtype for c in cs} == set(N.DTYPES) and {c.dres for c in cs} == set(N.LNB_DRES)
    assert {c.variant for c in cs} == set(N.VARIANTS)
    assert {(c.rows, c.C) for c in cs} >= {(r, C) for r in N.LNB_SMALL_ROWS for C in N.LN_CS}
    assert {(c.rows, c.C) for c in cs} >= {(r, C) for r in N.LNB_BIG_ROWS for C in N.LNB_BIG_CS}
    assert {c.rpg for c in cs} == {0, 1, 5, 40, 500}
    nwgs = sorted({c.nwg for c in cs})
    assert nwgs == [1, 2, 3, 63, 64, 65]
    assert N.reduce_classes(nwgs) == {(False, False), (False, True), (True, False), (True, True)}
    assert N.reduce_runs(63) == [(0, 15), (1, 0), (1, 0), (1, 0)] and N.reduce_classes([64]) == {(True, False)}
    assert N.reduce_classes([65]) == {(True, False), (True, True)} and (False, False) in N.reduce_classes([1, 2, 3])
    # one wave accumulates both sets inside a workgroup, and a workgroup lies wholly in set 1
    both = whole = False
    for c in cs:
        if not c.rpg:
            continue
        sel = torch.zeros(c.nwg * N.LNB_RPW, dtype=torch.bool)
        sel[:c.rows] = N.lnb_problem(c)["sel"]
        live = torch.zeros_like(sel)
        live[:c.rows] = True
        w = sel.view(c.nwg, N.LNB_RPW // 4, 4)
        lv = live.view(c.nwg, N.LNB_RPW // 4, 4)
        both |= bool(((w & lv).any(1) & (~w & lv).any(1)).any())
        whole |= bool((w | ~lv).view(c.nwg, -1).all(1).any())
    assert both and whole


def test_groupnorm_cases_reach_every_item_count_and_chunk_class():
    cs = N.GN_CASES
    assert {(c.P, c.Ctot, c.groups) for c in cs} >= set(N.GN_SHAPES) | {(400, 768, 32)}
    items = {c.items for c in cs}
    assert {1, N.GN_THREADS, N.GN_THREADS + 1, N.GN_THREADS * N.GN_VMAX} <= items and max(items) == 6144
    assert {c.cg // 4 for c in cs} >= {5, 6} and max(c.cg for c in cs) == N.GN_THREADS
    assert {(c.out, c.dtype) for c in cs} == {(o, d) for o in N.GN_OUTS for d in N.DTYPES}
    assert {c.ips for c in cs if c.n_inst == 3 and c.two} == {0, 1, 2, 3} and any(c.n_inst == 3 and not c.two for c in cs)
    assert [N.gn_sets(N.GNCase(1, 4, 1, 3, i, True, "f32", "f32", "randn")).tolist() for i in range(4)] == [
        [False] * 3, [False, True, True], [False, False, True], [False] * 3]
    assert {c.variant for c in cs} == set(N.VARIANTS)
    bs = N.GNB_CASES
    assert {c.n_inst for c in bs} == {1, 3} and {c.variant for c in bs} == set(N.VARIANTS)
    assert {(c.cg, c.P) for c in bs} >= {(24, 399), (24, 400), (24, 401), (24, 1024), (32, 576), (32, 768), (28, 343),
                                          (256, 37), (256, 38), (256, 96)} and any(c.cg == 4 for c in bs)
    assert {c.cg: c.pc for c in bs} == {4: 2400, 24: 400, 32: 300, 28: 342, 256: 37} and N.GNB_LDS % (2 * 28)
    assert {c.chunks for c in bs} == {1, 2, 3} and {N.chunk_class(c) for c in bs} == {"one", "full", "partial"}
    for c in bs:
        assert c.P * c.cg // 4 <= N.GN_THREADS * N.GN_VMAX and 2 * c.cg <= N.GN_THREADS and 2 * c.pc * c.cg <= N.GNB_LDS
    assert any(2 * c.cg == N.GN_THREADS for c in bs)


def test_staging_cases_reach_every_value():
    cs = N.AC_CASES
    assert {c.n for c in cs} == {4, 1020, 1024, 1028} and all(c.n % 4 == 0 for c in cs)
    assert {(c.n, c.add_n) for c in cs} >= {(n, a) for n in N.AC_NS for a in (0, 4, n)} | {(1028, 24)} and 1028 % 24
    assert {(c.out, c.dtype) for c in cs} == {(o, d) for o in N.GN_OUTS for d in N.DTYPES}
    used = set()
    for c in cs:
        used |= {k for _, k in N.ac_problem(c)["slots"]}
    assert used == set(range(len(N.PLANTED)))
    assert {(r, c) for r, c, _, _ in N.SR_CASES} == {(1, 8), (5, 264), (33, 768)}
    assert {rp for _, _, rp, _ in N.SR_CASES} == {1, 2, 33, 100} and {d for _, _, _, d in N.SR_CASES} == {"bf16", "fp16"}
    seen = set()
    for case in N.SR_CASES:
        seen |= set(N.sr_problem(case)["scale"].tolist())
    assert seen == {float(torch.tensor(s, dtype=F32)) for s in N.SR_SCALES}
    assert set(N.PI_CASES) == {(1, 8, 16, 4, 2), (1, 24, 40, 8, 2), (2, 16, 32, 16, 1), (3, 32, 48, 16, 2)}


# ------------------------------------------------------------------------------------------------ planted operands
def _is_tie(v, dtype):
    """v (fp32) lies exactly halfway between two neighbouring values of dtype."""
    r = v.to(dtype).float()
    other = v + (v - r)
    return bool(r != v) and bool(other.to(dtype).float() == other) and bool((r - v).abs() == (other - v).abs())


def test_planted_values_are_what_they_claim():
    sums = [torch.tensor(a, dtype=F32) + torch.tensor(b, dtype=F32) for a, b in N.PLANTED]
    for (a, b), s in zip(N.PLANTED, sums):  # a, b and a + b are fp32 values
        assert float(torch.tensor(a, dtype=F32)) == a and float(torch.tensor(b, dtype=F32)) == b and float(s) == a + b
    for ties, dtype in ((N.BF16_TIES, BF16), (N.F16_TIES, F16)):
        up = set()
        for k, odd in ties:
            assert _is_tie(sums[k], dtype), k
            rounded_up = abs(float(sums[k].to(dtype))) > abs(float(sums[k]))
            assert rounded_up == odd, k      # ties go to the even neighbour: up exactly where the lower one is odd
            up.add(rounded_up)
        assert up == {False, True}
    inf = float("inf")
    assert [float(sums[k].to(F16)) for k in range(8, 15)] == [65504.0, inf, inf, -65504.0, -inf, 65504.0, -65504.0]
    assert all(torch.isfinite(sums[k].to(BF16)) for k in range(8, 15))
    for k in range(15, 23):  # at or below fp16's subnormal range: the cast lands on a multiple of 2^-24 below 2^-14
        h = float(sums[k].to(F16))
        assert abs(h) < 2.0 ** -14 or k == 22, k
        assert h / 2.0 ** -24 == round(h / 2.0 ** -24)
    assert float(sums[16].to(F16)) == 2.0 ** -23 and float(sums[17].to(F16)) == 2.0 ** -23 and _is_tie(sums[16], F16)
    assert float(sums[19].to(F16)) == 0.0 and float(sums[20].to(F16)) == 2.0 ** -24 and float(sums[18].to(F16)) == -1023 * 2.0 ** -24
    assert float(sums[22].to(F16)) == 514 * 2.0 ** -24


@pytest.mark.parametrize("c", N.AC_CASES, ids=N.ac_id)
def test_add_cast_operands(c):
    pr = N.ac_problem(c)
    assert pr["x"].dtype == F32 and pr["want"].dtype == F32 and len(pr["slots"]) == min(len(N.PLANTED), c.n // 4)
    for e, k in pr["slots"]:
        a, b = N.PLANTED[k]
        assert float(pr["want"][e]) == a + b, (e, k)
        if c.add_n:
            assert float(pr["x"][e]) == a and float(pr["add"][e % c.add_n]) == b
    if c.add_n:
        ref = pr["x"].double() + pr["add"].double()[torch.arange(c.n) % c.add_n]
        assert float((pr["want"].double() - ref).abs().max()) <= 2.0 ** -24 * float(ref.abs().max())
        assert int((pr["add"] != 0).sum()) >= c.add_n // 2


def test_backward_gradients_are_exact_integers():
    for c in N.LNB_CASES:
        pr, ref = N.lnb_problem(c), N.lnb_reference(c)
        for t in (pr["dy"], pr["dres"], pr["prefill"]):
            if t is not None:
                assert bool((t == t.round()).all()) and bool((t != 0).all()) and float(t.abs().max()) <= 9
        assert float(pr["dy"].abs().max()) <= 3
        assert torch.equal(pr["dy"].to(BF16).float(), pr["dy"]) and torch.equal(pr["dy"].to(F16).float(), pr["dy"])
        dbeta = ref["dgb"][1::2]
        assert bool((dbeta == dbeta.round()).all()) and 3 * c.rows < 2 ** 24
        assert torch.equal(ref["dbeta_part"].sum(0)[:c.sets], dbeta)
    for c in N.GNB_CASES:
        pr, ref = N.gnb_problem(c), N.gnb_reference(c)
        assert bool((pr["dy"] == pr["dy"].round()).all()) and bool((pr["dy"] != 0).all()) and float(pr["dy"].abs().max()) <= 3
        assert torch.equal(ref["dbeta_part"].sum(0), ref["dgb"][1]) and 3 * c.P * c.n_inst < 2 ** 24


@pytest.mark.parametrize("case", N.PI_CASES, ids=str)
def test_patch_im2col_reference(case):
    """The coded images hold distinct integers, the index restatement equals F.unfold, and the two swaps move it."""
    imgs = N.pi_problem(case, True)
    allv = torch.cat([t.reshape(-1) for t in imgs.values()])
    assert allv.unique().numel() == allv.numel() and float(allv.max()) < 2 ** 24 and bool((allv == allv.round()).all())
    Bm, ht, hs, patch, nmod = case
    ref = N.pi_reference(case, imgs)
    assert ref.shape == (nmod * Bm * (2 * (ht // patch) ** 2 + (hs // patch) ** 2), 3 * patch * patch)
    assert torch.equal(N.restate_pi(case, imgs), ref)
    for mut in ("swap_to", "swap_kyx"):
        assert not torch.equal(N.restate_pi(case, imgs, mut), ref), mut
    rnd = N.pi_problem(case, False)
    assert torch.equal(N.restate_pi(case, rnd), N.pi_reference(case, rnd))
    for dt in (BF16, F16):
        assert not torch.equal(N.restate_pi(case, rnd, "swap_to").to(dt), N.pi_reference(case, rnd).to(dt))


# ------------------------------------------------------------------------------------------------ bars hold, mutations move
def _over(got, ref, bar):
    return float(((got.double() - ref).abs() / bar).max())


def _fwd_bars(c, ref, d):
    out = [torch.full_like(ref, d)] if c.has_f32 else []
    if c.has_typed:
        out.append(N.bar(ref, d, N.DT[c.dtype]))
    return out


@pytest.mark.parametrize("c", N.LN_CASES, ids=N.ln_id)
def test_layernorm_bar_holds_and_mutations_pass_it(c):
    ref, d = N.ln_reference(c)
    assert d > 0 and float((N.restate_ln(c, F64) - ref).abs().max()) <= 1e-11 * max(1.0, float(ref.abs().max()))
    y32 = N.restate_ln(c, F32)
    assert y32.dtype == F32
    assert _over(y32, ref, torch.full_like(ref, d)) <= 1.0, _over(y32, ref, torch.full_like(ref, d))
    if c.has_typed:
        dt = N.DT[c.dtype]
        assert _over(y32.to(dt), ref, N.bar(ref, d, dt)) <= 1.0
    for mut in N.ln_mutations(c):
        got = N.restate_ln(c, F32 if mut == "one_pass" else F64, mut)
        for b in _fwd_bars(c, ref, d):
            assert _over(got, ref, b) > 1.0, (mut, _over(got, ref, b))


def test_layernorm_mutations_are_all_exercised():
    seen = set()
    for c in N.LN_CASES:
        seen |= {(m, c.variant) for m in N.ln_mutations(c)}
    assert {m for m, _ in seen} == {"skip_mean", "one_pass", "eps", "gamma_set", "beta_set", "add_map", "neighbour"}
    assert ("one_pass", "offset") in seen and ("eps", "small") in seen
    assert sum("add_map" in N.ln_mutations(c) for c in N.LN_CASES) >= 6


@pytest.mark.parametrize("c", N.GN_CASES, ids=N.gn_id)
def test_groupnorm_bar_holds_and_mutations_pass_it(c):
    ref, d = N.gn_reference(c)
    assert d > 0 and float((N.restate_gn(c, F64) - ref).abs().max()) <= 1e-11 * max(1.0, float(ref.abs().max()))
    y32 = N.restate_gn(c, F32)
    assert y32.dtype == F32
    assert _over(y32, ref, torch.full_like(ref, d)) <= 1.0, _over(y32, ref, torch.full_like(ref, d))
    if c.has_typed:
        dt = N.DT[c.dtype]
        assert _over(y32.to(dt), ref, N.bar(ref, d, dt)) <= 1.0
    for mut in N.gn_mutations(c):
        got = N.restate_gn(c, F32 if mut == "one_pass" else F64, mut)
        for b in _fwd_bars(c, ref, d):
            assert _over(got, ref, b) > 1.0, (mut, _over(got, ref, b))


def test_groupnorm_mutations_are_all_exercised():
    seen = set()
    for c in N.GN_CASES:
        seen |= set(N.gn_mutations(c))
    assert seen == {"skip_mean", "one_pass", "eps", "neighbour", "gamma_set", "beta_set"}


@pytest.mark.parametrize("c", N.LNB_CASES, ids=N.lnb_id)
def test_layernorm_backward_bars_hold_and_mutations_pass_them(c):
    ref = N.lnb_reference(c)
    dx64, dgb64 = N.restate_lnb(c, F64)
    assert float((dx64 - ref["dx"]).abs().max()) <= 1e-10 * max(1.0, float(ref["dx"].abs().max()))
    assert float((dgb64 - ref["dgb"]).abs().max()) <= 1e-10 * max(1.0, float(ref["dgb"].abs().max()))
    dx32, dgb32 = N.restate_lnb(c, F32)
    assert dx32.dtype == F32 and dgb32.dtype == F32
    assert _over(dx32, ref["dx"], torch.full_like(ref["dx"], ref["delta"])) <= 1.0
    assert torch.equal(dgb32[1::2].double(), ref["dgb"][1::2])
    assert bool((ref["dgamma_bar"] > 0).all()) or c.rows <= c.rpg
    live = ref["dgamma_bar"] > 0
    assert float(((dgb32[0::2].double() - ref["dgb"][0::2]).abs()[live] / ref["dgamma_bar"][live]).max()) <= 1.0
    muts = ["mg_no_gamma"] + (["drop_row"] if c.rows > 1 else []) + (["no_dres"] if c.dres != "none" else [])
    if c.rpg and c.rows > c.rpg:
        muts.append("row_other_set")
    for mut in muts:
        dx, dgb = N.restate_lnb(c, F64, mut)
        if mut in ("mg_no_gamma", "no_dres"):
            assert _over(dx, ref["dx"], torch.full_like(ref["dx"], ref["delta"])) > 1.0, mut
        else:
            assert not torch.equal(dgb[1::2], ref["dgb"][1::2]), mut
            assert float(((dgb[0::2] - ref["dgb"][0::2]).abs() / ref["dgamma_bar"].clamp(min=1e-30)).max()) > 1.0, mut


@pytest.mark.parametrize("c", N.GNB_CASES, ids=N.gnb_id)
def test_groupnorm_backward_bars_hold_and_mutations_pass_them(c):
    ref = N.gnb_reference(c)
    dx64, dgb64 = N.restate_gnb(c, F64)
    assert float((dx64 - ref["dx"]).abs().max()) <= 1e-10 * max(1.0, float(ref["dx"].abs().max()))
    assert float((dgb64 - ref["dgb"]).abs().max()) <= 1e-10 * max(1.0, float(ref["dgb"].abs().max()))
    dx32, dgb32 = N.restate_gnb(c, F32)
    assert dx32.dtype == F32 and dgb32.dtype == F32
    assert _over(dx32, ref["dx"], torch.full_like(ref["dx"], ref["delta"])) <= 1.0
    assert torch.equal(dgb32[1].double(), ref["dgb"][1])
    assert float(((dgb32[0].double() - ref["dgb"][0]).abs() / ref["dgamma_bar"]).max()) <= 1.0
    dx, _ = N.restate_gnb(c, F64, "mg_no_gamma")
    assert _over(dx, ref["dx"], torch.full_like(ref["dx"], ref["delta"])) > 1.0
    _, dgb = N.restate_gnb(c, F64, "drop_pos")
    assert not torch.equal(dgb[1], ref["dgb"][1])       # dbeta is compared bitwise: one missing integer always shows
    # dgamma's bar is a worst case over a chain of P + n_inst additions: up to 1024 positions it stays below one term
    # (|dy xhat| of the dropped position), at 6144 positions it cannot, and dbeta alone names the defect
    moved = float(((dgb[0] - ref["dgb"][0]).abs() / ref["dgamma_bar"]).max()) > 1.0
    assert moved or c.P > 1024


# ------------------------------------------------------------------------------------------------ host rejections
FAKE = 1 << 20  # 16-byte aligned, never dereferenced: every call below fails validation before a launch


def _lib():
    from mmt_amd import _lib
    return _lib


def test_layernorm_rejects_bad_arguments_on_the_host():
    L = _lib()

    def call(x=FAKE, add=None, add_rows=0, of=FAKE, ot=FAKE, g0=FAKE, b0=FAKE, g1=None, b1=None, rows=8, rpg=0, C=256,
             dtype=L.MMT_BF16):
        return L.LIB.mmt_layernorm(x, add, add_rows, of, ot, g0, b0, g1, b1, rows, rpg, C, 1e-6, dtype, None)

    for name in ("x", "g0", "b0"):
        assert call(**{name: None}) == N.EBADARG, name
    for rows in (0, -1):
        assert call(rows=rows) == N.EBADARG
    for C in (0, 128, 255, 257, 384, 1280, 2048, -256):
        assert call(C=C) == N.EBADARG, C
    assert call(add=FAKE, add_rows=0) == N.EBADARG and call(add=FAKE, add_rows=-3) == N.EBADARG
    assert call(g1=FAKE, b1=None, rpg=4) == N.EBADARG
    assert call(g1=FAKE, b1=FAKE, rpg=0) == N.EBADARG and call(g1=FAKE, b1=FAKE, rpg=-2) == N.EBADARG
    for dtype in (L.MMT_F64, 4, 7, -1):
        assert call(dtype=dtype) == N.EBADARG, dtype


def test_layernorm_backward_rejects_bad_arguments_on_the_host():
    L = _lib()

    def add(x=FAKE, dy=FAKE, dt=L.MMT_BF16, g0=FAKE, g1=None, dres=None, dx=FAKE, dgb=FAKE, ws=FAKE, wsf=None, rows=40,
            rpg=0, C=256):
        wsf = (rows + 31) // 32 * 4 * C if wsf is None else wsf
        return L.LIB.mmt_layernorm_bwd_add(x, dy, dt, g0, g1, dres, dx, dgb, 0, ws, wsf, rows, rpg, C, 1e-6, None)

    def plain(x=FAKE, dy=FAKE, dt=L.MMT_BF16, g0=FAKE, g1=None, dx=FAKE, dgb=FAKE, ws=FAKE, wsf=None, rows=40, rpg=0,
              C=256):
        wsf = (rows + 31) // 32 * 4 * C if wsf is None else wsf
        return L.LIB.mmt_layernorm_bwd(x, dy, dt, g0, g1, dx, dgb, 0, ws, wsf, rows, rpg, C, 1e-6, None)

    for f, aligned in ((add, ("x", "dy", "g0", "g1", "dx", "ws", "dres")), (plain, ("x", "dy", "g0", "g1", "dx", "ws"))):
        for name in ("x", "dy", "g0", "dx", "dgb", "ws"):
            assert f(**{name: None}) == N.EBADARG, name
        assert f(rows=0) == N.EBADARG and f(rows=-5) == N.EBADARG
        for C in (0, 128, 257, 384, 1280, -512):
            assert f(C=C) == N.EBADARG, C
        assert f(g1=FAKE, rpg=0) == N.EBADARG and f(g1=FAKE, rpg=-1) == N.EBADARG
        for name in aligned:
            for d in (4, 8):
                extra = dict(rpg=4) if name == "g1" else {}
                assert f(**{name: FAKE + d}, **extra) == N.EBADARG, (name, d)
        for rows, C in ((1, 256), (32, 768), (33, 1024), (2048, 512)):
            need = (rows + 31) // 32 * 4 * C
            assert f(rows=rows, C=C, wsf=need - 1) == N.EBADARG and f(rows=rows, C=C, wsf=0) == N.EBADARG
        for dt in (L.MMT_F64, 4, -1):
            assert f(dt=dt) == N.EBADARG, dt


def test_groupnorm_rejects_bad_arguments_on_the_host():
    L = _lib()

    def fwd(x=FAKE, of=FAKE, ot=FAKE, g0=FAKE, b0=FAKE, n=2, ips=1, P=16, Ctot=64, groups=4, dtype=L.MMT_F32):
        return L.LIB.mmt_groupnorm(x, of, ot, g0, b0, FAKE, FAKE, n, ips, P, Ctot, groups, 1e-5, dtype, None)

    def bwd(x=FAKE, dy=FAKE, ga=FAKE, dx=FAKE, dgb=FAKE, ws=FAKE, wsf=None, n=2, P=16, Ctot=64, groups=4):
        wsf = n * 2 * Ctot if wsf is None else wsf
        return L.LIB.mmt_groupnorm_bwd(x, dy, ga, dx, dgb, 0, ws, wsf, n, P, Ctot, groups, 1e-5, None)

    for name in ("x", "g0", "b0"):
        assert fwd(**{name: None}) == N.EBADARG, name
    for name in ("x", "dy", "ga", "dx", "dgb", "ws"):
        assert bwd(**{name: None}) == N.EBADARG, name
    for f in (fwd, bwd):
        assert f(n=0) == N.EBADARG and f(n=-1) == N.EBADARG and f(P=0) == N.EBADARG and f(P=-4) == N.EBADARG
        assert f(groups=0) == N.EBADARG and f(groups=-2) == N.EBADARG
        assert f(Ctot=66, groups=4) == N.EBADARG                              # Ctot % groups
        assert f(Ctot=12, groups=2) == N.EBADARG and f(Ctot=64, groups=32) == N.EBADARG  # cg % 4
        assert f(P=1537, Ctot=16, groups=1) == N.EBADARG and f(P=6145, Ctot=4, groups=1) == N.EBADARG  # P * cg / 4 > 6144
        assert f(P=1, Ctot=516, groups=1) == N.EBADARG                        # cg > 512
    assert bwd(P=1, Ctot=260, groups=1) == N.EBADARG and bwd(P=1, Ctot=512, groups=1) == N.EBADARG  # 2 cg > 512
    assert bwd(wsf=2 * 2 * 64 - 1) == N.EBADARG and bwd(wsf=0) == N.EBADARG and bwd(n=3, wsf=2 * 2 * 64) == N.EBADARG
    for name in ("x", "dy", "ga", "dx"):
        for d in (4, 8):
            assert bwd(**{name: FAKE + d}) == N.EBADARG, (name, d)
    for dtype in (L.MMT_F64, 4, -1):
        assert fwd(dtype=dtype) == N.EBADARG, dtype


def test_staging_entry_points_reject_bad_arguments_on_the_host():
    L = _lib()

    def ac(x=FAKE, add=None, add_n=0, of=FAKE, ot=FAKE, n=64, dtype=L.MMT_BF16):
        return L.LIB.mmt_add_cast(x, add, add_n, of, ot, n, dtype, None)

    assert ac(x=None) == N.EBADARG and ac(n=0) == N.EBADARG and ac(n=-4) == N.EBADARG
    for n in (1, 2, 3, 62, 65):
        assert ac(n=n) == N.EBADARG, n
    for add_n in (0, -4, 2, 6, 63):
        assert ac(add=FAKE, add_n=add_n) == N.EBADARG, add_n
    for dtype in (L.MMT_F64, 4, -1):
        assert ac(dtype=dtype) == N.EBADARG, dtype

    def sr(x=FAKE, scale=FAKE, rows_per=1, out=FAKE, rows=4, cols=64, dtype=L.MMT_BF16):
        return L.LIB.mmt_scale_rows_cast(x, scale, rows_per, out, rows, cols, dtype, None)

    for name in ("x", "scale", "out"):
        assert sr(**{name: None}) == N.EBADARG, name
    assert sr(rows=0) == N.EBADARG and sr(rows=-1) == N.EBADARG and sr(cols=0) == N.EBADARG and sr(cols=-8) == N.EBADARG
    for cols in (4, 12, 63, 65):
        assert sr(cols=cols) == N.EBADARG, cols
    assert sr(rows_per=0) == N.EBADARG and sr(rows_per=-2) == N.EBADARG
    for name in ("x", "out"):
        for d in (2, 4, 8):
            assert sr(**{name: FAKE + d}) == N.EBADARG, (name, d)
    for dtype in (L.MMT_F32, L.MMT_F64, 4, -1):  # the 16-bit types only
        assert sr(dtype=dtype) == N.EBADARG, dtype

    def pi(t0=FAKE, t1=FAKE, o0=FAKE, o1=FAKE, s0=FAKE, s1=FAKE, out=FAKE, Bm=1, ht=32, hs=64, patch=16, dtype=L.MMT_BF16):
        return L.LIB.mmt_patch_im2col(t0, t1, o0, o1, s0, s1, out, Bm, ht, hs, patch, dtype, None)

    for name in ("t0", "o0", "s0", "out"):
        assert pi(**{name: None}) == N.EBADARG, name
    assert pi(Bm=0) == N.EBADARG and pi(Bm=-1) == N.EBADARG
    for missing in (("t1",), ("o1",), ("s1",), ("t1", "o1"), ("o1", "s1"), ("t1", "s1")):  # a mixed second modality
        assert pi(**{k: None for k in missing}) == N.EBADARG, missing
    for patch in (2, 6, 15, 18):
        assert pi(patch=patch, ht=2 * patch, hs=4 * patch) == N.EBADARG, patch
    assert pi(ht=40) == N.EBADARG and pi(hs=72) == N.EBADARG and pi(ht=8, hs=64) == N.EBADARG
    for dtype in (L.MMT_F64, 4, -1):
        assert pi(dtype=dtype) == N.EBADARG, dtype
        assert pi(t1=None, o1=None, s1=None, dtype=dtype) == N.EBADARG, dtype
