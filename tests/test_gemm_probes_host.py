"""The GEMM probes themselves (tests/gemm_probes.py), on the CPU: the shape lists sit on the tile edges they
claim, every listed case reaches the kernel it names with the split it asks for, the integer reference is
exact in every arithmetic the kernels use, and a dropped, doubled or misplaced product changes the outputs."""
import hashlib
import os
import re

import pytest
import torch

import gemm_probes as P
from conftest import ROOT

CASES = P.all_cases()
MUT_SHAPES = [(129, 136, 72), (65, 72, 584), (257, 264, 4096)]


def test_tile_table_matches_the_library_sources():
    """TILES against the `impl` comment of include/mmt_hip.h (tile shapes, K split) and, for the ring depth the
    header does not state, against the launch switch of gemm_glds.hip (source text only; nothing is loaded)."""
    text = open(os.path.join(ROOT, "include", "mmt_hip.h")).read()
    doc = text[text.index("int32_t impl;"):text.index("int32_t ln_fold;")]
    doc = re.sub(r"\s*\n\s*", " ", doc)
    seen = {int(i): (int(bm), int(bn)) for i, bm, bn in re.findall(r"(?<![\dx])([1-8]) (\d+)x(\d+)", doc)}
    assert seen == {i: t[:2] for i, t in P.TILES.items()}, seen
    for i, ks in re.findall(r"(?<![\dx])([1-8]) \d+x\d+ \(K split(?: over)? (\d)", doc):
        assert P.TILES[int(i)][2] == int(ks)
    assert {i for i, t in P.TILES.items() if t[2] == 2} == {int(i) for i, _ in re.findall(
        r"(?<![\dx])([1-8]) \d+x\d+ \(K split(?: over)? (\d)", doc)}
    src = open(os.path.join(ROOT, "multi-modal-tracking_amd", "csrc", "gemm_glds.hip")).read()
    sw = {int(i): tuple(int(v) for v in (bm, bn, ks, st)) for i, bm, bn, ks, st in re.findall(
        r"case (\d): launch<T, (\d+), (\d+), \d+, \d+, (\d+), (\d+)>\(p, nsk, st\)", src)}
    sw[7] = tuple(int(v) for v in re.search(r"gemm_glds_kernel<T, (256), (256), \d, \d, (\d), (\d), false, 0>\)", src).groups())
    sw[8] = tuple(int(v) for v in re.search(r"gemm_glds_kernel_occ2<T, (128), (128), \d, \d, (\d), (\d)>\)", src).groups())
    assert sw == P.TILES, sw
    reg = open(os.path.join(ROOT, "multi-modal-tracking_amd", "csrc", "gemm.hip")).read()
    assert "DEPTH = 3" in reg and "nk64 >= %d" % P.REG_KG2_STEPS in reg and "blocks(128, 128) >= %d" % P.REG_BIG_TILES in reg


@pytest.mark.parametrize("dname,impl", P.SWEEP)
def test_edge_shapes_cover_the_tile_edges(dname, impl):
    bm, bn, ks, st = P.tile_of(impl, dname)
    S, c = P.kstep(dname), 16 // P.esize(dname)
    shapes = P.edge_shapes(impl, dname)
    assert {0, 1, bm - 1} <= {m % bm for m, _, _ in shapes}
    assert {0, 8, bn - 8} <= {n % bn for _, n, _ in shapes}  # (the LDS-DMA kernels take N % 8 == 0 only)
    assert {0, c, S - c} <= {k % S for _, _, k in shapes}
    steps = {(k + S - 1) // S for _, _, k in shapes}
    slots = ks * st
    assert min(steps) < slots and slots in steps and max(steps) > 2 * slots
    if ks == 2:
        assert any(n % 2 and n > 2 for n in steps)
    if impl == -1 or dname == "f32":  # both sides of the second k-group's threshold, an odd count above it, N % 8 != 0
        assert {P.REG_KG2_STEPS - 1, P.REG_KG2_STEPS, P.REG_KG2_STEPS + 1} <= steps
        assert {1, 63, 65} <= {n for _, n, _ in shapes} and {1, bn - 1} <= {n % bn for _, n, _ in shapes}
    # the sweep lists: all three epilogue code paths on every LDS-DMA tile
    if dname != "f32" and impl != -1:
        paths = {P.epilogue_path(s) for e in P.EPILOGUES for s in P.sweep_cases(dname, impl, e)}
        assert paths == ({0} if impl == 7 else {0, 1, 2})  # (impl 7 is compiled with the general epilogue alone)
        assert all(len(P.sweep_cases(dname, impl, e)) >= 30 for e in P.EPILOGUES)
        assert any(s.stats for s in P.sweep_cases(dname, impl, "residual_stats"))
    else:
        assert all(len(P.sweep_cases(dname, impl, e)) >= 100 for e in ("general", "compact", "c2_sum_rt_mod"))


def test_split_lists_cover_the_slice_edges():
    for impl in P.SPLIT_IMPLS:
        ks = P.TILES[impl][2]
        for nsk in range(2, 9):
            cs = P.split_cases(impl, nsk)
            nks = [(s.K + 63) // 64 for s in cs if not s.conv]
            assert nsk * ks in nks and nsk * ks + 1 in nks           # every slice at its minimum; uneven slices
            assert any(n > 3 and all(n % q for q in range(2, n)) for n in nks)
            assert any(s.K % 64 == 8 for s in cs)
            assert all(s.groups == 2 and s.r_inplace and s.c2_copy == 1 for s in cs if not s.conv)
        assert any(s.conv and s.K == 216 for nsk in range(2, 9) for s in P.split_cases(impl, nsk))


def test_big_grids_and_remap_remainders():
    for impl in P.BIG_IMPLS:
        cs = P.big_cases(impl)
        grids = [P.grid_of(s) for s in cs]
        assert all(wg > 512 and tm > 8 for wg, tm in grids), grids
        assert {0, 1, 4} <= {tm % 8 for _, tm in grids}
        assert {64, 72} <= {s.K for s in cs}
        kern = {P.kernel_of(s)[1] for s in cs}
        assert kern == {8 if impl == 0 else impl}, kern          # auto: the two-per-CU tile's row-group order
        for s in cs:
            assert (s.M + 8) * (s.N + 8) * 2 <= 72 << 20
        if impl in (5, 6):
            assert any(P.split_used(impl, s) == 2 for s in cs)
    rem = {P.grid_of(s)[0] % 8 for _, _, s in CASES}
    assert {0, 1, 7} <= rem, rem


def test_every_case_reaches_the_kernel_it_names():
    assert len(CASES) > 5000
    for kind, impl, s in CASES:
        assert P.takes(impl, s), (kind, impl, s, P.kernel_of(s))
        if s.splitk >= 2:
            assert P.split_used(impl, s) == s.splitk, (kind, impl, s, P.kernel_of(s))
        else:
            assert P.split_used(impl, s) == 1, (kind, impl, s)
        assert 9 * s.K + 72 < 2 ** 24
    kinds = {(k, i) for k, i, _ in CASES}
    for k, impls in (("split", P.SPLIT_IMPLS), ("rowmap", P.ROWMAP_IMPLS), ("mn", P.MN_IMPLS), ("conv", P.CONV_IMPLS),
                     ("big", P.BIG_IMPLS), ("rowscale", P.ROWSCALE_IMPLS), ("ln", P.LN_IMPLS[2])):
        assert {(k, i) for i in impls} <= kinds, k
    for mode in ("gemm", "conv"):
        for impl in (0, 1, 3):
            for n in (1, 2, 3, 4):
                specs = P.multi_cases(mode, impl, n)
                assert len(specs) == n and P.multi_one_launch(specs)
                assert len({(s.M, s.N, s.K) for s in specs}) == n


def test_selection_reproduces_the_recorded_answers():
    """mmt_gemm_select against tests/golden/gemm_select_cases.txt, recorded from an independent restatement of the
    dispatch: family, tile configuration, K slices and epilogue code of every case, mmt_gemm_multi's joint launches,
    and the case list itself (no case may leave or change unnoticed)."""
    lines = [ln for ln in open(os.path.join(ROOT, "tests", "golden", "gemm_select_cases.txt")).read().split("\n")
             if ln and not ln.startswith("#")]
    sha = hashlib.sha256("".join(repr(s) for _, _, s in CASES).encode()).hexdigest()
    assert lines[0] == "cases %d sha256 %s" % (len(CASES), sha)

    def token(s):
        k = P.kernel_of(s)
        if k is None or k[0] == "gemv":
            return "x" if k is None else "v"
        return "r%d.%d" % k[1:] if k[0] == "reg" else "g%d.%d.%d" % (k[1], k[2], P.epilogue_path(s))
    wrong = [(i, s, want, token(s)) for i, ((_, _, s), want) in enumerate(zip(CASES, lines[1:])) if token(s) != want]
    assert not wrong, (len(wrong), wrong[:3])
    multi = ["multi %s %d %d %d" % (mode, impl, n, P.multi_one_launch(P.multi_cases(mode, impl, n)))
             for mode in ("gemm", "conv") for impl in (1, 3, 0) for n in (1, 2, 3, 4)]
    assert multi == lines[1 + len(CASES):]


def test_predicates_mirror_the_silent_fallbacks():
    """What the dispatcher declines: the predicates must say so, or a probe would test another kernel."""
    s = P.Spec(129, 136, 512, impl=7, splitk=2, c_f32=1)
    assert P.kernel_of(s)[0] == "reg" and not P.takes(7, s)          # impl 7 / 8: no split-K
    assert P.takes(8, s.but(impl=8)) and P.split_used(8, s.but(impl=8)) == 1  # (impl 8 drops the split instead)
    assert P.split_used(1, s.but(impl=1, K=64, splitk=5)) == 1       # one K-step: nothing to split
    assert P.split_used(3, s.but(impl=3, K=512, splitk=5)) == 4      # nsk * KS <= nk
    assert P.split_used(1, s.but(impl=1, splitk=8, ws_floats=1 << 16)) == 1  # workspace too small
    conv = P.Spec(128, 40, 216, impl=7, conv=(8, 1, 24, 1, 0))
    assert P.kernel_of(conv)[0] == "reg" and P.takes(5, conv.but(impl=5))
    assert P.kernel_of(P.Spec(64, 65, 64, impl=1))[0] == "reg"       # N % 8 != 0
    assert P.kernel_of(P.Spec(64, 64, 64, impl=-1, c2=True, c2_copy=2)) is None
    assert P.kernel_of(P.Spec(64, 64, 64, impl=2, w_t=1)) is None    # MN-major: impl 0 / 1 / 8 only
    assert P.kernel_of(P.Spec(64, 64, 64, impl=1, row_scale_div=3, r=1)) is None
    assert P.kernel_of(P.Spec(8, 64, 64, dtype="f32", groups=1, c_f32=1)) == ("gemv",)
    assert not P.takes(7, P.Spec(64, 64, 128, impl=7, c_f32=1, ln_fold=2)) and P.takes(8, P.Spec(64, 64, 128, impl=8, c_f32=1, ln_fold=2))
    assert not P.takes(8, P.Spec(64, 64, 128, impl=8, c_f32=1, ln_fold=1))


@pytest.mark.parametrize("M,N,K", MUT_SHAPES)
def test_reference_is_exact_in_every_arithmetic(M, N, K):
    A, W, bias, acc = P.operands(M, N, K, 2, 0)
    assert acc.dtype == torch.int64
    assert int(A.abs().min()) >= 1 and int(W.abs().min()) >= 1 and int(A.abs().max()) <= 3 and int(W.abs().max()) <= 3
    assert torch.equal(torch.einsum("gmk,gnk->gmn", A.double(), W.double()).to(torch.int64), acc)
    f32 = torch.einsum("gmk,gnk->gmn", A.float(), W.float())
    assert torch.equal(f32.to(torch.int64), acc) and torch.equal(f32, acc.float())
    rev = torch.einsum("gmk,gnk->gmn", A.float().flip(-1), W.float().flip(-1))  # another summation order
    assert torch.equal(rev, f32)
    # the largest partial sum in any order is below sum |a w| + |bias| + |R| < 2^24
    bound = torch.einsum("gmk,gnk->gmn", A.abs(), W.abs()).max().item() + 8 + 64
    assert bound <= 9 * K + 72 < 2 ** 24
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        for t in (A, W, bias):
            assert torch.equal(t.to(dt).to(torch.int64), t)


@pytest.mark.parametrize("M,N,K", MUT_SHAPES)
def test_probes_discriminate(M, N, K):
    """Mutated references (what a subtly wrong kernel would compute) against the true one."""
    A, W, _, acc = P.operands(M, N, K, 1, 0)
    A, W, acc = A[0], W[0], acc[0]

    def changed(mut, region=None):
        d = mut != acc
        return (d[region] if region is not None else d).float().mean().item()
    for k in (0, K // 2 + 3, K - 1):
        prod = A[:, k, None] * W[None, :, k]
        assert changed(acc - prod) == 1.0 and changed(acc + prod) == 1.0      # one k dropped / counted twice
    for c in (0, (K // 8) // 2, K // 8 - 1):                                   # one 8-chunk dropped
        part = A[:, 8 * c:8 * c + 8] @ W[:, 8 * c:8 * c + 8].t()
        assert changed(acc - part) == 1.0
    full = lambda a, w: a @ w.t()
    assert changed(full(A.roll(1, 0), W)) >= 0.8                               # rows shifted by one
    assert changed(full(A, W.roll(1, 0))) >= 0.8                               # columns shifted by one
    if M > 128:                                                                # a tile's rows swapped with the next tile's
        idx = torch.arange(M)
        n = min(64, M - 64)
        idx[:n], idx[64:64 + n] = torch.arange(64, 64 + n), torch.arange(n)
        moved = idx != torch.arange(M)
        assert changed(full(A[idx], W), moved) >= 0.8
    # K clipped to the last whole 64-step, and a K tail read past K as if the pitch columns were data
    if K % 64:
        assert changed(full(A[:, :K // 64 * 64], W[:, :K // 64 * 64])) == 1.0


def test_sixteen_bit_expectations_round_once():
    """At K = 4096 part of the reference values is not representable in bf16 (the rounding is exercised); at
    K <= 72 all are exact."""
    _, _, bias, big = P.operands(257, 264, 4096, 2, 0)
    big = big + bias[:, None, :]  # (acc alone is even: an even number of odd chunk sums)
    _, _, bias, small = P.operands(129, 136, 72, 2, 0)
    small = small + bias[:, None, :]
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(small.float().to(dt).to(torch.int64), small)
    inexact = (big.float().bfloat16().to(torch.int64) != big).float().mean().item()
    assert 0.05 <= inexact <= 0.5, inexact
    assert int(big.abs().max()) < 65504  # finite in fp16
    # one rounding, to nearest even: never further than half a bf16 ulp (ulp <= 2^-7 |v|)
    err = (big.float().bfloat16().double() - big.double()).abs()
    assert bool((err <= big.double().abs() * 2.0 ** -8).all())


def test_storage_is_poisoned_and_compared_whole():
    s = P.Spec(65, 72, 136, impl=3, c_f32=1, r=1, act=2, a_seg=(7, 3), k_split=72, c_seg=(63, 66))
    pr = P.build(s)
    geo = pr.geo
    a = pr.inp["a"][0]
    assert a.shape[1] == 72 + 8 and torch.isnan(a[:, 72:]).all() and torch.isnan(a[-8:]).all()
    rows = P.a_phys_rows(s, geo)
    assert not torch.isnan(a[rows, :72]).any() and int((~torch.isnan(a[:, 0])).sum()) == s.M
    a1 = pr.inp["a1"][0]
    assert not torch.isnan(a1[rows, :64]).any() and torch.isnan(a1[rows, 64:]).all()
    w = pr.inp["w"][0]
    assert w.shape == (72 + 8, 136) and torch.isnan(w[72:]).all() and not torch.isnan(w[:72]).any()
    assert torch.isnan(pr.inp["bias"][0][72:]).all() and torch.isnan(pr.inp["r"][0][:, 72:]).all()
    assert torch.isnan(pr.inp["r"][0][-8:]).all()
    c, e = pr.out["c"][0], pr.expect["c"][0]
    assert torch.isnan(c).all() and c.shape[1] == 72 + 8
    crow = P.c_phys_rows(s)
    assert int((~torch.isnan(e)).sum()) == s.M * s.N and not torch.isnan(e[crow, :72]).any()
    assert torch.isnan(e[63:66]).all() and torch.isnan(e[-8:]).all()
    assert P.same(e, e) and not P.same(c, e)
    hit = e.clone()
    hit[64, 3] = 1.0                      # a pitch row written
    assert not P.same(hit, e) and "1 guard" in P.describe(hit, e)
    miss = e.clone()
    miss[0, 0] = P.NAN                    # an element never written (or a NaN read into it)
    assert not P.same(miss, e) and "1 NaN" in P.describe(miss, e)
    off = e.clone()
    off[5, 5] += 1
    assert not P.same(off, e) and "1 wrong" in P.describe(off, e)
    # MN-major storage and the column split
    t = P.build(P.Spec(120, 136, 200, impl=1, groups=1, c_f32=1, a_t=1, w_t=2, c2=True, c2_copy=3, bias=False))
    assert t.inp["a"][0].shape == (208, 128) and torch.isnan(t.inp["a"][0][200:]).all() and torch.isnan(t.inp["a"][0][:, 120:]).all()
    assert torch.isnan(t.inp["w"][0][:, 128:]).all() and not torch.isnan(t.inp["w"][0][:200, :128]).any()
    e2 = t.expect["c2"][0][:120 * 8].view(120, 8)
    assert torch.equal(e2[:, 1:], torch.zeros(120, 7)) and torch.equal(e2[:, 0].to(torch.int64), t.inp["a"][0][:200, :120].sum(0).to(torch.int64))


def test_folded_layernorm_probe_is_exact_up_to_the_statistics():
    pr = P.build_ln(P.Spec(65, 72, 128, impl=3, c_f32=1, ln_fold=2))
    a = pr.inp["a"][0][:65, :128].double()
    assert torch.equal(a.mean(1), torch.full((65,), 2.0, dtype=torch.float64))
    assert torch.equal((a * a).mean(1) - 4.0, torch.ones(65, dtype=torch.float64))
    st = pr.inp["stats_in"][0][:65].view(65, 2, 2)
    assert torch.equal(st[:, :, 0].sum(1), torch.full((65,), 256.0)) and torch.equal(st[:, :, 1].sum(1), torch.full((65,), 640.0))
    ref = torch.nn.functional.layer_norm(a, (128,), eps=P.LN_EPS) @ pr.inp["w"][0][:72].double().t() + pr.inp["bias"][0][:72].double()
    assert (ref - pr.expect["c"][0][:65, :72]).abs().max().item() <= 1e-9 * ref.abs().max().item()
