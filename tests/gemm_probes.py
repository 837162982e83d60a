"""Probe inputs, exact integer references and dispatch predicates of the GEMM tests (no tests here).

Operands.  A and W hold integers from {-3, -2, -1, 1, 2, 3} (never 0: each of the M*N*K products is nonzero,
so an output element changes when one product of its row is dropped or counted twice), bias integers in
[-8, 8], R integers in [-64, 64], row_scale values in {0, 1, 2}: all exact in bf16, fp16 and fp32.

Reference.  An int64 matmul plus an integer epilogue.  With K <= 4096 every partial sum stays below
9 * 4096 + 72 < 2^24, so the kernels' fp32 accumulation is exact in any summation order, tile shape or
split; the expected 16-bit outputs are ref.float().to(dtype), one round-to-nearest-even of an exact value,
which is what from_f<T> does.  Only the exact activations: 0 and 2 (ReLU).  (Above 2^28 products the matmul
runs as a float64 BLAS matmul, which test_gemm_probes_host.py shows bitwise equal: sums < 2^24 << 2^53.)

Poisoned storage.  Every buffer is larger than the problem and the surplus is NaN: A with lda = K + 8 and 8
rows past the last row a segment map can address, W with 8 rows past N (W^T: ldw = N + 8 and 8 rows past K),
bias / R with 8 extra elements / rows, C and C2 with ldc = N + 8 and 8 rows past M, pre-filled with NaN.  The
kernels clamp rows to M - 1 / N - 1 and zero-fill chunks past K, so the surplus is never part of the
contract; it lies inside the allocation (an over-read faults nothing) and turns the result into NaN.
`expected buffers` are whole storage images -- the reference inside the M x N region, NaN everywhere else --
and same() compares all of it: every element written with the right value, no guard element touched, no
NaN read into the region.

TILES is the geometry of the launch switch of gemm_glds.hip (BM, BN, k-groups KS, ring slots ST; K-step 64);
the register-staged kernel (impl -1 and all fp32) runs 64x64 tiles with one k-group below 8 K-steps and
two from 8 on, 128x128 tiles from 512 of them up, behind a ring of 3 register stages; its K-step is 64
(16-bit) or 32 (fp32) elements.

kernel_of() / takes() / split_used() / grid_of() / epilogue_path() read the library's own answer (mmt_gemm_select on
params_of(spec), no GPU needed), so a probe that wants impl 7 or five slices proves that it gets them.
"""
import dataclasses
import functools
import math

import torch
import torch.nn.functional as F

NAN = float("nan")
PAD = 8
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
# impl: (BM, BN, KS, ST)
TILES = {1: (128, 128, 1, 4), 2: (128, 64, 2, 3), 3: (64, 64, 2, 4), 4: (128, 128, 1, 4), 5: (256, 128, 1, 3),
         6: (128, 256, 1, 3), 7: (256, 256, 1, 2), 8: (128, 128, 1, 2)}
REG_TILE = (64, 64, 2, 3)  # register-staged: 64x64, up to two k-groups, 3 register stages
REG_KG2_STEPS = 8          # K-steps from which it runs two k-groups
REG_BIG_TILES = 512        # 128x128 tiles (x groups) from which it runs 128x128
GLDS_IMPLS = (1, 2, 3, 4, 5, 6, 7, 8)
WS_FLOATS, CNT_N = 8 << 20, 1 << 16  # the split-K workspace the tests hand in unless a case says otherwise


@dataclasses.dataclass(frozen=True)
class Spec:
    """One launch.  M, N, K are the logical sizes (conv: M = B * h * h, K = taps * cin)."""
    M: int
    N: int
    K: int
    impl: int = 0
    dtype: str = "bf16"
    groups: int = 2
    act: int = 0
    c_f32: int = 0
    bias: bool = True
    r: int = 0              # 0 none, 1 fp32, 2 in the compute dtype (r_t)
    r_inplace: bool = False  # C is R's buffer (the residual stream's X += ...)
    r_mode: int = 0
    r_p0: int = 0
    r_p1: int = 1
    c2: bool = False
    c2_copy: int = 0
    stats: bool = False     # ln_stats_out
    a_seg: tuple = None     # (a_seg_rows, a_segs_a)
    k_split: int = 0
    c_seg: tuple = None     # (c_seg_rows, c_seg_pitch)
    conv: tuple = None      # (conv_h, conv_up, conv_cin, conv_k3, 1: an image pitch larger than the map)
    a_t: int = 0
    w_t: int = 0
    splitk: int = 0
    ws_floats: int = WS_FLOATS
    cnt_n: int = CNT_N
    row_scale_div: int = 0
    ln_fold: int = 0
    seed: int = 0

    def but(self, **kw):
        return dataclasses.replace(self, **kw)


def esize(dname):
    return 4 if dname == "f32" else 2


def kstep(dname):
    return 32 if dname == "f32" else 64


def tile_of(impl, dname="bf16"):
    """(BM, BN, KS, ST) the edge shapes of `impl` are derived from (auto: the 64x64 tile it picks at these sizes)."""
    if dname == "f32" or impl == -1:
        return REG_TILE
    return TILES[3] if impl == 0 else TILES[impl]


# ------------------------------------------------------------------------------------------------ storage geometry
def geometry(s):
    """Strides of the poisoned storage of a spec (elements): what the launch passes."""
    g = {"ldc": s.N + PAD, "ldr": s.N + PAD, "ldw": s.N + PAD if s.w_t else 0}
    if s.c2_copy in (3, 4):
        g["ldc"] = s.N - 8 + PAD
    if s.r_inplace:
        g["ldr"] = g["ldc"]
    if s.conv:
        h, up, cin, k3, extra = s.conv
        hi = h // up
        g["lda"] = cin + PAD
        g["img_pitch"] = (hi * hi + 7) // 8 * 8 + 8 if extra else hi * hi  # (a_stride_a % 8 == 0)
        g["seg"] = (s.M, 1, g["img_pitch"] if extra else 0, 0)
        g["a_rows"] = (s.M // (h * h)) * g["img_pitch"]
    elif s.a_t:
        g["lda"] = s.M + PAD
        g["seg"] = (s.M, 1, 0, 0)
        g["a_rows"] = s.K
    else:
        kmax = max(s.k_split, s.K - s.k_split) if s.k_split else s.K
        g["lda"] = kmax + PAD
        if s.a_seg:
            sr, sa = s.a_seg
            g["blk_rows"] = sa * (sr + 1) + 3  # segments one NaN row apart, blocks three more
            g["seg"] = (sr, sa, (sr + 1) * g["lda"], g["blk_rows"] * g["lda"])
            g["a_rows"] = a_phys_rows(s, g)[-1].item() + 1
        else:
            g["seg"] = (s.M, 1, 0, 0)
            g["a_rows"] = s.M
    g["c_rows"] = c_phys_rows(s)[-1].item() + 1
    return g


def a_phys_rows(s, g):
    """Storage row of every logical A row (GEMM mode)."""
    m = torch.arange(s.M)
    if not s.a_seg:
        return m
    sr, sa = s.a_seg
    seg = m // sr
    return (seg % sa) * (sr + 1) + (seg // sa) * g["blk_rows"] + m % sr


def c_phys_rows(s):
    m = torch.arange(s.M)
    if not s.c_seg:
        return m
    rows, pitch = s.c_seg
    return (m // rows) * pitch + m % rows


def r_phys_rows(s):
    """Storage row of R that output row m reads."""
    m = torch.arange(s.M)
    if s.r_mode == 1:
        return m % s.r_p0
    if s.r_mode == 2:
        hw = s.r_p0 * s.r_p0
        b, rem = m // hw, m % hw
        y, x, hs = rem // s.r_p0, rem % s.r_p0, s.r_p0 // s.r_p1
        return b * hs * hs + (y // s.r_p1) * hs + x // s.r_p1
    return c_phys_rows(s)


# ------------------------------------------------------------------------------------------------ dispatch (the library's)
def _lib():
    from mmt_amd import _lib
    return _lib


def dtype_code(dname):
    L = _lib()
    return {"f32": L.MMT_F32, "bf16": L.MMT_BF16, "fp16": L.MMT_F16}[dname]


_FAKE = 1 << 20  # stands for every buffer when the library is only asked: non-null, 16-B aligned, never dereferenced


def params_of(s, ptrs=None):
    """mmt_gemm_params of a spec.  ptrs: name -> device addresses (per group: a, w, c, bias, r, c2, a1, stats, colsum,
    stats_in; row_scale; sk = (slabs, tickets)); without it every buffer the spec has is a fake address, which is
    all the selection looks at.  The split-K workspace is handed in with a forced split only."""
    L, geo = _lib(), geometry(s)
    at = (lambda name, q: _FAKE) if ptrs is None else (lambda name, q: ptrs[name][q])
    p = L.GemmParams()
    for q in range(s.groups):
        p.a[q], p.w[q], p.c[q] = at("a", q), at("w", q), at("c", q)
        p.bias[q] = at("bias", q) if s.bias else None
        p.r[q] = at("r", q) if s.r else None
        p.c2[q] = at("c2", q) if s.c2 else None
        p.a1[q] = at("a1", q) if s.k_split else None
        p.ln_stats_out[q] = at("stats", q) if s.stats else None
        p.ln_colsum[q] = at("colsum", q) if s.ln_fold else None
        p.ln_stats_in[q] = at("stats_in", q) if s.ln_fold == 2 else None
    p.lda, p.ldc, p.ldr = geo["lda"], geo["ldc"], geo["ldr"]
    p.a_seg_rows, p.a_segs_a, p.a_stride_a, p.a_stride_b = geo["seg"]
    p.M, p.N, p.K, p.k_split = s.M, s.N, s.K, s.k_split
    p.act, p.c_f32, p.c2_copy, p.groups, p.impl = s.act, s.c_f32, s.c2_copy, s.groups, s.impl
    p.r_mode, p.r_p0, p.r_p1, p.r_t = s.r_mode, s.r_p0, s.r_p1, int(s.r == 2)
    if s.conv:
        p.conv_h, p.conv_up, p.conv_cin, p.conv_k3 = s.conv[:4]
    if s.splitk:
        p.splitk, p.sk_ws_floats, p.sk_cnt_n = s.splitk, s.ws_floats, s.cnt_n
        p.sk_ws, p.sk_cnt = at("sk", 0), at("sk", 1)
    if s.c_seg:
        p.c_seg_rows, p.c_seg_pitch = s.c_seg
    p.a_t, p.w_t, p.ldw = s.a_t, s.w_t, geo["ldw"]
    if s.row_scale_div:
        p.row_scale, p.row_scale_div = at("row_scale", 0), s.row_scale_div
    if s.ln_fold:
        p.ln_fold, p.ln_eps = s.ln_fold, LN_EPS
    return p


@functools.lru_cache(maxsize=None)
def select(s):
    """mmt_gemm_select's answer for a spec (a GemmChoice), None when mmt_gemm rejects it."""
    return _lib().gemm_select(params_of(s), dtype_code(s.dtype))


def kernel_of(s):
    """The kernel a launch ends up in: ("glds", tile configuration, K slices), ("reg", BM, k-groups),
    ("gemv",) or None when mmt_gemm rejects it."""
    c, L = select(s), _lib()
    if c is None:
        return None
    if c.family == L.GEMM_GEMV:
        return ("gemv",)
    return ("glds", c.cfg, c.nsk) if c.family == L.GEMM_LDS_DMA else ("reg", c.bm, c.kgroups)


def epilogue_path(s):
    """Which epilogue code of the LDS-DMA kernels a spec runs: 0 general, 1 compact 16-bit, 2 residual producer."""
    return select(s).epi


def takes(impl, s):
    """The kernel family `impl` names runs spec s (s.impl == impl): -1 / fp32 the register-staged tiles, 1..8 that
    LDS-DMA tile, 0 any tiled kernel."""
    k = kernel_of(s)
    if k is None or k[0] == "gemv" or s.impl != impl:
        return False
    if impl == -1 or s.dtype == "f32":
        return k[0] == "reg"
    return k[0] in ("glds", "reg") if impl == 0 else k[:2] == ("glds", impl)


def split_used(impl, s):
    """K slices the launch runs with (1: no split)."""
    k = kernel_of(s)
    return k[2] if k and k[0] == "glds" and s.impl == impl else 1


def grid_of(s):
    """(workgroups, tiles_m) of the launch."""
    c = select(s)
    return c.wgs, (s.M + c.bm - 1) // c.bm


# ------------------------------------------------------------------------------------------------ shape lists
def edge_mnk(impl, dname="bf16"):
    bm, bn, ks, st = tile_of(impl, dname)
    reg = impl == -1 or dname == "f32"
    S, c, d = kstep(dname), 16 // esize(dname), ks * st
    Ms = [1, 8, bm - 1, bm, bm + 1, bm + bm // 2 + 3]
    Ns = [8, bn - 8, bn, bn + 8, bn + bn // 2 + 8] + ([1, 63, 65] if reg else [])
    Ks = [c, S - c, S, S + c, S * d - c, S * d, S * d + c, S * (d + 1) + c, S * (2 * d + 1)]
    if reg:  # both sides of the step count at which the second k-group starts, and an odd count under it
        Ks += [S * (REG_KG2_STEPS - 1), S * REG_KG2_STEPS, S * (REG_KG2_STEPS + 1)]
    return Ms, Ns, sorted(set(Ks))


def edge_shapes(impl, dname="bf16"):
    """(M, N, K) on the tile's edges: every (M, N) pair at two K, every K at two (M, N) pairs."""
    bm, bn, ks, st = tile_of(impl, dname)
    Ms, Ns, Ks = edge_mnk(impl, dname)
    S, c, d = kstep(dname), 16 // esize(dname), ks * st
    out = [(m, n, k) for k in (S + c, S * (d + 1) + c) for m in Ms for n in Ns]
    out += [(m, n, k) for (m, n) in ((bm + 1, bn + 8), (bm - 1, bn - 8)) for k in Ks]
    return sorted(set(out))


EPILOGUES = {
    "general": dict(act=2, r=1, c_f32=1),                       # bias + ReLU + fp32 R into an fp32 C
    "compact": dict(act=2),                                     # 16-bit C, bias, ReLU
    "compact_pre": dict(act=2, c2=True, c2_copy=2),             # ... with C2 the pre-activation
    "residual": dict(r=1, c_f32=1, c2=True, c2_copy=1),         # fp32 C = acc + bias + R, C2 its 16-bit copy
    "residual_stats": dict(r=1, c_f32=1, c2=True, c2_copy=1, stats=True),
    "c2_sum_rt_mod": dict(r=2, c2=True, r_mode=1, r_p0=5),      # 16-bit C, C2 = C + R, R in dtype at row m % 5
}
SWEEP = [(d, i) for d in ("bf16", "fp16") for i in (-1, 1, 2, 3, 4, 5, 6, 7, 8, 0)] + [("f32", 0)]


def sweep_cases(dname, impl, epi):
    """The plain sweep of one (dtype, impl, epilogue): specs the named kernel takes (possibly none)."""
    kw = EPILOGUES[epi]
    if epi == "residual_stats":  # N % 64 == 0 and |C2| <= 9 * 16 + 8 + 64 <= 256: exact sums of squares
        bm, bn = tile_of(impl, dname)[:2]
        shapes = [(m, n, k) for m in edge_mnk(impl, dname)[0] for n in (64, bn, bn + 64) for k in (8, 16)]
    else:
        shapes = edge_shapes(impl, dname)
    cases = [Spec(m, n, k, impl=impl, dtype=dname, **kw) for m, n, k in shapes]
    if epi in ("general", "compact"):  # one group: grids of 7, 9, 15 and 17 workgroups (the XCD remap's remainders)
        bm, bn = tile_of(impl, dname)[:2]
        k = kstep(dname) + 16 // esize(dname)
        cases += [Spec(tm * bm - 1, tn * bn - 8, k, impl=impl, dtype=dname, groups=1, **kw)
                  for tm, tn in ((7, 1), (3, 3), (5, 3), (17, 1))]
    return [s for s in cases if takes(impl, s)]


SPLIT_IMPLS = (1, 2, 3, 4, 6)


def split_cases(impl, nsk):
    """K with exactly nsk * KS steps, one more, a prime count, and a one-chunk K tail on the last slice; the conv
    mode once (K = 9 * 24 = 216: four steps, the last one zero-filled from 24 on)."""
    bm, bn, ks, _ = TILES[impl]
    lo = nsk * ks
    prime = next(p for p in (5, 7, 11, 13, 17, 19, 23) if p > lo)
    base = Spec(bm + 1, bn + 8, 0, impl=impl, splitk=nsk, c_f32=1, r=1, r_inplace=True, c2=True, c2_copy=1)
    out = [base.but(K=64 * lo), base.but(K=64 * (lo + 1)), base.but(K=64 * prime), base.but(K=64 * lo + 8),
           base.but(M=bm - 1, N=bn - 8, K=64 * (lo + 1) + 8)]
    if nsk * ks <= 4:
        out.append(Spec((bm // 64 + 1) * 64, bn + 8, 216, impl=impl, splitk=nsk, c_f32=1, act=2, conv=(8, 1, 24, 1, 0)))
    return out


ROWMAP_IMPLS = (0, 1, 3, 8, -1)


def rowmap_cases(impl):
    bm, bn = tile_of(impl)[:2]
    M, N, K = bm + bm // 2 + 3, bn + 8, 136
    out = []
    for sr in (1, 7, bm + 1):
        out.append(Spec(M, N, K, impl=impl, c_f32=1, a_seg=(sr, 3)))
        for ks in (8, 72, K - 8):
            out.append(Spec(M, N, K, impl=impl, c_f32=1, a_seg=(sr, 3), k_split=ks))
    for ks in (8, 72, K - 8):
        out.append(Spec(M, N, K, impl=impl, k_split=ks))
    for cr in (1, bm - 1, bm + 1):
        out.append(Spec(M, N, K, impl=impl, c_f32=1, r=1, c_seg=(cr, cr + 3)))
        out.append(Spec(M, N, K, impl=impl, r=2, c2=True, c_seg=(cr, cr + 3)))
    for p0 in (1, 5, M):
        out.append(Spec(M, N, K, impl=impl, c_f32=1, r=1, r_mode=1, r_p0=p0, act=2))
    for p1 in (1, 2):  # 1x1 conv over B maps of 8 x 8, R at the (8 / p1)^2 resolution
        out.append(Spec(3 * 64, N, 72, impl=impl, c_f32=1, r=1, r_mode=2, r_p0=8, r_p1=p1, conv=(8, 1, 72, 0, 0)))
    return [s for s in out if takes(impl, s)]


MN_IMPLS = (0, 1, 8)
MN_SIZES = (8, 120, 128, 136)
MN_KS = (8, 56, 64, 72, 200, 264)


def mn_cases(impl, splitk):
    """MN-major operands; with a split, only the K that hold it (splitk slices of >= 1 step)."""
    out = []
    pairs = [(m, n) for m in MN_SIZES for n in MN_SIZES]
    for K in MN_KS:
        if splitk and (K + 63) // 64 < splitk:
            continue
        for M, N in pairs:
            out.append(Spec(M, N, K, impl=impl, splitk=splitk, groups=1, c_f32=1, w_t=1, act=2))
            out.append(Spec(M, N, K, impl=impl, splitk=splitk, groups=1, w_t=1))
            if N > 8:
                for mode in (3, 4):
                    out.append(Spec(M, N, K, impl=impl, splitk=splitk, groups=1, c_f32=1, w_t=2, c2=True, c2_copy=mode, bias=False))
                    out.append(Spec(M, N, K, impl=impl, splitk=splitk, groups=1, c_f32=1, a_t=1, w_t=2, c2=True, c2_copy=mode, bias=False))
            out.append(Spec(M, N, K, impl=impl, splitk=splitk, groups=1, c_f32=1, a_t=1, w_t=1))
    return [s for s in out if takes(impl, s) and split_used(impl, s) == max(splitk, 1)]


CONV_IMPLS = (-1, 1, 2, 3, 5, 6)


def conv_cases(impl, dname):
    """B chosen so that M = B * h * h crosses the tile's row edge; packed and padded image pitch."""
    bm = tile_of(impl, dname)[0]
    out = []
    for k3, up, cin, h, extra in ((1, 1, 8, 4, 0), (1, 2, 24, 8, 1), (1, 4, 72, 12, 0), (2, 1, 24, 12, 1), (2, 2, 72, 4, 0),
                                  (2, 4, 8, 8, 0), (0, 1, 72, 8, 1), (0, 2, 8, 12, 0), (0, 4, 24, 4, 1), (1, 1, 72, 8, 0),
                                  (1, 2, 8, 12, 1), (2, 4, 24, 4, 0)):
        B = bm // (h * h) + 1
        M, K = B * h * h, (9 if k3 else 1) * cin
        out.append(Spec(M, 40, K, impl=impl, dtype=dname, act=2, c_f32=1, r=1, conv=(h, up, cin, k3, extra)))
        out.append(Spec(M, 72, K, impl=impl, dtype=dname, act=2, conv=(h, up, cin, k3, extra)))
    return [s for s in out if takes(impl, s)]


BIG_IMPLS = (5, 6, 7, 8, 0)


def big_cases(impl):
    """More than 512 workgroups with tiles_m 9 (a row group and one tile), 12 (and half a group), 16 (two groups);
    the workgroup count comes from two groups (and K slices on impl 5 / 6), not from a large N."""
    bm, bn = TILES[8 if impl == 0 else impl][:2]
    out = []
    for tm, K in ((9, 64), (12, 72), (16, 72), (9, 72)):
        M = tm * bm - 3
        if impl in (5, 6) and K == 72:
            tn = 512 // (4 * tm) + 1
            out.append(Spec(M, tn * bn - 8, K, impl=impl, splitk=2, ws_floats=24 << 20, act=2))
        else:
            groups = 1 if (tm, K) == (9, 72) else 2
            tn = 512 // (groups * tm) + 1
            out.append(Spec(M, tn * bn - 8, K, impl=impl, groups=groups, act=2))
    return out


ROWSCALE_IMPLS = (0, 8)


def rowscale_cases(impl):
    M = 128 * 2 + 5
    out = []
    for div in (1, 7, M):
        out.append(Spec(M, 136, 72, impl=impl, row_scale_div=div, c_f32=1, r=1, c2=True, c2_copy=1))
        out.append(Spec(M, 136, 72, impl=impl, row_scale_div=div, r=1))
    return out


def multi_cases(mode, impl, n):
    """n problems of different (M, N, K) for one mmt_gemm_multi launch."""
    bm, bn = tile_of(impl)[:2]
    if mode == "conv":
        probs = [Spec(2 * 64, 40, 216, impl=impl, act=2, conv=(8, 1, 24, 1, 0)),
                 Spec(2 * 144, 72, 72, impl=impl, act=2, c_f32=1, r=1, conv=(12, 2, 8, 1, 1), groups=1),
                 Spec(9 * 16, 8, 72, impl=impl, conv=(4, 1, 72, 0, 0)),
                 Spec(3 * 64, bn + 8, 648, impl=impl, act=2, conv=(8, 4, 72, 2, 0))]
    else:
        probs = [Spec(bm + 1, bn + 8, 72, impl=impl, act=2, c_f32=1, r=1),
                 Spec(bm - 1, 8, 584, impl=impl, groups=1),
                 Spec(1, bn - 8, 56, impl=impl, r=2, c2=True, r_mode=1, r_p0=1),
                 Spec(bm + bm // 2 + 3, bn, 264, impl=impl, c_f32=1, k_split=136, groups=1)]
    return [p.but(seed=i + 1) for i, p in enumerate(probs[:n])]


def multi_one_launch(specs):
    """mmt_gemm_multi takes the problems in one launch (mmt_gemm_select's answer for the array; it answers for
    mmt_gemm when asked about one problem, so for a single spec: an LDS-DMA kernel takes it)."""
    L = _lib()
    if len(specs) == 1:
        return kernel_of(specs[0])[0] == "glds"
    arr = (L.GemmParams * len(specs))(*[params_of(s) for s in specs])
    c = L.gemm_select(arr, dtype_code(specs[0].dtype), len(specs))
    return c is not None and c.family == L.GEMM_LDS_DMA and c.joint == len(specs)


LN_IMPLS = {1: (0, 1, 2, 3, 4, 5, 6), 2: (0, 1, 2, 3, 4, 5, 6, 8)}
LN_KS = {1: (64, 128, 512, 72, 200), 2: (64, 128, 512)}
LN_EPS = 1e-6
LN_BAR = 2.0 ** -19


def ln_cases(impl, mode):
    bm, bn = tile_of(impl)[:2]
    return [Spec(bm + 1, bn + 8, K, impl=impl, c_f32=1, ln_fold=mode) for K in LN_KS[mode]]


def all_cases():
    """Every spec of every list (the host test's coverage and predicate checks)."""
    out = []
    for d, i in SWEEP:
        for e in EPILOGUES:
            out += [("sweep", i, s) for s in sweep_cases(d, i, e)]
    for i in SPLIT_IMPLS:
        for n in range(2, 9):
            out += [("split", i, s) for s in split_cases(i, n)]
    for i in ROWMAP_IMPLS:
        out += [("rowmap", i, s) for s in rowmap_cases(i)]
    for i in MN_IMPLS:
        for n in (0, 3):
            out += [("mn", i, s) for s in mn_cases(i, n)]
    for i in CONV_IMPLS:
        for d in ("bf16", "f32"):
            out += [("conv", i, s) for s in conv_cases(i, d)]
    for i in BIG_IMPLS:
        out += [("big", i, s) for s in big_cases(i)]
    for i in ROWSCALE_IMPLS:
        out += [("rowscale", i, s) for s in rowscale_cases(i)]
    for mode in (1, 2):
        for i in LN_IMPLS[mode]:
            out += [("ln", i, s) for s in ln_cases(i, mode)]
    return out


# ------------------------------------------------------------------------------------------------ operands
def _nonzero(shape, g):
    v = torch.randint(1, 4, shape, generator=g)
    return v * (torch.randint(0, 2, shape, generator=g) * 2 - 1)


def _chunk_parity(x, first, g):
    """Makes every aligned 8-chunk partial sum of A W^T odd, hence nonzero, so a dropped chunk shows in every
    output element and not only in the ~97 % where eight random products do not cancel: in the chunks of parity
    `first` along the last dim x holds an odd number of odd values, in the others only odd values (A is given
    first = 0, W first = 1: in every chunk one operand is all odd and the other has an odd count of odd
    values, so the chunk holds an odd number of odd products).  Values stay in {-3, ..., 3} without 0."""
    K = x.shape[-1]
    nc = (K + 7) // 8
    xp = torch.zeros(x.shape[:-1] + (nc * 8,), dtype=x.dtype)
    xp[..., :K] = x
    xp = xp.view(x.shape[:-1] + (nc, 8))
    sgn = torch.sign(xp)
    odd13 = torch.randint(0, 2, xp.shape, generator=g) * 2 + 1
    all_odd = torch.where(xp.abs() == 2, sgn * odd13, xp)
    even_cnt = (xp % 2 != 0).sum(-1) % 2 == 0
    e0 = xp[..., 0]
    flipped = torch.where(e0.abs() == 2, torch.sign(e0), 2 * torch.sign(e0))  # one value's parity changed
    odd_cnt = xp.clone()
    odd_cnt[..., 0] = torch.where(even_cnt, flipped, e0)
    sel = (torch.arange(nc) % 2 == first).view((1,) * (xp.dim() - 2) + (nc, 1))
    return torch.where(sel, odd_cnt, all_odd).reshape(x.shape[:-1] + (nc * 8,))[..., :K].contiguous()


def exact_matmul(A, W):
    """[G][M][K] x [G][N][K] -> int64 [G][M][N]."""
    if A.shape[1] * W.shape[1] * A.shape[2] * A.shape[0] > 1 << 28:
        return torch.einsum("gmk,gnk->gmn", A.double(), W.double()).to(torch.int64)
    return torch.einsum("gmk,gnk->gmn", A.to(torch.int64), W.to(torch.int64))


def conv_ref(x, W, h, up, cin, k3):
    """float64 F.conv2d on the nearest-upsampled integer input: x [G][B][hi][hi][cin], W [G][N][K] -> int64 [G][M][N]."""
    out = []
    for g in range(x.shape[0]):
        xu = x[g].double().permute(0, 3, 1, 2).repeat_interleave(up, 2).repeat_interleave(up, 3)
        N = W.shape[1]
        if k3:
            w4 = W[g].double().view(N, 3, 3, cin).permute(0, 3, 1, 2)
            if k3 == 2:
                w4 = w4.flip(2, 3)
            y = F.conv2d(xu, w4.contiguous(), padding=1)
        else:
            y = F.conv2d(xu, W[g].double().view(N, cin, 1, 1))
        out.append(y.permute(0, 2, 3, 1).reshape(-1, N))
    return torch.stack(out).round().to(torch.int64)


def operands(M, N, K, G, seed, conv=None):
    """Integer A [G][M][K] (conv: the input maps [G][B][hi][hi][cin]), W [G][N][K], bias [G][N] and acc = A W^T:
    computed once per shape and shared by the tests (the large grids' are not kept)."""
    return (_operands_cached if G * M * N <= 1 << 20 else _operands)(M, N, K, G, seed, conv)


def _operands(M, N, K, G, seed, conv=None):
    g = torch.Generator().manual_seed(((M * 1315423911) ^ (N * 2654435761) ^ (K * 97) ^ (G * 7) ^ seed) & 0x7FFFFFFF)
    W = _nonzero((G, N, K), g)
    bias = torch.randint(-8, 9, (G, N), generator=g)
    if conv:
        h, up, cin, k3 = conv
        A = _nonzero((G, M // (h * h), h // up, h // up, cin), g)
        acc = conv_ref(A, W, h, up, cin, k3)
    else:
        A, W = _chunk_parity(_nonzero((G, M, K), g), 0, g), _chunk_parity(W, 1, g)
        acc = exact_matmul(A, W)
    return A, W, bias, acc


_operands_cached = functools.lru_cache(maxsize=1024)(_operands)


def _image(rows, ld, dtype):
    return torch.full((rows, ld), NAN, dtype=dtype)


@dataclasses.dataclass
class Problem:
    spec: Spec
    geo: dict
    inp: dict      # name -> list over groups of storage tensors (row_scale: one tensor)
    out: dict      # name -> list over groups of pre-launch output storage ("c", "c2", "stats")
    expect: dict   # name -> list over groups of expected storage after the launch
    acc: torch.Tensor = None


def reference(s, acc, bias, R, scale=None):
    """Integer epilogue: (C, C2) as exact int64 [G][M][N] (C2 None without one); R already row-mapped to [G][M][N]."""
    pre = acc + (bias[:, None, :] if bias is not None else 0)
    v = pre.clamp(min=0) if s.act == 2 else pre
    if scale is not None:
        v = v * scale[None, :, None]
    vr = v + R if R is not None else v
    if not s.c2:
        return vr, None
    if s.c2_copy == 0:
        return v, vr
    if s.c2_copy == 2:
        return vr, pre
    return vr, vr  # 1: the copy; 3 / 4: the column split of the same values


def build(s):
    """Poisoned storage and expected storage images of a spec (CPU)."""
    assert s.act in (0, 2) and s.K <= 4096
    dt = DT[s.dtype]
    cdt = torch.float32 if s.c_f32 else dt
    G, M, N, K = s.groups, s.M, s.N, s.K
    geo = geometry(s)
    ckey = s.conv[:4] if s.conv else None
    Nw = N - 8 if s.w_t == 2 else N
    A, W, bias, acc = operands(M, Nw, K, G, s.seed, ckey)
    if s.w_t == 2:  # column N - 8 all ones, N - 7 .. N - 1 zero
        ones = torch.ones(G, 1, K, dtype=W.dtype)
        acc = torch.cat([acc, exact_matmul(A, ones), torch.zeros(G, M, 7, dtype=acc.dtype)], 2)
        bias = torch.cat([bias, torch.zeros(G, 8, dtype=bias.dtype)], 1)
    g = torch.Generator().manual_seed(M * 31 + N * 17 + K + s.seed + 5)
    inp, out, expect = {"a": [], "a1": [], "w": [], "bias": [], "r": []}, {"c": [], "c2": [], "stats": []}, {"c": [], "c2": [], "stats": []}
    crow = c_phys_rows(s)
    rrow = r_phys_rows(s)
    n_r = rrow.max().item() + 1
    Rv = torch.randint(-64, 65, (G, n_r, N), generator=g) if s.r else None
    scale = None
    if s.row_scale_div:
        scale = torch.randint(0, 3, ((M + s.row_scale_div - 1) // s.row_scale_div,), generator=g)
        inp["row_scale"] = torch.cat([scale.float(), torch.full((PAD,), NAN)])
        scale = scale[torch.arange(M) // s.row_scale_div]
    refc, refc2 = reference(s, acc, bias if s.bias else None, Rv[:, rrow] if s.r else None, scale)
    lda = geo["lda"]
    for q in range(G):
        if s.conv:
            h, up, cin, k3, extra = s.conv
            hi, B = h // up, M // (h * h)
            a = _image(geo["a_rows"] + PAD, lda, dt)  # rows are pixels
            px = (torch.arange(B)[:, None] * geo["img_pitch"] + torch.arange(hi * hi)[None]).reshape(-1)
            a[px, :cin] = A[q].reshape(-1, cin).to(dt)
            inp["a"].append(a)
        elif s.a_t:
            a = _image(K + PAD, lda, dt)
            a[:K, :M] = A[q].t().to(dt)
            inp["a"].append(a)
        else:
            rows = a_phys_rows(s, geo)
            k0 = s.k_split or K
            a = _image(geo["a_rows"] + PAD, lda, dt)
            a[rows, :k0] = A[q, :, :k0].to(dt)
            inp["a"].append(a)
            if s.k_split:
                a1 = _image(geo["a_rows"] + PAD, lda, dt)
                a1[rows, :K - k0] = A[q, :, k0:].to(dt)
                inp["a1"].append(a1)
        if s.w_t:
            w = _image(K + PAD, geo["ldw"], dt)
            w[:K, :Nw] = W[q].t().to(dt)
        else:
            w = _image(N + PAD, K, dt)
            w[:N] = W[q].to(dt)
        inp["w"].append(w)
        if s.bias:
            inp["bias"].append(torch.cat([bias[q].float(), torch.full((PAD,), NAN)]))
        ldc, crows = geo["ldc"], geo["c_rows"] + PAD
        c0 = _image(crows, ldc, cdt)
        if s.r:
            if s.r_inplace:
                c0[rrow, :N] = Rv[q, rrow].to(cdt)
            else:
                r = _image(n_r + PAD, geo["ldr"], dt if s.r == 2 else torch.float32)
                r[:n_r, :N] = Rv[q].to(r.dtype)
                inp["r"].append(r)
        ec = _image(crows, ldc, cdt)
        if s.c2_copy in (3, 4):
            ec[crow, :N - 8] = refc[q][:, :N - 8].float().to(cdt)
            nb = 8 if s.c2_copy == 3 else 1
            e2 = torch.full((M * nb + PAD,), NAN, dtype=cdt)
            e2[:M * nb] = refc[q][:, N - 8:N - 8 + nb].float().to(cdt).reshape(-1)
            out["c2"].append(torch.full_like(e2, NAN))
            expect["c2"].append(e2)
        else:
            ec[crow, :N] = refc[q].float().to(cdt)
            if s.c2:
                c2dt = dt if s.c2_copy else cdt
                e2 = _image(crows, ldc, c2dt)
                # c2_copy 2 with the compact epilogue stores the pre-activation at the plain row
                e2[crow, :N] = refc2[q].float().to(c2dt)
                out["c2"].append(torch.full_like(e2, NAN))
                expect["c2"].append(e2)
                if s.stats:
                    v = e2[crow, :N].double().view(M, N // 64, 64)
                    es = _image(crows, 2 * (N // 64), torch.float32)
                    es[crow] = torch.stack([v.sum(-1), (v * v).sum(-1)], -1).reshape(M, -1).float()
                    out["stats"].append(torch.full_like(es, NAN))
                    expect["stats"].append(es)
        out["c"].append(c0 if s.r_inplace else torch.full_like(ec, NAN))
        expect["c"].append(ec)
    return Problem(s, geo, inp, out, expect, acc)


def build_ln(s):
    """Folded LayerNorm: A rows hold 1 and 3 in equal numbers (mean 2, variance 1, exact integer sums), W and
    ln_colsum integers; expect["c"] is the float64 rstd * (acc - mu * colsum) + bias."""
    assert s.ln_fold and s.c_f32 and s.K % 2 == 0
    dt = DT[s.dtype]
    G, M, N, K = s.groups, s.M, s.N, s.K
    geo = geometry(s)
    g = torch.Generator().manual_seed(M + N * 3 + K * 5 + s.ln_fold)
    base = torch.cat([torch.ones(K // 2), torch.full((K // 2,), 3.0)]).to(torch.int64)
    A = torch.stack([torch.stack([base[torch.randperm(K, generator=g)] for _ in range(M)]) for _ in range(G)])
    W = _nonzero((G, N, K), g)
    bias = torch.randint(-8, 9, (G, N), generator=g)
    acc = exact_matmul(A, W)
    colsum = W.sum(-1)
    rstd = 1.0 / math.sqrt(1.0 + LN_EPS)
    ref = rstd * (acc.double() - 2.0 * colsum.double()[:, None, :]) + bias.double()[:, None, :]
    inp = {"a": [], "w": [], "bias": [], "colsum": [], "stats_in": []}
    out, expect = {"c": []}, {"c": []}
    for q in range(G):
        a = _image(M + PAD, geo["lda"], dt)
        a[:M, :K] = A[q].to(dt)
        w = _image(N + PAD, K, dt)
        w[:N] = W[q].to(dt)
        inp["a"].append(a)
        inp["w"].append(w)
        inp["bias"].append(torch.cat([bias[q].float(), torch.full((PAD,), NAN)]))
        inp["colsum"].append(torch.cat([colsum[q].float(), torch.full((PAD,), NAN)]))
        if s.ln_fold == 2:
            v = A[q].double().view(M, K // 64, 64)
            st = _image(M + PAD, 2 * (K // 64), torch.float32)
            st[:M] = torch.stack([v.sum(-1), (v * v).sum(-1)], -1).reshape(M, -1).float()
            inp["stats_in"].append(st)
        e = torch.full((M + PAD, geo["ldc"]), NAN, dtype=torch.float64)
        e[:M, :N] = ref[q]
        out["c"].append(torch.full((M + PAD, geo["ldc"]), NAN))
        expect["c"].append(e)
    return Problem(s, geo, inp, out, expect, acc)


def same(got, want):
    """Bitwise agreement of a storage image with its expectation, NaN guards included."""
    return bool(((got == want) | (torch.isnan(got) & torch.isnan(want))).all())


def describe(got, want):
    """What differs: wrong or unwritten values inside the region, NaN read into it, guard elements touched."""
    region = ~torch.isnan(want)
    nan_in = int((torch.isnan(got) & region).sum())
    wrong = int(((got != want) & region & ~torch.isnan(got)).sum())
    guard = int((~torch.isnan(got) & ~region).sum())
    msg = "%d wrong values, %d NaN (unwritten, or a surplus element read) in the region, %d guard elements written" % (wrong, nan_in, guard)
    bad = ((got != want) & region) | (~torch.isnan(got) & ~region)
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        msg += "; first at %s: got %r, expected %r" % (i, got[i].item(), want[i].item())
    return msg
