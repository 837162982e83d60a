"""Probe inputs and fp64 references of the normalisation / staging kernels of csrc/norm.hip (no tests here):
mmt_layernorm, mmt_layernorm_bwd / _bwd_add, mmt_groupnorm, mmt_groupnorm_bwd, mmt_add_cast, mmt_scale_rows_cast
and mmt_patch_im2col.

Bitwise families: add_cast, scale_rows_cast and patch_im2col are movement plus one fp32 operation and one rounding, so
every output element is known bit for bit; the output gradients of both backwards are integers of magnitude 1..3
(exact in bf16 and fp16), so every partial sum of dbeta is an exact integer in any order.

Bar families: the fp32 outputs y and dx are held within delta = max(4 x max|oracle in fp32 - oracle in fp64|,
2^-20 max|ref|) of the float64 oracle (plain torch: F.layer_norm / F.group_norm and autograd), 16-bit outputs within
msda_probes.bar(ref, delta, dtype) elementwise; delta comes from the oracle alone, never from the device.  dgamma has a
counted worst-case bar (ln_dgamma_bar, gn_dgamma_bar).

Data variants of the normalised families: randn (3 randn + 1), offset (the row's or group's mean is 50 standard
deviations: a one-pass variance fails), small (standard deviation 2^-6 and eps 1e-6, so eps decides 2 % of the output:
a launch with 1e-5 fails).  gamma and beta of the two parameter sets and every add row are drawn independently.

Storage images (head_probes.image / poison, gemm_probes.same / describe) are GUARD rows larger than the problem, NaN
outside it, and compared whole.  restate_*() are private restatements of the same arithmetic with one planted defect
(the host test's negative controls) and, in fp32, with the kernel's own summation order (the host test's proof that
each bar can be met).
"""
import dataclasses
import functools

import torch
import torch.nn.functional as F

import gemm_probes as P
import head_probes as H
import msda_probes as M

NAN = P.NAN
GUARD = H.GUARD
EBADARG = H.EBADARG
U32 = H.U32
F64, F32, BF16, F16 = torch.float64, torch.float32, torch.bfloat16, torch.float16
DT = {"f32": F32, "bf16": BF16, "fp16": F16}
bar, expected = M.bar, M.expected

LNB_RPW = 32                 # rows per workgroup of layernorm_bwd_kernel
RED_UNROLL, RED_RUNS = 16, 4  # layernorm_bwd_reduce_kernel: loads in flight, contiguous runs of workgroups
GN_THREADS, GN_VMAX = 512, 12
GNB_LDS = 2 * 9600
LN_CS = (256, 512, 768, 1024)
VARIANTS = ("randn", "offset", "small")
DTYPES = ("f32", "bf16", "fp16")


def delta_of(r32, r64):
    """The project's bar for an fp32 kernel against the fp32 restatement of its reference (msda_probes.delta)."""
    return max(4.0 * float((r32.double() - r64).abs().max()), 2.0 ** -20 * float(r64.abs().max()))


def _data(shape, variant, g):
    """fp32 values whose last-axis statistics follow the variant (the add rows are drawn at half that deviation)."""
    r = torch.randn(shape, generator=g)
    if variant == "randn":
        return 3 * r + 1
    if variant == "offset":
        return r + 50
    return (r + 1) * 2.0 ** -6


def _add_rows(shape, variant, g):
    return torch.randn(shape, generator=g) * {"randn": 1.5, "offset": 0.5, "small": 2.0 ** -7}[variant]


def _ints(shape, g):
    """Output gradients / residual gradients: integers of magnitude 1..3, never 0."""
    return H._nonzero(shape, 1, 3, g).float()


# ------------------------------------------------------------------------------------------------ 1. layernorm
LN_ROWS = (1, 3, 4, 5, 50)
LN_SETS = (("none0", 0), ("none_rows", 0), ("two", 1), ("two", 7), ("two", 25))
LN_ADDS = (0, 1, 7, 25, 50)
LN_OUTS = ("f32", "typed", "both", "inplace", "inplace_typed")


@dataclasses.dataclass(frozen=True)
class LNCase:
    C: int
    rows: int
    sets: str        # none0: gamma1 NULL, rows_per_group 0; none_rows: gamma1 NULL, rows_per_group = rows; two
    rpg: int         # rows per set (two)
    add_rows: int    # 0: add NULL
    out: str         # f32 / typed / both: separate buffers; inplace: out_f32 == in; inplace_typed: and a typed output
    dtype: str
    variant: str

    @property
    def eps(self):
        return 1e-6 if self.variant == "small" or self.C != 256 else 1e-5  # backbone 1e-6, fusion encoder (C 256) 1e-5

    @property
    def rpg_arg(self):
        return {"none0": 0, "none_rows": self.rows, "two": self.rpg}[self.sets]

    @property
    def has_f32(self):
        return self.out != "typed"

    @property
    def has_typed(self):
        return self.out in ("typed", "both", "inplace_typed")


def _ln_cases():
    out = []
    pairs = [(o, d) for o in LN_OUTS for d in DTYPES]
    k = 0
    for si, (sets, rpg) in enumerate(LN_SETS):      # every (set form x add form) at 50 rows
        for ai, add_rows in enumerate(LN_ADDS):
            o, d = pairs[k % len(pairs)]
            out.append(LNCase(LN_CS[(si + ai) % 4], 50, sets, rpg, add_rows, o, d, VARIANTS[(si + 2 * ai) % 3]))
            k += 1
    for ri, rows in enumerate(LN_ROWS[:4]):          # every rows % 4 below two workgroups, at every C
        for ci, C in enumerate(LN_CS):
            sets, rpg = (("none0", 0), ("none_rows", 0), ("two", 1))[(ri + ci) % 3]
            o, d = pairs[k % len(pairs)]
            out.append(LNCase(C, rows, sets, rpg, (0, 1, 7)[(ri + 2 * ci) % 3], o, d, VARIANTS[(ri + ci) % 3]))
            k += 1
    return tuple(out)


LN_CASES = _ln_cases()


def ln_id(c):
    return "C%d-r%d-%s%s-add%d-%s-%s-%s" % (c.C, c.rows, c.sets, c.rpg if c.sets == "two" else "", c.add_rows, c.out,
                                            c.dtype, c.variant)


def set_of_rows(rows, rpg, two):
    """Which parameter set a row takes: sets alternate every rpg rows."""
    r = torch.arange(rows)
    return ((r // rpg) & 1).bool() if two else torch.zeros(rows, dtype=torch.bool)


@functools.lru_cache(maxsize=None)
def ln_problem(c):
    g = H._gen(c.C, c.rows, len(c.sets), c.rpg, c.add_rows, len(c.out), len(c.dtype), len(c.variant))
    add = _add_rows((c.add_rows, c.C), c.variant, g) if c.add_rows else None
    x = _data((c.rows, c.C), c.variant, g)
    if add is not None:
        x = x - 0.5 * add[torch.arange(c.rows) % c.add_rows]  # x + add keeps the variant's statistics
    g0, b0, g1, b1 = (torch.randn(c.C, generator=g) for _ in range(4))
    return dict(x=x, add=add, g0=g0, b0=b0, g1=g1, b1=b1, sel=set_of_rows(c.rows, max(c.rpg, 1), c.sets == "two"))


def _affine(pr, dtype):
    sel = pr["sel"][:, None]
    return torch.where(sel, pr["g1"].to(dtype), pr["g0"].to(dtype)), torch.where(sel, pr["b1"].to(dtype), pr["b0"].to(dtype))


def ln_oracle(c, dtype=F64):
    """F.layer_norm of x + add[row % add_rows] with the row's set of gamma / beta, computed in `dtype`."""
    pr = ln_problem(c)
    v = pr["x"].to(dtype)
    if pr["add"] is not None:
        v = v + pr["add"].to(dtype)[torch.arange(c.rows) % c.add_rows]
    G, B = _affine(pr, dtype)
    return F.layer_norm(v, (c.C,), None, None, c.eps) * G + B


@functools.lru_cache(maxsize=None)
def ln_reference(c):
    """(y in float64, delta): computed once, shared, never modified."""
    r64 = ln_oracle(c, F64)
    return r64, delta_of(ln_oracle(c, F32), r64)


def _seq_sum(t):
    """Sum over the last axis in index order, one rounding per addition in t's type."""
    s = torch.zeros(t.shape[:-1], dtype=t.dtype)
    for i in range(t.shape[-1]):
        s = s + t[..., i]
    return s


_XOR = [torch.arange(64) ^ o for o in (32, 16, 8, 4, 2, 1)]


def _wave_sum(s):
    """wave_sum of common.hpp on [...][64] lanes: six xor-butterfly levels (every lane ends with the same value)."""
    for perm in _XOR:
        s = s + s[..., perm]
    return s[..., 0]


def _f4(t):
    return ((t[..., 0] + t[..., 1]) + t[..., 2]) + t[..., 3]


def _row_sum(t):
    """Sum of the last axis (C = 256 V).  fp32: in the LayerNorm kernels' order -- lane l adds the float4 granules
    l, l + 64, ..., each as ((x + y) + z) + w, then the butterfly; float64: torch's."""
    if t.dtype != F32:
        return t.sum(-1)
    g = t.reshape(t.shape[:-1] + (t.shape[-1] // 256, 64, 4))
    s = torch.zeros(t.shape[:-1] + (64,), dtype=F32)
    for i in range(g.shape[-3]):
        s = s + _f4(g[..., i, :, :])
    return _wave_sum(s)


def _group_sum(v):
    """Sum over the last two axes [P][cg] of a group.  fp32: in the GroupNorm kernels' order -- thread t adds the
    float4 items t, t + 512, ..., then the butterfly of its wave, then the 8 wave sums in order; float64: torch's."""
    if v.dtype != F32:
        return v.sum((-1, -2))
    lead = v.shape[:-2]
    items = v.shape[-2] * v.shape[-1] // 4
    pad = torch.zeros(lead + (GN_THREADS * GN_VMAX, 4), dtype=F32)
    pad[..., :items, :] = v.reshape(lead + (items, 4))
    g = pad.view(lead + (GN_VMAX, GN_THREADS, 4))
    s = torch.zeros(lead + (GN_THREADS,), dtype=F32)
    for i in range(-(-items // GN_THREADS)):
        s = s + _f4(g[..., i, :, :])
    return _seq_sum(_wave_sum(s.view(lead + (GN_THREADS // 64, 64))))


def _stats(v, n, eps, mut):
    """(mean, rstd) of the last axis as the kernels compute them: _row_sum * (1 / n), two-pass variance, rsqrt."""
    inv_n = torch.tensor(1.0, dtype=v.dtype) / n
    s = _row_sum(v)
    if mut == "skip_mean":  # the row's largest element
        s = s - v.gather(-1, v.abs().argmax(-1, keepdim=True))[..., 0]
    mean = s * inv_n
    if mut == "one_pass":
        var = _row_sum(v * v) * inv_n - mean * mean
    else:
        d = v - mean[..., None]
        var = _row_sum(d * d) * inv_n
    return mean, torch.rsqrt(var + torch.tensor(eps, dtype=v.dtype))


def _other_eps(eps):
    return 1e-5 if eps == 1e-6 else 1e-6


def restate_ln(c, dtype=F64, mut=None):
    """The forward restated: fp32 with the kernel's row sum (_row_sum), float64 with torch's.  Mutations: skip_mean (one element
    left out of the mean), one_pass (E[x^2] - mean^2), eps (the other launch's value), gamma_set / beta_set (the
    first row of set 1 takes set 0's), add_map (row % rows_per_group), neighbour (the next row's statistics)."""
    pr = ln_problem(c)
    rows = torch.arange(c.rows)
    v = pr["x"].to(dtype)
    if pr["add"] is not None:
        amap = (rows % c.rpg) % c.add_rows if mut == "add_map" else rows % c.add_rows
        v = v + pr["add"].to(dtype)[amap]
    mean, rstd = _stats(v, c.C, _other_eps(c.eps) if mut == "eps" else c.eps, mut)
    if mut == "neighbour":
        mean, rstd = torch.roll(mean, -1), torch.roll(rstd, -1)
    G, B = _affine(pr, dtype)
    if mut in ("gamma_set", "beta_set"):
        (G if mut == "gamma_set" else B)[c.rpg] = (pr["g0"] if mut == "gamma_set" else pr["b0"]).to(dtype)
    return (v - mean[:, None]) * rstd[:, None] * G + B


def ln_mutations(c):
    """The planted defects that change this case's arithmetic at all."""
    out = ["skip_mean", "eps"] if c.variant == "small" else ["skip_mean"]
    if c.variant == "offset":
        out.append("one_pass")
    if c.sets == "two" and c.rows > c.rpg:
        out += ["gamma_set", "beta_set"]
        r = torch.arange(c.rows)
        if c.add_rows and not torch.equal((r % c.rpg) % c.add_rows, r % c.add_rows):
            out.append("add_map")
    if c.rows > 1:
        out.append("neighbour")
    return out


# ------------------------------------------------------------------------------------------------ 2. layernorm backward
LNB_SMALL_ROWS, LNB_BIG_ROWS, LNB_BIG_CS = (1, 31, 32, 33, 77), (2016, 2048, 2053), (256, 768)
LNB_RPGS = (1, 5, 40, 500)
LNB_DRES = ("none", "separate", "alias")


@dataclasses.dataclass(frozen=True)
class LNBCase:
    C: int
    rows: int
    rpg: int         # 0: one set (gamma1 NULL)
    dres: str
    dtype: str       # of dy
    variant: str

    @property
    def eps(self):
        return 1e-6 if self.variant == "small" or self.C != 256 else 1e-5

    @property
    def nwg(self):
        return (self.rows + LNB_RPW - 1) // LNB_RPW

    @property
    def sets(self):
        return 2 if self.rpg else 1


def _lnb_cases():
    out, k = [], 0
    for rows in LNB_SMALL_ROWS:
        for C in LN_CS:
            out.append(LNBCase(C, rows, (0, 1, 5, 40)[k % 4] if rows > 1 else (0, 1)[k % 2], LNB_DRES[(k + k // 4) % 3],
                               DTYPES[(k + k // 3) % 3], VARIANTS[(k + k // 5) % 3]))
            k += 1
    for rows in LNB_BIG_ROWS:
        for C in LNB_BIG_CS:
            out.append(LNBCase(C, rows, (500, 0, 5, 500, 40, 1)[k % 6], LNB_DRES[(k + 1) % 3], DTYPES[k % 3],
                               VARIANTS[(k + k // 2) % 3]))
            k += 1
    return tuple(out)


LNB_CASES = _lnb_cases()


def lnb_id(c):
    return "C%d-r%d-rpg%d-dres_%s-%s-%s" % (c.C, c.rows, c.rpg, c.dres, c.dtype, c.variant)


def reduce_runs(nwg):
    """What the four runs of layernorm_bwd_reduce_kernel do with nwg partials: (unrolled passes, tail iterations)."""
    out = []
    for run in range(RED_RUNS):
        n = (run + 1) * nwg // RED_RUNS - run * nwg // RED_RUNS
        out.append((n // RED_UNROLL, n % RED_UNROLL))
    return out


def reduce_classes(nwgs):
    return {(p > 0, t > 0) for n in nwgs for p, t in reduce_runs(n)}


@functools.lru_cache(maxsize=None)
def lnb_problem(c):
    g = H._gen(c.C, c.rows, c.rpg, len(c.dres), len(c.dtype), len(c.variant), 3)
    x = _data((c.rows, c.C), c.variant, g)
    dy = _ints((c.rows, c.C), g)
    dres = _ints((c.rows, c.C), g) if c.dres != "none" else None
    g0, g1 = torch.randn(c.C, generator=g), torch.randn(c.C, generator=g)
    prefill = H._nonzero((4, c.C), 1, 9, g).float()
    return dict(x=x, dy=dy, dres=dres, g0=g0, g1=g1, prefill=prefill, sel=set_of_rows(c.rows, max(c.rpg, 1), c.rpg > 0))


def lnb_oracle(c, dtype=F64):
    """Autograd through F.layer_norm in `dtype`: dx (+ dres) [rows][C] and dgb [2 sets][C] as (dgamma0, dbeta0,
    dgamma1, dbeta1); with one set only the first two rows."""
    pr = lnb_problem(c)
    x = pr["x"].to(dtype).clone().requires_grad_(True)
    g0, g1 = pr["g0"].to(dtype).clone().requires_grad_(True), pr["g1"].to(dtype).clone().requires_grad_(True)
    b0, b1 = torch.zeros(c.C, dtype=dtype, requires_grad=True), torch.zeros(c.C, dtype=dtype, requires_grad=True)
    sel = pr["sel"][:, None]
    y = F.layer_norm(x, (c.C,), None, None, c.eps) * torch.where(sel, g1, g0) + torch.where(sel, b1, b0)
    y.backward(pr["dy"].to(dtype))
    dx = x.grad if pr["dres"] is None else x.grad + pr["dres"].to(dtype)
    dgb = torch.stack([g0.grad, b0.grad, g1.grad, b1.grad][:2 * c.sets])
    return dx.detach(), dgb.detach()


def ln_dgamma_bar(c):
    """Worst-case |dgamma - reference| per column [sets][C], counted from the kernels' fixed order.
    Row statistics: K = 4 V + 6 additions on the longest chain of a row reduction (a lane's 4 V values, then the 6
    butterfly levels).  mean = sum * (1 / C): within e_mean = (K + 2) U32 mean|x| (the chain, the rounding of 1 / C
    and the product).  The variance repeats the chain over squares of differences that carry e_mean (relative
    2 e_mean rstd + 2 U32), a product, the eps add and a 1-ulp rsqrt that halves the argument's relative error:
    rstd within e_mean rstd + (K / 2 + 6) U32, relatively.  xhat = (x - mean) * rstd then lies within
    rstd e_mean (1 + |xhat|) + (K / 2 + 8) U32 |xhat| and the term dy * xhat rounds once more (dy is an integer).
    Column sum: at most 8 rows in a wave, 3 wave adds, ceil(nwg / 4) partials in a run, 3 run adds:
    n_add = 8 + 3 + ceil(nwg / 4) + 3 additions, each at most U32 of sum |terms|.
    bar = sum over the set's rows |dy| (rstd e_mean (1 + |xhat|) + (K / 2 + 9 + n_add) U32 |xhat|)."""
    pr = lnb_problem(c)
    x, dy = pr["x"].double(), pr["dy"].double()
    K = 4 * (c.C // 256) + 6
    n_add = 8 + 3 + -(-c.nwg // RED_RUNS) + 3
    mean = x.mean(1, keepdim=True)
    rstd = torch.rsqrt(((x - mean) ** 2).mean(1, keepdim=True) + c.eps)
    xhat = ((x - mean) * rstd).abs()
    e_mean = (K + 2) * U32 * x.abs().mean(1, keepdim=True)
    per = dy.abs() * (rstd * e_mean * (1 + xhat) + (K / 2 + 9 + n_add) * U32 * xhat)
    sel = pr["sel"][:, None]
    return torch.stack([(per * ~sel).sum(0), (per * sel).sum(0)][:c.sets])


@functools.lru_cache(maxsize=None)
def lnb_reference(c):
    """dx, dgb (float64), delta of dx, the dgamma bar and the per-workgroup dbeta partials [nwg][sets][C]."""
    dx, dgb = lnb_oracle(c, F64)
    dx32, _ = lnb_oracle(c, F32)
    pr = lnb_problem(c)
    pad = torch.zeros(c.nwg * LNB_RPW, c.C, dtype=F64)
    parts = []
    for s in range(2):
        pad[:c.rows] = pr["dy"].double() * (pr["sel"][:, None] == bool(s))
        parts.append(pad.view(c.nwg, LNB_RPW, c.C).sum(1))
    return dict(dx=dx, dgb=dgb, delta=delta_of(dx32, dx), dgamma_bar=ln_dgamma_bar(c), dbeta_part=torch.stack(parts, 1))


def restate_lnb(c, dtype=F64, mut=None):
    """dx = rstd (g - mean(g) - xhat mean(g xhat)) (+ dres), g = dy gamma; dgamma / dbeta summed in the kernels' order
    (fp32) or by torch (float64).  Mutations: drop_row (the last row left out of both column sums), row_other_set
    (the first row of set 1 counted to set 0), mg_no_gamma (mean(g) taken of dy), no_dres."""
    pr = lnb_problem(c)
    x, dy = pr["x"].to(dtype), pr["dy"].to(dtype)
    sel = pr["sel"].clone()
    G = torch.where(sel[:, None], pr["g1"].to(dtype), pr["g0"].to(dtype))
    mean, rstd = _stats(x, c.C, c.eps, None)
    xhat = (x - mean[:, None]) * rstd[:, None]
    g = dy * G
    inv_c = torch.tensor(1.0, dtype=dtype) / c.C
    mg = _row_sum(dy if mut == "mg_no_gamma" else g) * inv_c
    mgx = _row_sum(g * xhat) * inv_c
    dx = rstd[:, None] * (g - mg[:, None] - xhat * mgx[:, None])
    if pr["dres"] is not None and mut != "no_dres":
        dx = dx + pr["dres"].to(dtype)
    keep = torch.ones(c.rows, dtype=torch.bool)
    if mut == "drop_row":
        keep[-1] = False
    if mut == "row_other_set":
        sel[c.rpg] = False
    dgb = []
    for s in range(c.sets):
        m = (keep & (sel == bool(s)))[:, None]
        for t in (dy * xhat, dy):
            t = t * m
            if dtype == F32:  # [nwg][8 rows of a wave][4 waves][C]: rows, then waves, then the runs of workgroups, in order
                pad = torch.zeros(c.nwg * LNB_RPW, c.C, dtype=F32)
                pad[:c.rows] = t
                part = _seq_sum(_seq_sum(pad.view(c.nwg, LNB_RPW // 4, 4, c.C).permute(0, 2, 3, 1)).permute(0, 2, 1))
                runs = [_seq_sum(part[r * c.nwg // RED_RUNS:(r + 1) * c.nwg // RED_RUNS].t()) for r in range(RED_RUNS)]
                dgb.append(((runs[0] + runs[1]) + runs[2]) + runs[3])
            else:
                dgb.append(t.sum(0))
    return dx, torch.stack(dgb)


# ------------------------------------------------------------------------------------------------ 3. groupnorm
@dataclasses.dataclass(frozen=True)
class GNCase:
    P: int
    Ctot: int
    groups: int
    n_inst: int
    ips: int         # inst_per_set as passed (<= 0: every instance takes set 0)
    two: bool        # gamma1 / beta1 given
    out: str         # f32 / typed / both
    dtype: str
    variant: str

    @property
    def cg(self):
        return self.Ctot // self.groups

    @property
    def items(self):
        return self.P * self.cg // 4

    @property
    def eps(self):
        return 1e-6 if self.variant == "small" else 1e-5

    @property
    def has_f32(self):
        return self.out != "typed"

    @property
    def has_typed(self):
        return self.out != "f32"


GN_SHAPES = ((1, 32, 8), (5, 96, 4), (7, 40, 2), (64, 64, 2), (171, 24, 2), (57, 36, 1), (1024, 48, 2), (48, 512, 1))
GN_OUTS = ("f32", "typed", "both")


def _gn_cases():
    pairs = [(o, d) for o in GN_OUTS for d in DTYPES]
    out, k = [], 0
    for P_, Ctot, groups in GN_SHAPES:
        o, d = pairs[k % 9]
        out.append(GNCase(P_, Ctot, groups, 1 + k % 2, k % 2, bool(k % 2), o, d, VARIANTS[k % 3]))
        k += 1
    out.append(GNCase(400, 768, 32, 2, 1, True, "both", "bf16", "randn"))     # the frame's launch
    for ips in (0, 1, 2, 3):                                                  # three instances: set 1 from ips on
        o, d = pairs[k % 9]
        out.append(GNCase(5, 96, 4, 3, ips, True, o, d, VARIANTS[k % 3]))
        k += 1
    out.append(GNCase(7, 40, 2, 3, 1, False, "typed", "fp16", "offset"))      # gamma1 NULL: inst_per_set is ignored
    return tuple(out)


GN_CASES = _gn_cases()


def gn_id(c):
    return "P%d-C%d-g%d-n%d-ips%d-%s-%s-%s-%s" % (c.P, c.Ctot, c.groups, c.n_inst, c.ips, "two" if c.two else "one", c.out,
                                                  c.dtype, c.variant)


def gn_sets(c):
    """Instances at or past inst_per_set all take set 1 (no alternation, unlike mmt_layernorm); <= 0: none does."""
    ips = c.ips if c.ips > 0 else c.n_inst
    return (torch.arange(c.n_inst) >= ips) & bool(c.two)


def _group_data(n_inst, P_, Ctot, groups, variant, g):
    """[n_inst][P][Ctot] channels-last, each (instance, group) with the variant's statistics about its own centre."""
    cg = Ctot // groups
    x = _data((n_inst, P_, groups, cg), variant, g)
    if variant != "small":
        x = x * (1 + 0.25 * torch.arange(groups).view(1, 1, groups, 1) % 3)  # groups differ in scale as well
    return x.reshape(n_inst, P_, Ctot).contiguous()


@functools.lru_cache(maxsize=None)
def gn_problem(c):
    g = H._gen(c.P, c.Ctot, c.groups, c.n_inst, c.ips + 1, int(c.two), len(c.out), len(c.dtype), len(c.variant))
    x = _group_data(c.n_inst, c.P, c.Ctot, c.groups, c.variant, g)
    g0, b0, g1, b1 = (torch.randn(c.Ctot, generator=g) for _ in range(4))
    return dict(x=x, g0=g0, b0=b0, g1=g1, b1=b1, sel=gn_sets(c))


def gn_oracle(c, dtype=F64):
    pr = gn_problem(c)
    xhat = F.group_norm(pr["x"].to(dtype).permute(0, 2, 1), c.groups, None, None, c.eps).permute(0, 2, 1)
    sel = pr["sel"].view(-1, 1, 1)
    return xhat * torch.where(sel, pr["g1"].to(dtype), pr["g0"].to(dtype)) + torch.where(sel, pr["b1"].to(dtype), pr["b0"].to(dtype))


@functools.lru_cache(maxsize=None)
def gn_reference(c):
    r64 = gn_oracle(c, F64)
    return r64, delta_of(gn_oracle(c, F32), r64)


def _gn_stats(x, groups, eps, mut):
    """x [n][P][Ctot] -> (mean, rstd) [n][groups], two-pass, the sums by _group_sum."""
    n, P_, Ctot = x.shape
    cg = Ctot // groups
    v = x.view(n, P_, groups, cg).permute(0, 2, 1, 3)               # [n][groups][P][cg]
    cnt = torch.tensor(float(P_ * cg), dtype=x.dtype)
    tot = _group_sum
    s = tot(v)
    if mut == "skip_mean":  # the group's largest element
        s = s - v.flatten(2).gather(-1, v.flatten(2).abs().argmax(-1, keepdim=True))[..., 0]
    mean = s / cnt
    if mut == "one_pass":
        var = tot(v * v) / cnt - mean * mean
    else:
        d = v - mean[..., None, None]
        var = tot(d * d) / cnt
    return mean, torch.rsqrt(var + torch.tensor(eps, dtype=x.dtype))


def restate_gn(c, dtype=F64, mut=None):
    """Mutations: skip_mean, one_pass, eps, neighbour (the next group's statistics), gamma_set / beta_set (the first
    instance of set 1 takes set 0's)."""
    pr = gn_problem(c)
    x = pr["x"].to(dtype)
    mean, rstd = _gn_stats(x, c.groups, _other_eps(c.eps) if mut == "eps" else c.eps, mut)
    if mut == "neighbour":
        mean, rstd = (torch.roll(t.reshape(-1), -1).view(t.shape) for t in (mean, rstd))
    sel_g, sel_b = pr["sel"].clone(), pr["sel"].clone()
    if mut in ("gamma_set", "beta_set"):
        (sel_g if mut == "gamma_set" else sel_b)[int(pr["sel"].nonzero()[0])] = False
    G = torch.where(sel_g.view(-1, 1, 1), pr["g1"].to(dtype), pr["g0"].to(dtype))
    B = torch.where(sel_b.view(-1, 1, 1), pr["b1"].to(dtype), pr["b0"].to(dtype))
    ex = lambda t: t.repeat_interleave(c.cg, 1)[:, None, :]  # noqa: E731  [n][groups] -> [n][1][Ctot]
    return (x - ex(mean)) * ex(rstd) * G + B


def gn_mutations(c):
    out = ["skip_mean", "eps"] if c.variant == "small" else ["skip_mean"]
    if c.variant == "offset":
        out.append("one_pass")
    if c.groups * c.n_inst > 1:
        out.append("neighbour")
    if bool(gn_sets(c).any()):
        out += ["gamma_set", "beta_set"]
    return out


# ------------------------------------------------------------------------------------------------ 4. groupnorm backward
@dataclasses.dataclass(frozen=True)
class GNBCase:
    P: int
    Ctot: int
    groups: int
    n_inst: int
    variant: str

    @property
    def cg(self):
        return self.Ctot // self.groups

    @property
    def eps(self):
        return 1e-6 if self.variant == "small" else 1e-5

    @property
    def pc(self):
        return GNB_LDS // (2 * self.cg)

    @property
    def chunks(self):
        return -(-self.P // self.pc)

    @property
    def last_chunk(self):
        return self.P - (self.chunks - 1) * self.pc


GNB_CASES = (GNBCase(50, 8, 2, 3, "randn"), GNBCase(6144, 4, 1, 1, "offset"),                     # cg 4: PC 2400
             GNBCase(399, 48, 2, 1, "small"), GNBCase(400, 48, 2, 3, "randn"), GNBCase(401, 48, 2, 1, "offset"),
             GNBCase(1024, 48, 2, 3, "small"),                                                      # cg 24: PC 400
             GNBCase(576, 64, 2, 1, "randn"), GNBCase(768, 64, 2, 3, "offset"),                     # cg 32: PC 300
             GNBCase(343, 56, 2, 3, "small"),                                                       # cg 28: PC 342
             GNBCase(37, 256, 1, 3, "randn"), GNBCase(38, 512, 2, 1, "offset"), GNBCase(96, 256, 1, 3, "small"))  # cg 256


def gnb_id(c):
    return "P%d-C%d-g%d-n%d-%s" % (c.P, c.Ctot, c.groups, c.n_inst, c.variant)


def chunk_class(c):
    return "one" if c.last_chunk == 1 else "full" if c.last_chunk == c.pc else "partial"


@functools.lru_cache(maxsize=None)
def gnb_problem(c):
    g = H._gen(c.P, c.Ctot, c.groups, c.n_inst, len(c.variant), 4)
    x = _group_data(c.n_inst, c.P, c.Ctot, c.groups, c.variant, g)
    return dict(x=x, dy=_ints((c.n_inst, c.P, c.Ctot), g), gamma=torch.randn(c.Ctot, generator=g),
                prefill=H._nonzero((2, c.Ctot), 1, 9, g).float())


def gnb_oracle(c, dtype=F64):
    """Autograd through F.group_norm in `dtype`: dx [n][P][Ctot], dgb [2][Ctot] (dgamma, dbeta)."""
    pr = gnb_problem(c)
    x = pr["x"].to(dtype).clone().requires_grad_(True)
    ga = pr["gamma"].to(dtype).clone().requires_grad_(True)
    be = torch.zeros(c.Ctot, dtype=dtype, requires_grad=True)
    y = F.group_norm(x.permute(0, 2, 1), c.groups, ga, be, c.eps).permute(0, 2, 1)
    y.backward(pr["dy"].to(dtype))
    return x.grad.detach(), torch.stack([ga.grad, be.grad]).detach()


def gn_dgamma_bar(c):
    """As ln_dgamma_bar with the group's reductions: a thread's ceil(items / 512) float4 values (4 additions each), 6
    butterfly levels and the 8 wave sums: K = 4 ceil(items / 512) + 14; mean = sum / n: e_mean = (K + 2) U32 mean|x|;
    rstd within e_mean rstd + (K / 2 + 6) U32 relatively; xhat within rstd e_mean (1 + |xhat|) + (K / 2 + 8) U32 |xhat|,
    one more rounding for dy * xhat.  Column sum: the P positions in order, then the n_inst instances:
    n_add = P + n_inst.  bar = sum over instances and positions |dy| (rstd e_mean (1 + |xhat|) + (K / 2 + 9 + n_add)
    U32 |xhat|)."""
    pr = gnb_problem(c)
    items = c.P * c.cg // 4
    K = 4 * -(-items // GN_THREADS) + 14
    n_add = c.P + c.n_inst
    v = pr["x"].double().view(c.n_inst, c.P, c.groups, c.cg)
    mean = v.mean((1, 3), keepdim=True)
    rstd = torch.rsqrt(((v - mean) ** 2).mean((1, 3), keepdim=True) + c.eps)
    xhat = ((v - mean) * rstd).abs()
    e_mean = (K + 2) * U32 * v.abs().mean((1, 3), keepdim=True)
    per = pr["dy"].double().view(v.shape).abs() * (rstd * e_mean * (1 + xhat) + (K / 2 + 9 + n_add) * U32 * xhat)
    return per.sum((0, 1)).reshape(c.Ctot)


@functools.lru_cache(maxsize=None)
def gnb_reference(c):
    dx, dgb = gnb_oracle(c, F64)
    dx32, _ = gnb_oracle(c, F32)
    return dict(dx=dx, dgb=dgb, delta=delta_of(dx32, dx), dgamma_bar=gn_dgamma_bar(c),
                dbeta_part=gnb_problem(c)["dy"].double().sum(1))


def restate_gnb(c, dtype=F64, mut=None):
    """Mutations: mg_no_gamma, drop_pos (the last position of the first chunk left out of both column sums)."""
    pr = gnb_problem(c)
    x, dy, ga = pr["x"].to(dtype), pr["dy"].to(dtype), pr["gamma"].to(dtype)
    mean, rstd = _gn_stats(x, c.groups, c.eps, None)
    ex = lambda t: t.repeat_interleave(c.cg, 1)[:, None, :]  # noqa: E731
    xhat = (x - ex(mean)) * ex(rstd)
    g = dy * ga
    cnt = torch.tensor(float(c.P * c.cg), dtype=dtype)

    def gsum(t):  # [n][P][Ctot] -> [n][groups]
        return _group_sum(t.view(c.n_inst, c.P, c.groups, c.cg).permute(0, 2, 1, 3))

    mg, mgx = gsum(dy if mut == "mg_no_gamma" else g) / cnt, gsum(g * xhat) / cnt
    dx = ex(rstd) * (g - ex(mg) - xhat * ex(mgx))
    keep = torch.ones(c.P, dtype=torch.bool)
    if mut == "drop_pos":
        keep[min(c.pc, c.P) - 1] = False
    dgb = []
    for t in (dy * xhat, dy):
        t = (t * keep[None, :, None]).permute(0, 2, 1)             # [n][Ctot][P]
        dgb.append(_seq_sum(_seq_sum(t).t()) if dtype == F32 else t.sum((0, 2)))
    return dx, torch.stack(dgb)


# ------------------------------------------------------------------------------------------------ 5. add_cast
F16_MAX_TIE = 65520.0  # halfway between fp16's largest finite value 65504 and 2^16: from here on fp16 overflows
# (a, b): a + b is exact in fp32 and is what the cast sees; with add == NULL the input holds the sum itself
PLANTED = (
    (1.0, 2.0 ** -8), (1.0 + 2.0 ** -7, 2.0 ** -8), (-1.0, -2.0 ** -8), (-1.0 - 2.0 ** -7, -2.0 ** -8),  # bf16 ties: even, odd
    (1.0, 2.0 ** -11), (1.0 + 2.0 ** -10, 2.0 ** -11), (-3.0, -2.0 ** -10), (-3.0 - 2.0 ** -9, -2.0 ** -10),  # fp16 ties
    (F16_MAX_TIE, -2.0 ** -7), (F16_MAX_TIE, 0.0), (F16_MAX_TIE, 2.0 ** -7), (-F16_MAX_TIE, 2.0 ** -7),
    (-F16_MAX_TIE, 0.0), (65504.0, 0.0), (-65504.0, -2.0 ** -7),
    (2.0 ** -24, 0.0), (2.0 ** -24, 2.0 ** -25), (2.0 ** -23, 2.0 ** -25), (-2.0 ** -14, 2.0 ** -24),  # fp16 subnormals
    (2.0 ** -25, 0.0), (2.0 ** -25, 2.0 ** -40), (-2.0 ** -25, 0.0), (2.0 ** -15, 2.0 ** -24 + 2.0 ** -25),
)
BF16_TIES = ((0, False), (1, True), (2, False), (3, True))      # index into PLANTED, the kept value's last bit is odd
F16_TIES = ((4, False), (5, True), (6, False), (7, True))
AC_NS = (4, 1020, 1024, 1028)


@dataclasses.dataclass(frozen=True)
class ACCase:
    n: int
    add_n: int   # 0: add NULL
    out: str     # f32 / typed / both
    dtype: str


def _ac_cases():
    pairs = [(o, d) for o in GN_OUTS for d in DTYPES]
    forms = [(n, a) for n in AC_NS for a in (0, 4, n)] + [(1028, 24)]
    return tuple(ACCase(n, a, *pairs[(k + k // 9) % 9]) for k, (n, a) in enumerate(forms + forms[3:]))


AC_CASES = _ac_cases()


def ac_id(c):
    return "n%d-add%d-%s-%s" % (c.n, c.add_n, c.out, c.dtype)


def planted_slots(c):
    """(element, index into PLANTED): every fourth element from 0 on takes a planted pair, rotated by the case."""
    k = min(len(PLANTED), c.n // 4)
    rot = c.n + c.add_n + len(c.out) + len(c.dtype)
    return [(4 * i, (i + rot) % len(PLANTED)) for i in range(k)]


@functools.lru_cache(maxsize=None)
def ac_problem(c):
    """Random fp32 operands with the planted pairs: `in` takes a, the add element that position reads takes b (every
    position of the same residue shares it, so those positions take pairs with that b: planted_slots walks PLANTED in
    order and the first pair that lands on a residue decides)."""
    g = H._gen(c.n, c.add_n, len(c.out), len(c.dtype), 5)
    x = torch.randn(c.n, generator=g) * 4
    add = torch.randn(c.add_n, generator=g) if c.add_n else None
    slots = []
    for e, k in planted_slots(c):
        a, b = PLANTED[k]
        if add is None:
            x[e] = a + b
        else:
            j = e % c.add_n
            if any(e2 % c.add_n == j for e2, _ in slots):   # the residue's b is set: find the pair of this rotation with it
                cands = [kk for kk in range(len(PLANTED)) if PLANTED[kk][1] == float(add[j])]
                k = cands[(e // 4) % len(cands)]
                a, b = PLANTED[k]
            add[j] = b
            x[e] = a
        slots.append((e, k))
    want = x if add is None else x + add[torch.arange(c.n) % c.add_n]   # one fp32 addition per element
    return dict(x=x, add=add, slots=slots, want=want)


# ------------------------------------------------------------------------------------------------ 6. scale_rows_cast
SR_SHAPES = ((1, 8), (5, 264), (33, 768))
SR_ROWS_PER = (1, 2, 33, 100)
SR_SCALES = (0.0, 1.0, -2.0, 1 / 0.9)
SR_CASES = tuple((r, cols, rp, d) for r, cols in SR_SHAPES for rp in SR_ROWS_PER for d in ("bf16", "fp16"))


@functools.lru_cache(maxsize=None)
def sr_problem(case):
    rows, cols, rows_per, _ = case
    g = H._gen(rows, cols, rows_per, 6)
    x = torch.randn(rows, cols, generator=g) * 3
    ns = -(-rows // rows_per)
    scale = torch.tensor([SR_SCALES[(i + rows_per) % 4] for i in range(ns)], dtype=F32)
    return dict(x=x, scale=scale, want=x * scale[torch.arange(rows) // rows_per][:, None])  # one fp32 product


# ------------------------------------------------------------------------------------------------ 7. patch_im2col
PI_CASES = ((1, 8, 16, 4, 2), (1, 24, 40, 8, 2), (2, 16, 32, 16, 1), (3, 32, 48, 16, 2))  # (Bm, ht, hs, patch, modalities)
PI_NAMES = ("t0", "o0", "s0", "t1", "o1", "s1")


@functools.lru_cache(maxsize=None)
def pi_problem(case, coded):
    """The six images [Bm][3][h][h] (one modality: three).  coded: every pixel of every image a distinct integer
    below 2^24; else random fp32."""
    Bm, ht, hs, patch, nmod = case
    g = H._gen(*case, 7)
    imgs, base = {}, 0
    for name in PI_NAMES[:3 * nmod]:
        h = hs if name[0] == "s" else ht
        n = Bm * 3 * h * h
        imgs[name] = ((base + torch.arange(n)).float() if coded else torch.randn(n, generator=g) * 2).view(Bm, 3, h, h)
        base += n
    assert base < 2 ** 24
    return imgs


def pi_reference(case, imgs):
    """F.unfold of each image, rows (m * Bm + b) * ntok + tok with the tokens in the order template, online
    template, search, columns (c * P + ky) * P + kx."""
    Bm, ht, hs, patch, nmod = case
    seqs = []
    for m in range(nmod):
        toks = [F.unfold(imgs["%s%d" % (k, m)], patch, stride=patch).transpose(1, 2) for k in "tos"]
        seqs.append(torch.cat(toks, 1))                  # [Bm][ntok][3 P P]
    return torch.cat(seqs, 0).reshape(-1, 3 * patch * patch)


def restate_pi(case, imgs, mut=None):
    """The same gather by explicit indices.  Mutations: swap_to (template and online template exchanged), swap_kyx."""
    Bm, ht, hs, patch, nmod = case
    gt, gs = ht // patch, hs // patch
    nt, ntok = gt * gt, 2 * gt * gt + gs * gs
    out = torch.empty(nmod * Bm * ntok, 3 * patch * patch)
    col = torch.arange(3 * patch * patch)
    ch, ky, kx = col // (patch * patch), (col // patch) % patch, col % patch
    if mut == "swap_kyx":
        ky, kx = kx, ky
    order = "ots" if mut == "swap_to" else "tos"
    for m in range(nmod):
        for b in range(Bm):
            for tok in range(ntok):
                k, t, g = (order[0], tok, gt) if tok < nt else (order[1], tok - nt, gt) if tok < 2 * nt else (order[2], tok - 2 * nt, gs)
                img = imgs["%s%d" % (k, m)][b]
                out[(m * Bm + b) * ntok + tok] = img[ch, (t // g) * patch + ky, (t % g) * patch + kx]
    return out
