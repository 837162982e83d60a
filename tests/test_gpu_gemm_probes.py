"""mmt_gemm / mmt_gemm_multi against exact integer probes (tests/gemm_probes.py) on shapes derived from every
tile's edges: M and N one below, at and one above a tile, K tails of one chunk, K around the ring depth, odd
step counts under two k-groups, the smallest legal K split, row groups and grids of every remainder.

Every comparison but the folded LayerNorm's is bitwise: with operands in {-3, ..., 3} without 0 every partial
sum is an exact fp32 integer in any summation order, tile shape or split, so the expected C / C2 are known
bit for bit, the one rounding to bf16 / fp16 included.  All storage is oversized and poisoned with NaN and
compared whole: an element of the M x N region that was not written, a pitch column or surplus row that was,
or a surplus element that was read into a sum each fail the launch.  test_gemm_probes_host.py shows that every
case reaches the kernel it names with the K split it asks for, and that a dropped, doubled or misplaced
product changes the expected values."""
import pytest
import torch

import gemm_probes as P

pytestmark = pytest.mark.gpu


def _lib():
    from mmt_amd import _lib
    return _lib


_code = P.dtype_code


_WS = {}


def _workspace(s):
    """Split-K slabs (NaN: a slab element read before it was written shows) and zeroed tickets, kept per size."""
    if s.ws_floats not in _WS:
        _WS[s.ws_floats] = (torch.empty(s.ws_floats, device="cuda"), torch.zeros(s.cnt_n, device="cuda", dtype=torch.int32))
    ws, cnt = _WS[s.ws_floats]
    ws.fill_(P.NAN)
    return ws, cnt


def _prepare(prob):
    """Uploads a problem's storage and fills mmt_gemm_params; returns (params, device tensors to keep and check)."""
    s = prob.spec
    dev = {k: [t.cuda() for t in v] for k, v in prob.inp.items() if isinstance(v, list)}
    out = {k: [t.cuda() for t in v] for k, v in prob.out.items()}
    if s.splitk:
        dev["sk"] = _workspace(s)
    if s.row_scale_div:
        dev["row_scale"] = [prob.inp["row_scale"].cuda()]
    held = dict(dev, **out)
    if s.r_inplace:
        held["r"] = out["c"]
    ptrs = {k: [t.data_ptr() for t in v] for k, v in held.items()}
    return P.params_of(s, ptrs), dev, out


def _verify(prob, out, errors, tag=""):
    s = prob.spec
    for name, exp in prob.expect.items():
        for g, e in enumerate(exp):
            if not P.same(out[name][g], e.cuda()):
                errors.append("%s%s[%d] of %s: %s" % (tag, name, g, s, P.describe(out[name][g].cpu(), e)))


def _run(s, errors, repeats=1):
    """Launches spec s (`repeats` times, each on fresh outputs) and checks every output image."""
    L = _lib()
    prob = P.build(s)
    for rep in range(repeats):
        p, dev, out = _prepare(prob)
        L.check(L.LIB.mmt_gemm(p, _code(s.dtype), torch.cuda.current_stream().cuda_stream), "mmt_gemm %s" % (s,))
        _verify(prob, out, errors, "launch %d: " % rep if repeats > 1 else "")
        if s.splitk and int(dev["sk"][1].abs().sum()):
            errors.append("tickets not zero after %s" % (s,))
        torch.cuda.synchronize()
    del dev, out


def _report(errors, n):
    assert not errors, "%d of %d checks failed:\n%s" % (len(errors), n, "\n".join(errors[:6]))


SWEEP_IDS = [(d, i, e) for d, i in P.SWEEP for e in P.EPILOGUES if P.sweep_cases(d, i, e)]


@pytest.mark.parametrize("dname,impl,epi", SWEEP_IDS)
def test_edge_sweep(dname, impl, epi):
    """Two groups over edge_shapes(impl) per epilogue: general (bias + ReLU + fp32 R, fp32 C), compact (16-bit C),
    compact with the pre-activation copy, residual producer (fp32 C, 16-bit C2), the same with the LayerNorm row
    statistics (sums and sums of squares of the stored C2 per 64 columns, exact integers, compared for
    equality), and a 16-bit C with C2 = C + R, R in the compute dtype behind a modulo row map."""
    cases = P.sweep_cases(dname, impl, epi)
    errors = []
    for s in cases:
        _run(s, errors)
    _report(errors, len(cases))


@pytest.mark.parametrize("impl", P.SPLIT_IMPLS)
@pytest.mark.parametrize("nsk", range(2, 9))
def test_split_k(impl, nsk):
    """Every slice at its minimum (nsk * KS steps), one step more, a prime step count, a one-chunk K tail on the
    last slice; two groups, an in-place fp32 residual (C = R) and the C2 copy; the conv mode (K = 9 * 24) where
    its four steps hold the split.  Two launches each, both exact (so they repeat bitwise); tickets left zero;
    the slabs start as NaN."""
    cases = P.split_cases(impl, nsk)
    errors = []
    for s in cases:
        _run(s, errors, repeats=2)
    _report(errors, len(cases))


@pytest.mark.parametrize("impl", P.ROWMAP_IMPLS)
def test_row_maps(impl):
    """Segmented A rows (runs of 1, 7, BM + 1 rows, 3 per block, NaN rows between segments and blocks), a second K
    source from k = 8 / 72 / K - 8, the output row map with R read through it, the modulo and the conv residual maps."""
    cases = P.rowmap_cases(impl)
    errors = []
    for s in cases:
        _run(s, errors)
    _report(errors, len(cases))


@pytest.mark.parametrize("impl", P.MN_IMPLS)
@pytest.mark.parametrize("splitk", [0, 3])
def test_mn_major(impl, splitk):
    """w_t 1 (ldw > N), w_t 2 with c2_copy 3 / 4 (the ones column gives the exact column sums of A, columns 1..7
    of C2 exactly zero), a_t 1 (lda > M); K not a multiple of 64 (rows past K are NaN in storage and must read as
    zero).  impl 8's split equals impl 1's because both equal the integer reference."""
    cases = P.mn_cases(impl, splitk)
    errors = []
    for s in cases:
        _run(s, errors)
    _report(errors, len(cases))


@pytest.mark.parametrize("impl", P.CONV_IMPLS)
@pytest.mark.parametrize("dname", ["bf16", "f32"])
def test_conv(impl, dname):
    """Implicit-GEMM 1x1 / 3x3 / flipped 3x3 conv through the upsample map against float64 F.conv2d of the upsampled
    integer input: K = 72, 216, 648 (tails, a tap boundary inside a K-step), M across a tile edge, packed and
    padded image pitch (the padding pixels are NaN)."""
    cases = P.conv_cases(impl, dname)
    errors = []
    for s in cases:
        _run(s, errors)
    _report(errors, len(cases))


@pytest.mark.parametrize("impl", P.BIG_IMPLS)
@pytest.mark.parametrize("i", range(4))
def test_big_grid_tile_order(impl, i):
    """More than 512 workgroups with tiles_m 9 / 12 / 16 (the row-group tile order): every element written, with
    its own value, nothing else touched -- the order is a bijection."""
    errors = []
    _run(P.big_cases(impl)[i], errors)
    _report(errors, 1)


@pytest.mark.parametrize("impl", P.ROWSCALE_IMPLS)
def test_row_scale(impl):
    """row_scale in {0, 1, 2} with row_scale_div 1 / 7 / M: fp32 C with the 16-bit C2 copy, and a 16-bit C."""
    cases = P.rowscale_cases(impl)
    errors = []
    for s in cases:
        _run(s, errors)
    _report(errors, len(cases))


@pytest.mark.parametrize("mode", ["gemm", "conv"])
@pytest.mark.parametrize("impl", [1, 3, 0])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_gemm_multi(mode, impl, n):
    """1 to 4 problems of different shapes in one launch: each output exact, no problem's guard region touched."""
    L = _lib()
    probs = [P.build(s) for s in P.multi_cases(mode, impl, n)]
    held = [_prepare(pr) for pr in probs]
    arr = (L.GemmParams * n)(*[h[0] for h in held])
    L.check(L.LIB.mmt_gemm_multi(arr, n, _code("bf16"), torch.cuda.current_stream().cuda_stream), "mmt_gemm_multi")
    errors = []
    for i, (pr, h) in enumerate(zip(probs, held)):
        _verify(pr, h[2], errors, "problem %d: " % i)
    torch.cuda.synchronize()
    _report(errors, n)


LN_IDS = [(m, i) for m in (1, 2) for i in P.LN_IMPLS[m]]


@pytest.mark.parametrize("mode,impl", LN_IDS)
def test_layernorm_fold(mode, impl, capsys):
    """Linear(LayerNorm(x)) folded into the GEMM on rows of 1s and 3s (mean 2, variance 1, integer sums) against
    the float64 rstd * (acc - mu * colsum) + bias.  The inexact steps are 1 / K, the variance subtraction, the
    reciprocal square root, two multiplies and an add: the bar is 2^-19 = 1.9e-6 of max |ref| (16 fp32 ulps).
    Measured on an MI355X, the largest error over every impl and K: 7.5e-8 of max |ref| with the statistics summed
    in the K loop (ln_fold 1), 6.9e-8 with handed-in statistics (ln_fold 2) -- about half an fp32 ulp of the
    largest value, 25 times below the bar.  The guard storage must stay NaN."""
    L = _lib()
    worst = 0.0
    errors = []
    for s in P.ln_cases(impl, mode):
        prob = P.build_ln(s)
        p, dev, out = _prepare(prob)
        L.check(L.LIB.mmt_gemm(p, _code(s.dtype), torch.cuda.current_stream().cuda_stream), "mmt_gemm %s" % (s,))
        for g, e in enumerate(prob.expect["c"]):
            got = out["c"][g].cpu().double()
            region = ~torch.isnan(e)
            if not torch.equal(torch.isnan(got), ~region):
                errors.append("c[%d] of %s: %s" % (g, s, P.describe(got, e)))
                continue
            rel = ((got - e)[region].abs().max() / e[region].abs().max()).item()
            worst = max(worst, rel)
            if rel > P.LN_BAR:
                errors.append("c[%d] of %s: error %.3g of max |ref| over the bar %.3g" % (g, s, rel, P.LN_BAR))
    with capsys.disabled():
        print("\nln_fold %d impl %d: largest error %.3g of max |ref| (bar %.3g)" % (mode, impl, worst, P.LN_BAR))
    _report(errors, len(P.ln_cases(impl, mode)))
