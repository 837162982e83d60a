"""The kernels of csrc/norm.hip against the probes of tests/norm_probes.py, through the C ABI: mmt_layernorm,
mmt_layernorm_bwd / _bwd_add, mmt_groupnorm, mmt_groupnorm_bwd, mmt_add_cast, mmt_scale_rows_cast, mmt_patch_im2col.

Every output (workspaces included) is a NaN-filled storage image GUARD rows larger than the problem and is compared
whole: an element that should have been written and was not fails, and so does a guard element that was.  Inputs are
compared with their originals after the launch.  Bitwise families use gemm_probes.same; bar families are held
elementwise within a bar that comes from the float64 oracle alone (norm_probes.delta_of, msda_probes.bar) or from a
counted worst case (ln_dgamma_bar, gn_dgamma_bar), and print their worst error as a fraction of that bar.
test_norm_probes_host.py shows on the CPU that the bars can be met and that one planted defect passes them."""
import pytest
import torch

import gemm_probes as P
import head_probes as H
import norm_probes as N

pytestmark = pytest.mark.gpu

F64, F32, BF16, F16 = N.F64, N.F32, N.BF16, N.F16
GUARD = N.GUARD


def _lib():
    from mmt_amd import _lib
    return _lib


def _code(dtype):
    L = _lib()
    return {F32: L.MMT_F32, BF16: L.MMT_BF16, F16: L.MMT_F16}[dtype]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _check(errors, what, got, want):
    """got (device or host) against a storage image `want` (host), every element, guards included."""
    got = got.cpu()
    if got.shape != want.shape or got.dtype != want.dtype:
        errors.append("%s: %s %s, expected %s %s" % (what, got.dtype, tuple(got.shape), want.dtype, tuple(want.shape)))
    elif not P.same(got, want):
        errors.append("%s: %s" % (what, P.describe(got, want)))


def _check_bar(errors, what, got, rows, ref, bar):
    """The first `rows` rows of the image within `bar` of `ref` elementwise (a NaN fails), the guard rows still NaN;
    returns the worst |got - ref| / bar."""
    got = got.cpu()
    body = got[:rows].double().reshape(ref.shape)
    ratio = (body - ref).abs() / bar
    worst = float(ratio.max())
    bad = ~(ratio <= 1.0)
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        errors.append("%s: %.3g x the bar at %s (got %r, reference %r, bar %.3g)" %
                      (what, float(ratio[bad].nan_to_num(float("inf")).max()), i, body[i].item(), ref[i].item(), bar[i].item()))
        worst = float("inf")
    if not bool(torch.isnan(got[rows:]).all()):
        errors.append("%s: %d guard elements written" % (what, int((~torch.isnan(got[rows:])).sum())))
    return worst


def _unchanged(errors, pairs):
    for name, dev, host in pairs:
        if dev is not None:
            _check(errors, "input " + name, dev, host)


def _report(errors):
    assert not errors, "%d checks failed:\n%s" % (len(errors), "\n".join(errors[:8]))


def _fmt(worst):
    return {k: "%.3f" % v for k, v in worst.items()}


# ------------------------------------------------------------------------------------------------ layernorm
@pytest.mark.parametrize("c", N.LN_CASES, ids=N.ln_id)
def test_layernorm(c):
    """y within delta of the float64 oracle (fp32) and within the 16-bit bar (typed); where one launch writes both,
    the typed image is the fp32 image rounded once; in place, the input image becomes the output image."""
    L = _lib()
    pr = N.ln_problem(c)
    ref, d = N.ln_reference(c)
    dt = N.DT[c.dtype]
    inplace = c.out.startswith("inplace")
    x_h = H.image(c.rows, c.C, pr["x"], F32)
    x = x_h.cuda()
    hosts = {k: pr[k] for k in ("add", "g0", "b0")}
    if c.sets == "two":
        hosts.update(g1=pr["g1"], b1=pr["b1"])
    dev = {k: (None if v is None else v.cuda()) for k, v in hosts.items()}
    of = x if inplace else (H.poison(c.rows, c.C, F32).cuda() if c.has_f32 else None)
    ot = H.poison(c.rows, c.C, dt).cuda() if c.has_typed else None
    L.check(L.LIB.mmt_layernorm(x.data_ptr(), _ptr(dev["add"]), c.add_rows, _ptr(of), _ptr(ot), dev["g0"].data_ptr(),
                                dev["b0"].data_ptr(), _ptr(dev.get("g1")), _ptr(dev.get("b1")), c.rows, c.rpg_arg, c.C,
                                c.eps, _code(dt), _st()), "mmt_layernorm")
    torch.cuda.synchronize()
    errors, worst = [], {}
    if of is not None:
        worst["f32"] = _check_bar(errors, "out_f32", of, c.rows, ref, torch.full_like(ref, d))
    if ot is not None:
        worst[c.dtype] = _check_bar(errors, "out_t", ot, c.rows, ref, N.bar(ref, d, dt))
    if of is not None and ot is not None:
        _check(errors, "out_t against out_f32 rounded once", ot, of.cpu().to(dt))
    _unchanged(errors, [("x", None if inplace else x, x_h)] + [(k, dev[k], hosts[k]) for k in hosts])
    print("norm-probe layernorm %s: worst error / bar %s; delta %.3g" % (N.ln_id(c), _fmt(worst), d))
    _report(errors)


# ------------------------------------------------------------------------------------------------ layernorm backward
def _lnb_launch(c, pr, accumulate):
    """One launch on fresh images -> (dx, dgb, ws, inputs): dgb NaN (accumulate 0) or the integer prefill in its
    2 * sets rows; dres == dx: the dx image starts as dres."""
    L = _lib()
    dt = N.DT[c.dtype]
    x, dy = H.image(c.rows, c.C, pr["x"], F32).cuda(), H.image(c.rows, c.C, pr["dy"], dt).cuda()
    g0 = pr["g0"].cuda()
    g1 = pr["g1"].cuda() if c.rpg else None
    dres = H.image(c.rows, c.C, pr["dres"], F32).cuda() if c.dres == "separate" else None
    dx = H.image(c.rows, c.C, pr["dres"], F32).cuda() if c.dres == "alias" else H.poison(c.rows, c.C, F32).cuda()
    dgb_h = H.poison(4, c.C, F32)
    if accumulate:
        dgb_h[:2 * c.sets] = pr["prefill"][:2 * c.sets]
    dgb = dgb_h.cuda()
    ws = H.poison(c.nwg * 4, c.C, F32).cuda()
    ws_floats = c.nwg * 4 * c.C
    if c.dres == "none":
        rc = L.LIB.mmt_layernorm_bwd(x.data_ptr(), dy.data_ptr(), _code(dt), g0.data_ptr(), _ptr(g1), dx.data_ptr(),
                                     dgb.data_ptr(), accumulate, ws.data_ptr(), ws_floats, c.rows, c.rpg, c.C, c.eps, _st())
    else:
        rc = L.LIB.mmt_layernorm_bwd_add(x.data_ptr(), dy.data_ptr(), _code(dt), g0.data_ptr(), _ptr(g1),
                                         dx.data_ptr() if c.dres == "alias" else dres.data_ptr(), dx.data_ptr(),
                                         dgb.data_ptr(), accumulate, ws.data_ptr(), ws_floats, c.rows, c.rpg, c.C, c.eps,
                                         _st())
    L.check(rc, "mmt_layernorm_bwd")
    torch.cuda.synchronize()
    return dx, dgb, ws, dict(x=x, dy=dy, g0=g0, g1=g1, dres=dres)


@pytest.mark.parametrize("c", N.LNB_CASES, ids=N.lnb_id)
def test_layernorm_backward(c):
    """dgb_accumulate 0 over a NaN-filled dgb, then 1 over an integer prefill: dx within delta both times and equal
    bit for bit; dbeta the exact integer sums; dgamma within its counted bar; the accumulated image equal to prefill
    + the first launch's in fp32; the workspace written whole, its dbeta partials exact, nothing behind it."""
    pr, ref = N.lnb_problem(c), N.lnb_reference(c)
    dt = N.DT[c.dtype]
    n = 2 * c.sets
    errors, worst = [], {}
    dx0, dgb0, ws0, in0 = _lnb_launch(c, pr, 0)
    dx1, dgb1, ws1, _ = _lnb_launch(c, pr, 1)
    worst["dx"] = _check_bar(errors, "dx", dx0, c.rows, ref["dx"], torch.full_like(ref["dx"], ref["delta"]))
    _check(errors, "dx of the second launch", dx1, dx0.cpu())
    g0 = dgb0.cpu()
    _check(errors, "dbeta", g0[1:n:2], ref["dgb"][1::2].float())
    live = ref["dgamma_bar"] > 0    # a set without rows: dgamma is exactly 0
    ratio = (g0[0:n:2].double() - ref["dgb"][0::2]).abs() / ref["dgamma_bar"].clamp(min=1e-300)
    if not bool((ratio[live] <= 1.0).all()) or not bool((g0[0:n:2][~live] == 0).all()):
        errors.append("dgamma: %.3g x the bar" % float(ratio[live].nan_to_num(float("inf")).max()))
    worst["dgamma"] = float(ratio[live].max()) if bool(live.any()) else 0.0
    if not bool(torch.isnan(g0[n:]).all()):
        errors.append("dgb: %d elements written behind the %d rows" % (int((~torch.isnan(g0[n:])).sum()), n))
    want1 = H.poison(4, c.C, F32)
    want1[:n] = pr["prefill"][:n] + g0[:n]
    _check(errors, "dgb accumulated", dgb1, want1)
    w0 = ws0.cpu()
    part = w0[:c.nwg * 4].view(c.nwg, 4, c.C)
    _check(errors, "workspace dbeta partials", part[:, 1::2], ref["dbeta_part"].float())
    if bool(torch.isnan(w0[:c.nwg * 4]).any()) or not bool(torch.isnan(w0[c.nwg * 4:]).all()):
        errors.append("workspace: %d NaN inside, %d elements written behind nwg * 4 * C floats" %
                      (int(torch.isnan(w0[:c.nwg * 4]).sum()), int((~torch.isnan(w0[c.nwg * 4:])).sum())))
    _check(errors, "workspace of the second launch", ws1, w0)
    _unchanged(errors, [("x", in0["x"], H.image(c.rows, c.C, pr["x"], F32)), ("dy", in0["dy"], H.image(c.rows, c.C, pr["dy"], dt)),
                        ("gamma0", in0["g0"], pr["g0"]), ("gamma1", in0["g1"], pr["g1"]),
                        ("dres", in0["dres"], None if in0["dres"] is None else H.image(c.rows, c.C, pr["dres"], F32))])
    print("norm-probe layernorm_bwd %s: worst error / bar %s; delta %.3g" % (N.lnb_id(c), _fmt(worst), ref["delta"]))
    _report(errors)


# ------------------------------------------------------------------------------------------------ groupnorm
@pytest.mark.parametrize("c", N.GN_CASES, ids=N.gn_id)
def test_groupnorm(c):
    L = _lib()
    pr = N.gn_problem(c)
    ref, d = N.gn_reference(c)
    dt = N.DT[c.dtype]
    rows = c.n_inst * c.P
    ref = ref.reshape(rows, c.Ctot)
    x_h = H.image(rows, c.Ctot, pr["x"], F32)
    x = x_h.cuda()
    hosts = {k: pr[k] for k in (("g0", "b0", "g1", "b1") if c.two else ("g0", "b0"))}
    dev = {k: v.cuda() for k, v in hosts.items()}
    of = H.poison(rows, c.Ctot, F32).cuda() if c.has_f32 else None
    ot = H.poison(rows, c.Ctot, dt).cuda() if c.has_typed else None
    L.check(L.LIB.mmt_groupnorm(x.data_ptr(), _ptr(of), _ptr(ot), dev["g0"].data_ptr(), dev["b0"].data_ptr(),
                                _ptr(dev.get("g1")), _ptr(dev.get("b1")), c.n_inst, c.ips, c.P, c.Ctot, c.groups, c.eps,
                                _code(dt), _st()), "mmt_groupnorm")
    torch.cuda.synchronize()
    errors, worst = [], {}
    if of is not None:
        worst["f32"] = _check_bar(errors, "out_f32", of, rows, ref, torch.full_like(ref, d))
    if ot is not None:
        worst[c.dtype] = _check_bar(errors, "out_t", ot, rows, ref, N.bar(ref, d, dt))
    if of is not None and ot is not None:
        _check(errors, "out_t against out_f32 rounded once", ot, of.cpu().to(dt))
    _unchanged(errors, [("x", x, x_h)] + [(k, dev[k], hosts[k]) for k in hosts])
    print("norm-probe groupnorm %s: worst error / bar %s; delta %.3g" % (N.gn_id(c), _fmt(worst), d))
    _report(errors)


def _gnb_launch(c, pr, accumulate):
    L = _lib()
    rows = c.n_inst * c.P
    x, dy = H.image(rows, c.Ctot, pr["x"], F32).cuda(), H.image(rows, c.Ctot, pr["dy"], F32).cuda()
    gamma = pr["gamma"].cuda()
    dx = H.poison(rows, c.Ctot, F32).cuda()
    dgb_h = H.poison(2, c.Ctot, F32)
    if accumulate:
        dgb_h[:2] = pr["prefill"]
    dgb = dgb_h.cuda()
    ws = H.poison(c.n_inst * 2, c.Ctot, F32).cuda()
    L.check(L.LIB.mmt_groupnorm_bwd(x.data_ptr(), dy.data_ptr(), gamma.data_ptr(), dx.data_ptr(), dgb.data_ptr(), accumulate,
                                    ws.data_ptr(), c.n_inst * 2 * c.Ctot, c.n_inst, c.P, c.Ctot, c.groups, c.eps, _st()),
            "mmt_groupnorm_bwd")
    torch.cuda.synchronize()
    return dx, dgb, ws, dict(x=x, dy=dy, gamma=gamma)


@pytest.mark.parametrize("c", N.GNB_CASES, ids=N.gnb_id)
def test_groupnorm_backward(c):
    """As test_layernorm_backward: two launches (overwrite over NaN, accumulate over integers), dx within delta and
    repeatable, dbeta exact, dgamma within its counted bar, the workspace [n_inst][2][Ctot] written whole."""
    pr, ref = N.gnb_problem(c), N.gnb_reference(c)
    rows = c.n_inst * c.P
    errors, worst = [], {}
    dx0, dgb0, ws0, in0 = _gnb_launch(c, pr, 0)
    dx1, dgb1, ws1, _ = _gnb_launch(c, pr, 1)
    rdx = ref["dx"].reshape(rows, c.Ctot)
    worst["dx"] = _check_bar(errors, "dx", dx0, rows, rdx, torch.full_like(rdx, ref["delta"]))
    _check(errors, "dx of the second launch", dx1, dx0.cpu())
    g0 = dgb0.cpu()
    _check(errors, "dbeta", g0[1], ref["dgb"][1].float())
    worst["dgamma"] = _check_bar(errors, "dgamma", g0[0:1], 1, ref["dgb"][0:1], ref["dgamma_bar"][None])
    if not bool(torch.isnan(g0[2:]).all()):
        errors.append("dgb: %d elements written behind its 2 rows" % int((~torch.isnan(g0[2:])).sum()))
    want1 = H.poison(2, c.Ctot, F32)
    want1[:2] = pr["prefill"] + g0[:2]
    _check(errors, "dgb accumulated", dgb1, want1)
    w0 = ws0.cpu()
    _check(errors, "workspace dbeta partials", w0[:2 * c.n_inst].view(c.n_inst, 2, c.Ctot)[:, 1], ref["dbeta_part"].float())
    if bool(torch.isnan(w0[:2 * c.n_inst]).any()) or not bool(torch.isnan(w0[2 * c.n_inst:]).all()):
        errors.append("workspace: %d NaN inside, %d elements written behind n_inst * 2 * Ctot floats" %
                      (int(torch.isnan(w0[:2 * c.n_inst]).sum()), int((~torch.isnan(w0[2 * c.n_inst:])).sum())))
    _check(errors, "workspace of the second launch", ws1, w0)
    _unchanged(errors, [("x", in0["x"], H.image(rows, c.Ctot, pr["x"], F32)), ("dy", in0["dy"], H.image(rows, c.Ctot, pr["dy"], F32)),
                        ("gamma", in0["gamma"], pr["gamma"])])
    print("norm-probe groupnorm_bwd %s: worst error / bar %s; delta %.3g" % (N.gnb_id(c), _fmt(worst), ref["delta"]))
    _report(errors)


# ------------------------------------------------------------------------------------------------ staging (bitwise)
@pytest.mark.parametrize("c", N.AC_CASES, ids=N.ac_id)
def test_add_cast(c):
    """(in + add[i % add_n]) in fp32, cast once: bit for bit, rounding ties, the fp16 overflow threshold and fp16
    subnormals included."""
    L = _lib()
    pr = N.ac_problem(c)
    dt = N.DT[c.dtype]
    x_h = H.image(c.n, 1, pr["x"], F32)
    x = x_h.cuda()
    add = None if pr["add"] is None else pr["add"].cuda()
    of = H.poison(c.n, 1, F32).cuda() if c.out != "typed" else None
    ot = H.poison(c.n, 1, dt).cuda() if c.out != "f32" else None
    L.check(L.LIB.mmt_add_cast(x.data_ptr(), _ptr(add), c.add_n, _ptr(of), _ptr(ot), c.n, _code(dt), _st()), "mmt_add_cast")
    torch.cuda.synchronize()
    errors = []
    if of is not None:
        _check(errors, "out_f32", of, H.image(c.n, 1, pr["want"], F32))
    if ot is not None:
        _check(errors, "out_t", ot, H.image(c.n, 1, pr["want"].to(dt), dt))
    _unchanged(errors, [("in", x, x_h), ("add", add, pr["add"])])
    _report(errors)


@pytest.mark.parametrize("case", N.SR_CASES, ids=lambda s: "r%d-c%d-per%d-%s" % s)
def test_scale_rows_cast(case):
    L = _lib()
    rows, cols, rows_per, dname = case
    pr = N.sr_problem(case)
    dt = N.DT[dname]
    x_h = H.image(rows, cols, pr["x"], F32)
    x, scale = x_h.cuda(), pr["scale"].cuda()
    out = H.poison(rows, cols, dt).cuda()
    L.check(L.LIB.mmt_scale_rows_cast(x.data_ptr(), scale.data_ptr(), rows_per, out.data_ptr(), rows, cols, _code(dt), _st()),
            "mmt_scale_rows_cast")
    torch.cuda.synchronize()
    errors = []
    _check(errors, "out", out, H.image(rows, cols, pr["want"].to(dt), dt))
    _unchanged(errors, [("in", x, x_h), ("scale", scale, pr["scale"])])
    _report(errors)


def test_scale_rows_cast_has_no_fp32_form():
    L = _lib()
    pr = N.sr_problem(N.SR_CASES[2])
    x, scale = pr["x"].cuda(), pr["scale"].cuda()
    out = H.poison(x.shape[0], x.shape[1], F32).cuda()
    rc = L.LIB.mmt_scale_rows_cast(x.data_ptr(), scale.data_ptr(), 1, out.data_ptr(), x.shape[0], x.shape[1], L.MMT_F32, _st())
    torch.cuda.synchronize()
    assert rc == N.EBADARG and bool(torch.isnan(out).all())


@pytest.mark.parametrize("dname", N.DTYPES)
@pytest.mark.parametrize("case", N.PI_CASES, ids=lambda s: "Bm%d-ht%d-hs%d-p%d-m%d" % s)
def test_patch_im2col(case, dname):
    """Row (m * Bm + b) * ntok + tok, tokens template | online template | search, column (c * P + ky) * P + kx: fp32
    moves distinct integer codes, the 16-bit types random values cast once."""
    L = _lib()
    Bm, ht, hs, patch, nmod = case
    dt = N.DT[dname]
    imgs = N.pi_problem(case, dt == F32)
    want = N.pi_reference(case, imgs)
    dev = {k: v.cuda() for k, v in imgs.items()}
    out = H.poison(want.shape[0], want.shape[1], dt).cuda()
    L.check(L.LIB.mmt_patch_im2col(dev["t0"].data_ptr(), _ptr(dev.get("t1")), dev["o0"].data_ptr(), _ptr(dev.get("o1")),
                                   dev["s0"].data_ptr(), _ptr(dev.get("s1")), out.data_ptr(), Bm, ht, hs, patch, _code(dt),
                                   _st()), "mmt_patch_im2col")
    torch.cuda.synchronize()
    errors = []
    _check(errors, "out", out, H.image(want.shape[0], want.shape[1], want.to(dt), dt))
    _unchanged(errors, [(k, dev[k], imgs[k]) for k in imgs])
    _report(errors)
