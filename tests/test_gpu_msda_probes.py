"""The bimodal deformable attention against the probes of tests/msda_probes.py: mmt_msda_bimodal (fp32, bf16, fp16),
mmt_msda_bimodal_train_fwd / _bwd (separate buffers and one wider row), HipOps.msda_bimodal through autograd, and the
generic mmt_ms_deform_attn_forward / _backward_impl (fp32, the chunked and the per-level value gather) on the same
problems.

Exact families: every comparison is bitwise, on a NaN-guarded storage image compared whole (gemm_probes.same): an
element that should have been written and was not, and a gap, tail or surplus element that was, both fail.  Bar
families: elementwise against msda_probes.bar(ref, delta), delta from the oracle's own fp32 error; each test prints
its worst error as a fraction of its bar.  test_msda_probes_host.py shows that the references are exact and that one
dropped, displaced or mis-weighted term moves them."""
import pytest
import torch

import gemm_probes as P
import head_probes as H
import msda_probes as M

pytestmark = pytest.mark.gpu

F64, F32, BF16, F16 = M.F64, M.F32, M.BF16, M.F16
NAMES = {F32: "f32", BF16: "bf16", F16: "fp16"}


def _lib():
    from mmt_amd import _lib
    return _lib


def _code(dtype):
    L = _lib()
    return {F32: L.MMT_F32, BF16: L.MMT_BF16, F16: L.MMT_F16}[dtype]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _check(errors, what, got, want):
    """got (device) against a storage image `want` (host), every element, guards included."""
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


def _report(errors):
    assert not errors, "%d checks failed:\n%s" % (len(errors), "\n".join(errors[:8]))


# ------------------------------------------------------------------------------------------------ launches
def _train(pr, wide):
    """mmt_msda_bimodal_train_fwd and _bwd on NaN-poisoned outputs.  wide: offsets and logits in one row of M.WIDE
    bf16 (NaN in its gap and tail), and their gradients into one poisoned buffer of that shape.  -> (out, grad_value,
    grad_off, grad_awl) images; wide: grad_off is the whole wide buffer and grad_awl None."""
    L = _lib()
    ti = M.train_inputs(pr)
    B, hw, nq = pr["B"], pr["hw"], pr["nq"]
    rows = B * nq
    value, gout, ref = ti["value"].cuda(), ti["gout"].cuda(), ti["ref"].cuda()
    out, gv = H.poison(rows, M.CM, BF16).cuda(), H.poison(M.NL * rows, M.CM, BF16).cuda()
    if wide:
        ow = M.wide_rows(ti["off"], ti["awl"]).cuda()
        gow = H.poison(rows, M.WIDE, BF16).cuda()
        off_p, awl_p, pitch_o, pitch_a = ow.data_ptr(), ow.data_ptr() + 2 * M.WIDE_AWL, M.WIDE, M.WIDE
        goff_p, gawl_p = gow.data_ptr(), gow.data_ptr() + 2 * M.WIDE_AWL
        goff, gawl = gow, None
    else:
        off, awl = ti["off"].cuda(), ti["awl"].cuda()
        goff, gawl = H.poison(rows, 128, BF16).cuda(), H.poison(rows, 64, BF16).cuda()
        off_p, awl_p, pitch_o, pitch_a = off.data_ptr(), awl.data_ptr(), 128, 64
        goff_p, gawl_p = goff.data_ptr(), gawl.data_ptr()
    L.check(L.LIB.mmt_msda_bimodal_train_fwd(value.data_ptr(), off_p, pitch_o, awl_p, pitch_a, ref.data_ptr(),
                                             out.data_ptr(), B, hw, _st()), "mmt_msda_bimodal_train_fwd")
    L.check(L.LIB.mmt_msda_bimodal_train_bwd(value.data_ptr(), off_p, pitch_o, awl_p, pitch_a, ref.data_ptr(),
                                             gout.data_ptr(), gv.data_ptr(), goff_p, gawl_p, B, hw, _st()),
            "mmt_msda_bimodal_train_bwd")
    torch.cuda.synchronize()
    return out, gv, goff, gawl


def _infer(pr, dtype):
    L = _lib()
    value, offw = M.infer_inputs(pr, dtype)
    value, offw = value.cuda(), offw.cuda()
    out = H.poison(pr["B"] * pr["nq"], M.CM, dtype).cuda()
    L.check(L.LIB.mmt_msda_bimodal(offw.data_ptr(), value.data_ptr(), out.data_ptr(), pr["B"], pr["hw"], _code(dtype),
                                   _st()), "mmt_msda_bimodal")
    torch.cuda.synchronize()
    return out


def _generic(pr, value_impl):
    """mmt_ms_deform_attn_forward and _backward_impl in fp32 -> (out, grad_value, grad_loc, grad_attn) images."""
    L = _lib()
    gi = {k: v.cuda() for k, v in M.generic_inputs(pr).items()}
    B, hw, nq = pr["B"], pr["hw"], pr["nq"]
    rows = B * nq
    shapes = torch.tensor([[hw, hw]] * M.NL, dtype=torch.long).cuda()
    starts = (torch.arange(M.NL, dtype=torch.long) * nq).cuda()
    out, gv = H.poison(rows, M.CM, F32).cuda(), H.poison(M.NL * rows, M.CM, F32).cuda()
    gl, ga = H.poison(rows, 128, F32).cuda(), H.poison(rows, 64, F32).cuda()
    dims = (B, M.NL * nq, M.NH, M.DH, nq, M.NL, M.NP)
    L.check(L.LIB.mmt_ms_deform_attn_forward(gi["value"].data_ptr(), shapes.data_ptr(), starts.data_ptr(),
                                             gi["loc"].data_ptr(), gi["aw"].data_ptr(), out.data_ptr(), *dims, L.MMT_F32,
                                             _st()), "mmt_ms_deform_attn_forward")
    L.check(L.LIB.mmt_ms_deform_attn_backward_impl(gi["value"].data_ptr(), shapes.data_ptr(), starts.data_ptr(),
                                                   gi["loc"].data_ptr(), gi["aw"].data_ptr(), gi["gout"].data_ptr(),
                                                   gv.data_ptr(), gl.data_ptr(), ga.data_ptr(), *dims, nq, value_impl,
                                                   L.MMT_F32, _st()), "mmt_ms_deform_attn_backward_impl")
    torch.cuda.synchronize()
    return out, gv, gl, ga


def _train_images(pr, ref, wide):
    """The expected storage images of _train's outputs: the fp64 reference rounded once to bf16."""
    rows = pr["B"] * pr["nq"]
    e = {n: M.expected(ref[n], BF16) for n in M.OUTPUTS}
    out, gv = H.image(rows, M.CM, e["out"], BF16), H.image(M.NL * rows, M.CM, e["gv"], BF16)
    if wide:
        return out, gv, M.wide_rows(e["goff"].reshape(rows, 128), e["gawl"].reshape(rows, 64), guard=M.GUARD), None
    return out, gv, H.image(rows, 128, e["goff"], BF16), H.image(rows, 64, e["gawl"], BF16)


# ------------------------------------------------------------------------------------------------ exact families
@pytest.mark.parametrize("key", M.EXACT_KEYS, ids=M.key_id)
def test_train_entry_points_exact(key):
    """mmt_msda_bimodal_train_fwd: out; _bwd: grad_value (the bucketed gather), grad_off (the 8-lane channel sums)
    and grad_awl (the fused softmax backward), each equal to the fp64 reference rounded once, with separate buffers
    (pitches 128 / 64) and with one 208-column row whose gap and tail columns come back untouched."""
    pr, ref = M.problem(key), M.reference(key)
    errors = []
    for wide in (False, True):
        got, want = _train(pr, wide), _train_images(pr, ref, wide)
        names = ("out", "grad_value", "grad_off | grad_awl row" if wide else "grad_off", "grad_awl")
        for name, g, w in zip(names, got, want):
            if g is not None:
                _check(errors, "%s%s" % ("wide " if wide else "", name), g, w)
    _report(errors)


@pytest.mark.parametrize("key", M.EXACT_KEYS, ids=M.key_id)
def test_inference_exact(key):
    """mmt_msda_bimodal: in fp32 the reference itself, in bf16 and fp16 the reference rounded once."""
    pr, ref = M.problem(key), M.reference(key)
    rows = pr["B"] * pr["nq"]
    errors = []
    for dtype in (F32, BF16, F16):
        _check(errors, NAMES[dtype], _infer(pr, dtype), H.image(rows, M.CM, M.expected(ref["out"], dtype), dtype))
    _report(errors)


@pytest.mark.parametrize("key", M.EXACT_KEYS, ids=M.key_id)
def test_generic_op_exact(key):
    """mmt_ms_deform_attn_forward and _backward_impl (fp32) with the chunked (value_impl 1) and the per-level (2)
    value gather: the output and all three gradients equal the reference bit for bit."""
    pr, ref = M.problem(key), M.reference(key)
    rows = pr["B"] * pr["nq"]
    want = (H.image(rows, M.CM, ref["out"].float(), F32), H.image(M.NL * rows, M.CM, ref["gv"].float(), F32),
            H.image(rows, 128, ref["gl"].float(), F32), H.image(rows, 64, ref["ga"].float(), F32))
    errors = []
    for impl in (1, 2):
        for name, g, w in zip(("out", "grad_value", "grad_loc", "grad_attn"), _generic(pr, impl), want):
            _check(errors, "value_impl %d %s" % (impl, name), g, w)
    _report(errors)


def test_autograd_wiring_matches_the_direct_calls():
    """HipOps.msda_bimodal on a (B, nq, 192) offsets | logits tensor, forward and backward through autograd: the same
    bits as the direct calls, which are the reference rounded once."""
    from mmt_amd.train import HipOps
    key = ("blend", 8, 3, "")
    pr, ref = M.problem(key), M.reference(key)
    B, hw, nq = pr["B"], pr["hw"], pr["nq"]
    ti = M.train_inputs(pr)
    value = ti["value"].view(B, M.NL * nq, M.CM).cuda().requires_grad_(True)
    offw = torch.cat([ti["off"], ti["awl"]], 1).view(B, nq, 192).cuda().requires_grad_(True)
    t = torch.full((1 << 22,), M.NAN, device="cuda")  # NaN into the allocator's free blocks: the op's torch.empty outputs
    del t
    y = HipOps.msda_bimodal(value, offw, ti["ref"].cuda(), hw)
    y.backward(ti["gout"].view(B, nq, M.CM).cuda())
    torch.cuda.synchronize()
    direct = _train(pr, False)
    rows = B * nq
    errors = []
    got = (y.detach().reshape(rows, M.CM), value.grad.reshape(M.NL * rows, M.CM), offw.grad[..., :128].reshape(rows, 128),
           offw.grad[..., 128:].reshape(rows, 64))
    for name, g, d, n in zip(("out", "grad_value", "grad_off", "grad_awl"), got, direct, M.OUTPUTS):
        want = M.expected(ref[n], BF16).reshape(g.shape)
        _check(errors, "autograd " + name, g.contiguous(), want)
        _check(errors, "autograd against direct " + name, g.contiguous(), d[:g.shape[0]].cpu())
    _report(errors)


# ------------------------------------------------------------------------------------------------ bar families
@pytest.mark.parametrize("key", M.BAR_KEYS, ids=M.key_id)
def test_train_entry_points_within_bar(key):
    pr, ref, d = M.problem(key), M.reference(key), M.delta(key)
    rows = pr["B"] * pr["nq"]
    out, gv, goff, gawl = _train(pr, False)
    errors, worst = [], {}
    for name, n, g, r in (("out", "out", out, rows), ("grad_value", "gv", gv, M.NL * rows), ("grad_off", "goff", goff, rows),
                          ("grad_awl", "gawl", gawl, rows)):
        worst[name] = _check_bar(errors, name, g, r, ref[n], M.bar(ref[n], d[n], BF16))
    print("msda train %s: worst error / bar %s; delta %s" % (M.key_id(key), {k: "%.3f" % v for k, v in worst.items()},
                                                              {n: "%.3g" % d[n] for n in M.OUTPUTS}))
    _report(errors)


@pytest.mark.parametrize("key", M.BAR_KEYS, ids=M.key_id)
def test_inference_within_bar(key):
    pr, ref, d = M.problem(key), M.reference(key), M.delta(key)
    rows = pr["B"] * pr["nq"]
    errors, worst = [], {}
    for dtype in (F32, BF16, F16):
        worst[NAMES[dtype]] = _check_bar(errors, NAMES[dtype], _infer(pr, dtype), rows, ref["out"],
                                         M.bar(ref["out"], d["out"], dtype))
    print("msda inference %s: worst error / bar %s; delta %.3g" % (M.key_id(key), {k: "%.3f" % v for k, v in worst.items()},
                                                                   d["out"]))
    _report(errors)


def test_backward_is_deterministic():
    """Two runs of mmt_msda_bimodal_train_bwd on the hw = 22 collapse case (every list of the value gather full and
    long): identical bits."""
    pr = M.problem(("bar", 22, 2, "collapse"))
    a, b = _train(pr, False), _train(pr, False)
    for name, x, y in zip(("out", "grad_value", "grad_off", "grad_awl"), a, b):
        assert P.same(x.cpu(), y.cpu()), name
