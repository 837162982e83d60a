"""The training step's glue kernels against the probes of tests/train_glue_probes.py, through the C ABI: the eight
entry points of csrc/fusion_train.hip, mmt_box_loss / _bwd (csrc/loss.hip) and mmt_adamw_step (csrc/optim.hip).

Every output (workspaces included) is a NaN-filled storage image GUARD rows or elements larger than the problem and
is compared whole; inputs are compared with their originals after the launch.  Bitwise families use
gemm_probes.same: all of fusion_train.hip (a CPU restatement predicts the bits, the keep factors from the numpy
restatement of the counter hash), the box loss on dyadic boxes, and AdamW's census / moments / norm families.  Bar
families: the box loss on random boxes (per-sample rows of dpred and the scalars within 4x the CPU float32 error of
the same composition) and the AdamW update on N(0, 1) data (p, m, v within a counted number of fp32 roundings of the
float64 formula evaluated on the device's own clip factor and bias corrections); both print their worst error as a
fraction of the bar.  test_train_glue_probes_host.py shows on the CPU that the bars can be met and that the planted
defects fail these comparisons.

AdamW update, misaligned layouts: each step is checked from the device's own previous step (so one step's bar
applies), and p, m, v and the shadow equal the aligned run bit for bit wherever the clip factor has the aligned run's
bits -- always without clipping and whenever g keeps its alignment; with g misaligned the norm's scalar loop adds in
another order, the factor may differ in its last bit, and the run is held to the bars alone."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gemm_probes as P
import head_probes as H
import train_glue_probes as A

pytestmark = pytest.mark.gpu

F64, F32, BF16 = A.F64, A.F32, A.BF16
GUARD = A.GUARD


def _lib():
    from mmt_amd import _lib
    return _lib


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


def _unchanged(errors, pairs):
    for name, dev, host in pairs:
        if dev is not None:
            _check(errors, "input " + name, dev, host)


def _report(errors):
    assert not errors, "%d checks failed:\n%s" % (len(errors), "\n".join(errors[:8]))


def _img(t, width, dtype):
    return H.image(t.numel() // width, width, t, dtype)


def _shape_id(s):
    return "x".join(str(v) for v in s)


# ------------------------------------------------------------------------------------------------ query_prep
@pytest.mark.parametrize("family", A.QP_FAMILIES)
@pytest.mark.parametrize("shape", A.QP_SHAPES, ids=_shape_id)
def test_query_prep(shape, family):
    """qbi[b][q][h][c] = bf16(src[b][h][q][c] + lpos[h][q][c]) and srcb = bf16(src), bit for bit."""
    L = _lib()
    B, nq, d = shape
    pr = A.qp_problem(shape, family)
    want_q, want_s = A.qp_expected(pr)
    src_h, lpos_h = _img(pr["src"], d, F32), _img(pr["lpos"], d, F32)
    src, lpos = src_h.cuda(), lpos_h.cuda()
    qbi, srcb = H.poison(B * nq, 2 * d, BF16).cuda(), H.poison(B * 2 * nq, d, BF16).cuda()
    L.check(L.LIB.mmt_ft_query_prep(src.data_ptr(), lpos.data_ptr(), qbi.data_ptr(), srcb.data_ptr(), B, nq, d, _st()),
            "mmt_ft_query_prep")
    torch.cuda.synchronize()
    errors = []
    _check(errors, "qbi", qbi, _img(want_q, 2 * d, BF16))
    _check(errors, "srcb", srcb, _img(want_s, d, BF16))
    _unchanged(errors, [("src", src, src_h), ("lpos", lpos, lpos_h)])
    _report(errors)


@pytest.mark.parametrize("through", (True, False), ids=("through", "nothrough"))
@pytest.mark.parametrize("family", A.QP_FAMILIES)
@pytest.mark.parametrize("shape", A.QPB_SHAPES, ids=_shape_id)
def test_query_prep_backward(shape, family, through):
    """dsrc = (dthrough + unshuffle(dqbi)) + dsrcb with and without dthrough; dlpos the samples' fp32 sum in batch
    order."""
    L = _lib()
    B, nq, d = shape
    pr = A.qpb_problem(shape, family)
    want_dsrc, want_dlpos = A.qpb_expected(pr, through)
    hosts = dict(dqbi=_img(pr["dqbi"], 2 * d, BF16), dsrcb=_img(pr["dsrcb"], d, BF16))
    if through:
        hosts["dthrough"] = _img(pr["dthrough"], d, F32)
    dev = {k: v.cuda() for k, v in hosts.items()}
    dsrc, dlpos = H.poison(B * 2 * nq, d, F32).cuda(), H.poison(2 * nq, d, F32).cuda()
    L.check(L.LIB.mmt_ft_query_prep_bwd(dev["dqbi"].data_ptr(), dev["dsrcb"].data_ptr(), _ptr(dev.get("dthrough")),
                                        dsrc.data_ptr(), dlpos.data_ptr(), B, nq, d, _st()), "mmt_ft_query_prep_bwd")
    torch.cuda.synchronize()
    errors = []
    _check(errors, "dsrc", dsrc, _img(want_dsrc, d, F32))
    _check(errors, "dlpos", dlpos, _img(want_dlpos, d, F32))
    _unchanged(errors, [(k, dev[k], hosts[k]) for k in hosts])
    _report(errors)


# ------------------------------------------------------------------------------------------------ drop_residual
@pytest.mark.parametrize("case", A.DR_CASES, ids=A.dr_id)
def test_drop_residual_and_backward(case):
    """out = x + bf16(y * k) and dy = bf16(sum over the halves of bf16(bf16(dout) * k)): the keep factor of every
    element is the hash restatement's draw at out's flat index, forward and backward alike."""
    L = _lib()
    shape, dup, dr = case
    B, rows, d = shape
    yrows = rows // 2 if dup else rows
    pr = A.dr_problem(shape, dup)
    hosts = dict(x=_img(pr["x"], d, F32), y=_img(pr["y"], d, BF16), dout=_img(pr["dout"], d, F32), rng=A.rng_state(dr))
    dev = {k: (None if v is None else v.cuda()) for k, v in hosts.items()}
    out, dy = H.poison(B * rows, d, F32).cuda(), H.poison(B * yrows, d, BF16).cuda()
    L.check(L.LIB.mmt_ft_drop_residual(dev["x"].data_ptr(), dev["y"].data_ptr(), out.data_ptr(), _ptr(dev["rng"]), dr.salt,
                                       dr.p, B, rows, d, dup, _st()), "mmt_ft_drop_residual")
    L.check(L.LIB.mmt_ft_drop_residual_bwd(dev["dout"].data_ptr(), dy.data_ptr(), _ptr(dev["rng"]), dr.salt, dr.p, B, rows,
                                           d, dup, _st()), "mmt_ft_drop_residual_bwd")
    torch.cuda.synchronize()
    errors = []
    _check(errors, "out", out, _img(A.dr_expected(pr, dup, dr), d, F32))
    _check(errors, "dy", dy, _img(A.drb_expected(pr, dup, dr), d, BF16))
    _unchanged(errors, [(k, dev[k], hosts[k]) for k in hosts])
    _report(errors)


# ------------------------------------------------------------------------------------------------ relu_drop
@pytest.mark.parametrize("dr", A.RDB_DROPS, ids=lambda dr: dr.name)
@pytest.mark.parametrize("n", A.RD_NS)
def test_relu_drop_and_backward(n, dr):
    """out = bf16(h * k); dh = (h > 0) ? bf16(dy * k) : 0.  Without dropout (p = 0 or no rng) the forward refuses
    and writes nothing; the backward is the plain ReLU backward."""
    L = _lib()
    pr = A.rd_problem(n)
    hosts = dict(h=_img(pr["h"], 8, BF16), dy=_img(pr["dy"], 8, BF16), rng=A.rng_state(dr))
    dev = {k: (None if v is None else v.cuda()) for k, v in hosts.items()}
    out, dh = H.poison(n // 8, 8, BF16).cuda(), H.poison(n // 8, 8, BF16).cuda()
    rc = L.LIB.mmt_ft_relu_drop(dev["h"].data_ptr(), out.data_ptr(), _ptr(dev["rng"]), dr.salt, dr.p, n, _st())
    L.check(L.LIB.mmt_ft_relu_drop_bwd(dev["dy"].data_ptr(), dev["h"].data_ptr(), dh.data_ptr(), _ptr(dev["rng"]), dr.salt,
                                       dr.p, n, _st()), "mmt_ft_relu_drop_bwd")
    torch.cuda.synchronize()
    errors = []
    if A.drop_params(dr.p, dr.rng)[0]:
        L.check(rc, "mmt_ft_relu_drop")
        _check(errors, "out", out, _img(A.rd_expected(pr, dr), 8, BF16))
    else:
        assert rc == A.EBADARG
        _check(errors, "out of the refused call", out, H.poison(n // 8, 8, BF16))
    _check(errors, "dh", dh, _img(A.rdb_expected(pr, dr), 8, BF16))
    _unchanged(errors, [(k, dev[k], hosts[k]) for k in hosts])
    _report(errors)


# ------------------------------------------------------------------------------------------------ rows_cast
@pytest.mark.parametrize("case", A.RC_CASES, ids=_shape_id)
def test_rows_cast_and_backward(case):
    """out = bf16 of the window's rows; dx = dout on the window, zeros written on every other row, nothing behind."""
    L = _lib()
    S, rows, row0, nrows, C = case
    pr = A.rc_problem(case)
    want_out, want_dx = A.rc_expected(case, pr)
    hosts = dict(x=_img(pr["x"], C, F32), dout=_img(pr["dout"], C, BF16))
    dev = {k: v.cuda() for k, v in hosts.items()}
    out, dx = H.poison(S * nrows, C, BF16).cuda(), H.poison(S * rows, C, F32).cuda()
    L.check(L.LIB.mmt_ft_rows_cast(dev["x"].data_ptr(), out.data_ptr(), S, rows, row0, nrows, C, _st()), "mmt_ft_rows_cast")
    L.check(L.LIB.mmt_ft_rows_cast_bwd(dev["dout"].data_ptr(), dx.data_ptr(), S, rows, row0, nrows, C, _st()),
            "mmt_ft_rows_cast_bwd")
    torch.cuda.synchronize()
    errors = []
    _check(errors, "out", out, _img(want_out, C, BF16))
    _check(errors, "dx", dx, _img(want_dx, C, F32))
    _unchanged(errors, [(k, dev[k], hosts[k]) for k in hosts])
    _report(errors)


# ------------------------------------------------------------------------------------------------ box loss
def _loss_launch(pred, gt):
    """mmt_box_loss and _bwd on fp32 images of the float64 operands -> (out image, dpred image, errors)."""
    L = _lib()
    B = pred.shape[0]
    hosts = dict(pred=H.image(B, 4, pred, F32), gt=H.image(B, 4, gt, F32), dloss=torch.tensor([A.LOSS_DLOSS], dtype=F32))
    dev = {k: v.cuda() for k, v in hosts.items()}
    out, dpred = H.poison(4, 1, F32).cuda(), H.poison(B, 4, F32).cuda()
    L.check(L.LIB.mmt_box_loss(dev["pred"].data_ptr(), dev["gt"].data_ptr(), out.data_ptr(), B, A.LOSS_W[0], A.LOSS_W[1],
                               _st()), "mmt_box_loss")
    L.check(L.LIB.mmt_box_loss_bwd(dev["pred"].data_ptr(), dev["gt"].data_ptr(), dev["dloss"].data_ptr(), dpred.data_ptr(), B,
                                   A.LOSS_W[0], A.LOSS_W[1], _st()), "mmt_box_loss_bwd")
    torch.cuda.synchronize()
    errors = []
    for k in hosts:
        if not P.same(dev[k].cpu(), hosts[k]):  # NaN operands compare as the same NaN
            errors.append("input %s changed" % k)
    return out.cpu(), dpred.cpu(), errors


@pytest.mark.parametrize("B", A.LOSS_EXACT_BS)
def test_box_loss_exact(B):
    """Dyadic boxes of every category: the loss, the three statistics and every row of dpred equal the float64
    reference bit for bit (B = 512: the strided sample loop and the backward's second workgroup)."""
    pred, gt, ref_out, ref_d = A.loss_reference("exact", B)
    out, dpred, errors = _loss_launch(pred, gt)
    _check(errors, "out", out, H.image(4, 1, ref_out, F32))
    _check(errors, "dpred", dpred, H.image(B, 4, ref_d, F32))
    _report(errors)


@pytest.mark.parametrize("B", A.LOSS_BAR_BS)
def test_box_loss_random(B):
    """Random boxes: every sample's dpred row and the four scalars within 4x the CPU float32 error against float64."""
    pred, gt, ref_out, ref_d = A.loss_reference("random", B)
    out, dpred, errors = _loss_launch(pred, gt)
    row = A.loss_row_err(dpred[:B], ref_d) if not bool(torch.isnan(dpred[:B]).any()) else float("inf")
    sc = A.loss_scalar_err(out[:4, 0], ref_out) if not bool(torch.isnan(out[:4]).any()) else float("inf")
    print("train-glue box_loss B%d: worst row error / bar %.3f, worst scalar error / bar %.3f" %
          (B, row / A.LOSS_ROW_BAR, sc / A.LOSS_SCALAR_BAR))
    if not row <= A.LOSS_ROW_BAR:
        errors.append("dpred: worst row %.3g, bar %.3g" % (row, A.LOSS_ROW_BAR))
    if not sc <= A.LOSS_SCALAR_BAR:
        errors.append("scalars: %s against %s, bar %.3g" % (out[:4, 0].tolist(), ref_out.tolist(), A.LOSS_SCALAR_BAR))
    if not bool(torch.isnan(out[4:]).all()) or not bool(torch.isnan(dpred[B:]).all()):
        errors.append("guard elements written")
    _report(errors)


def test_box_loss_nan_stays_in_its_sample():
    """Identical boxes give the reference's NaN (alpha = 0 / 0).  A NaN or an inf in one sample's pred makes the loss
    NaN and leaves every other sample's dpred row as it is when that sample is a finite box."""
    pred, gt, _, ref_d = A.loss_reference("exact", 256)
    errors = []
    same_gt = torch.tensor([[0.25, 0.25, 0.5, 0.5]], dtype=F64)
    out, _, errs = _loss_launch(torch.tensor([[0.5, 0.5, 0.5, 0.5]], dtype=F64), same_gt)
    errors += errs
    if not bool(torch.isnan(out[0])):
        errors.append("identical boxes: loss %r" % out[0].item())
    k = 100
    for col, val in ((0, float("nan")), (2, float("inf")), (1, float("-inf"))):
        bad = pred.clone()
        bad[k, col] = val
        out, dpred, errs = _loss_launch(bad, gt)
        errors += errs
        if not bool(torch.isnan(out[0])):
            errors.append("pred[%d][%d] = %r: loss %r" % (k, col, val, out[0].item()))
        want = H.image(256, 4, ref_d, F32)
        dpred[k], want[k] = 0.0, 0.0   # the bad sample's own row is not held to anything
        _check(errors, "dpred beside the bad sample (pred[%d][%d] = %r)" % (k, col, val), dpred, want)
    _report(errors)


# ------------------------------------------------------------------------------------------------ AdamW
class _AdamW:
    """One problem on the device: p, g, m, v and the shadow carved out of NaN-filled buffers at the layout's
    (mis)alignments, the tables built as HipAdamW._tables builds them, the 32-byte state zeroed."""

    def __init__(self, family, layout, hp):
        from mmt_amd.optim import CHUNK_DTYPE, TENSOR_DTYPE
        pr = A.aw_problem(family)
        self.layout, self.hp = layout, hp
        self.buf = {k: A.aw_image(pr[k], layout, k, F32).cuda() for k in "pgmv"}
        self.buf["shadow"] = A.aw_image(None, layout, "shadow", BF16).cuda()
        size = {"p": 4, "g": 4, "m": 4, "v": 4, "shadow": 2}
        addr = {k: [self.buf[k].data_ptr() + size[k] * s for s in A.aw_starts(layout, k)[0]] for k in size}
        for k in size:
            assert self.buf[k].data_ptr() % 16 == 0
        t = np.zeros(len(A.AW_SIZES), TENSOR_DTYPE)
        for i, n in enumerate(A.AW_SIZES):
            t[i] = (addr["p"][i], addr["g"][i], addr["m"][i], addr["v"][i], 0 if i in A.AW_NO_SHADOW else addr["shadow"][i],
                    n, A.AW_GROUPS[i], 0)
        chunks = np.array([(i, 0, o) for i, o, _ in A.aw_chunks()], CHUNK_DTYPE)
        self.tables = [torch.from_numpy(a.view(np.uint8).copy()) for a in (t, chunks)]
        self.tens, self.chunks = (a.cuda() for a in self.tables)
        self.nchunks = len(chunks)
        self.state_h = torch.cat([torch.zeros(8), torch.full((GUARD,), A.NAN)])
        self.state = self.state_h.cuda()
        self.partial = torch.full((self.nchunks + GUARD,), A.NAN).cuda()

    def step(self, zero_grad):
        """One mmt_adamw_step -> host copies of every buffer, the state and the partials."""
        L = _lib()
        n = len(self.hp.lr)
        lr, wd = (ctypes.c_float * n)(*self.hp.lr), (ctypes.c_float * n)(*self.hp.wd)
        L.check(L.LIB.mmt_adamw_step(self.tens.data_ptr(), self.chunks.data_ptr(), self.nchunks, self.partial.data_ptr(),
                                     self.state.data_ptr(), ctypes.cast(lr, ctypes.c_void_p), ctypes.cast(wd, ctypes.c_void_p),
                                     n, self.hp.b1, self.hp.b2, self.hp.eps, self.hp.max_norm, zero_grad, _st()),
                "mmt_adamw_step")
        torch.cuda.synchronize()
        snap = {k: v.cpu() for k, v in self.buf.items()}
        snap.update(state=self.state.cpu(), partial=self.partial.cpu())
        return snap

    def tables_unchanged(self, errors):
        for name, dev, host in (("tensor table", self.tens, self.tables[0]), ("chunk table", self.chunks, self.tables[1])):
            if not torch.equal(dev.cpu(), host):
                errors.append("%s changed" % name)


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def _check_state(errors, snap, steps, clip_is_one=True):
    st = snap["state"]
    if int(_bits(st)[4]) != steps:
        errors.append("state[4] = %d after %d steps" % (int(_bits(st)[4]), steps))
    if clip_is_one and float(st[1]) != 1.0:
        errors.append("state[1] = %r without clipping" % float(st[1]))
    if not bool((st[5:8] == 0).all()) or not bool(torch.isnan(st[8:]).all()):
        errors.append("state written behind its five words")


def _check_layout(errors, what, img, layout, name):
    """The buffer holds numbers exactly where the layout has tensors and NaN everywhere else."""
    want = A.aw_image(torch.zeros(A.AW_TOTAL), layout, name, img.dtype)
    if not torch.equal(torch.isnan(img), torch.isnan(want)):
        bad = (torch.isnan(img) != torch.isnan(want)).nonzero()
        errors.append("%s: %d elements NaN inside a tensor or written outside one, first at %d" % (what, len(bad), int(bad[0])))


@pytest.mark.parametrize("layout", A.AW_LAYOUTS)
def test_adamw_census(layout):
    """g = -0.0, m = v = 0, 1 - lr wd = 1/2, 1/4, 1 by group: after each of two steps every element of every chunk is
    its start times its own group's factor once per step, the shadow its bf16 image, m and v zero, every guard NaN;
    g keeps its bits with zero_grad = 0 and is +0.0 after zero_grad = 1; state[4] counts the steps and partial stays
    untouched without a clip."""
    pr = A.aw_problem("census")
    run = _AdamW("census", layout, A.AW_CENSUS_HP)
    errors = []
    for steps, zero_grad in ((1, 0), (2, 1)):
        snap = run.step(zero_grad)
        want_p, want_sh = A.aw_census_expected(steps)
        tag = "step %d " % steps
        _check(errors, tag + "p", snap["p"], A.aw_image(want_p, layout, "p", F32))
        _check(errors, tag + "shadow", snap["shadow"], A.aw_shadow_image(want_sh, layout))
        for k in "mv":
            _check(errors, tag + k, snap[k], A.aw_image(pr[k], layout, k, F32))
        want_g = A.aw_image(torch.zeros(A.AW_TOTAL) if zero_grad else pr["g"], layout, "g", F32)
        if not torch.equal(_bits(snap["g"]), _bits(want_g)):
            errors.append(tag + "g: %d elements with other bits" % int((_bits(snap["g"]) != _bits(want_g)).sum()))
        _check_state(errors, snap, steps)
        _check(errors, tag + "partial", snap["partial"], torch.full((run.nchunks + GUARD,), A.NAN))
    run.tables_unchanged(errors)
    _report(errors)


AW_RUNS = {"moments": ("moments", A.AW_MOMENTS_HP, (0, 1)), "clip": ("update", A.AW_UPDATE_HPS["clip"], (0, 0, 0)),
           "noclip": ("update", A.AW_UPDATE_HPS["noclip"], (0, 0, 0))}   # family, hyperparameters, zero_grad per step


@functools.lru_cache(maxsize=None)
def _aligned(name):
    """The aligned layout's snapshots of a run, computed once and never modified."""
    family, hp, plan = AW_RUNS[name]
    run = _AdamW(family, "aligned", hp)
    return [run.step(z) for z in plan]


def _check_against_aligned(errors, tag, snap, ref_snap, layout):
    for k in ("p", "m", "v", "shadow"):
        a, b = _bits(A.aw_flat(snap[k], layout, k)), _bits(A.aw_flat(ref_snap[k], "aligned", k))
        if not torch.equal(a, b):
            errors.append("%s%s: %d elements differ from the aligned run, first at flat index %d" %
                          (tag, k, int((a != b).sum()), int((a != b).nonzero()[0])))


def _check_common(errors, tag, snap, layout, g_want):
    """What every family shares: numbers exactly on the tensors, the shadow the bf16 image of the device's p, g's bits."""
    for k in ("p", "g", "m", "v"):
        _check_layout(errors, tag + k, snap[k], layout, k)
    _check(errors, tag + "shadow", snap["shadow"], A.aw_shadow_image(A.aw_flat(snap["p"], layout, "p").bfloat16(), layout))
    want_g = A.aw_image(g_want, layout, "g", F32)
    if not torch.equal(_bits(snap["g"]), _bits(want_g)):
        errors.append(tag + "g: %d elements with other bits" % int((_bits(snap["g"]) != _bits(want_g)).sum()))


@pytest.mark.parametrize("layout", A.AW_LAYOUTS)
def test_adamw_moments(layout):
    """beta1 = 1/2, beta2 = 3/4, integer g and m, v in quarters: m and v after one and two steps are exact whether or
    not the multiply-adds are fused; g survives zero_grad = 0 and is zero after zero_grad = 1; p and the shadow have
    the aligned run's bits."""
    pr = A.aw_problem("moments")
    family, hp, plan = AW_RUNS["moments"]
    run = _AdamW(family, layout, hp)
    errors = []
    for steps, zero_grad in enumerate(plan, 1):
        snap = run.step(zero_grad)
        tag = "step %d " % steps
        want_m, want_v = A.aw_moments_expected(steps)
        _check(errors, tag + "m", snap["m"], A.aw_image(want_m, layout, "m", F32))
        _check(errors, tag + "v", snap["v"], A.aw_image(want_v, layout, "v", F32))
        _check_common(errors, tag, snap, layout, torch.zeros(A.AW_TOTAL) if zero_grad else pr["g"])
        _check_state(errors, snap, steps)
        _check_against_aligned(errors, tag, snap, _aligned("moments")[steps - 1], layout)
    run.tables_unchanged(errors)
    _report(errors)


def _ulps(got, ref):
    return abs(float(got) - ref) / float(np.spacing(np.float32(abs(ref))))


def _check_state_values(errors, tag, st, hp, t, norm64):
    """state[0] within the fp32 summation bound of the float64 norm; state[1..3] within 1 ulp of float64."""
    if hp.max_norm > 0 and not abs(float(st[0]) - norm64) <= A.aw_norm_bound() * norm64:
        errors.append("%snorm %r, float64 %r, bound %.3g" % (tag, float(st[0]), norm64, A.aw_norm_bound() * norm64))
    for i, ref in enumerate(A.aw_state_ref(hp, t, float(st[0])), 1):
        if not _ulps(st[i], ref) <= 1.0:
            errors.append("%sstate[%d] = %r, float64 %r: %.2f ulp" % (tag, i, float(st[i]), ref, _ulps(st[i], ref)))


@pytest.mark.parametrize("layout", A.AW_LAYOUTS)
def test_adamw_norm(layout):
    """g = 1 everywhere: partial[i] is chunk i's element count and the norm float32(sqrt(total elements)), so every
    gradient element is counted once, at every alignment of g."""
    hp = A.AW_NORM_HP
    run = _AdamW("norm", layout, hp)
    snap = run.step(0)
    errors = []
    want = torch.full((run.nchunks + GUARD,), A.NAN)
    want[:run.nchunks] = torch.tensor([float(n) for _, _, n in A.aw_chunks()])
    _check(errors, "partial", snap["partial"], want)
    if float(snap["state"][0]) != A.f32(float(A.AW_TOTAL) ** 0.5):
        errors.append("norm %r, expected %r" % (float(snap["state"][0]), A.f32(float(A.AW_TOTAL) ** 0.5)))
    _check_state(errors, snap, 1, clip_is_one=False)
    _check_state_values(errors, "", snap["state"], hp, 1, float(A.AW_TOTAL) ** 0.5)
    _check_common(errors, "", snap, layout, A.aw_problem("norm")["g"])
    run.tables_unchanged(errors)
    _report(errors)


@pytest.mark.parametrize("clip", ("clip", "noclip"))
@pytest.mark.parametrize("layout", A.AW_LAYOUTS)
def test_adamw_update(layout, clip):
    """N(0, 1) p and g, three steps, the clip active or not, group 2 without weight decay: each step's p, m, v within
    the counted bars of the float64 formula on the device's own previous step, clip factor and bias corrections;
    the state within its own bounds; bit for bit the aligned run wherever the clip factor has that run's bits."""
    family, hp, plan = AW_RUNS[clip]
    pr = A.aw_problem(family)
    run = _AdamW(family, layout, hp)
    norm64 = float(pr["g"].double().pow(2).sum().sqrt())
    prev = {k: pr[k] for k in "pmv"}
    errors, worst, bitwise = [], dict(p=0.0, m=0.0, v=0.0), True
    for steps, zero_grad in enumerate(plan, 1):
        snap = run.step(zero_grad)
        tag = "step %d " % steps
        st = snap["state"]
        _check_state(errors, snap, steps, clip_is_one=clip == "noclip")
        _check_state_values(errors, tag, st, hp, steps, norm64)
        if (float(st[1]) < 1.0) != (clip == "clip"):
            errors.append(tag + "clip factor %r" % float(st[1]))
        r = A.adamw_ref64(prev["p"], pr["g"], prev["m"], prev["v"], hp, st[1:4].tolist())
        ref, bars = dict(zip("pmv", r[:3])), r[3]
        for k in "pmv":
            got = A.aw_flat(snap[k], layout, k)
            ratio = (got.double() - ref[k]).abs() / bars[k]
            if not bool((ratio <= 1.0).all()):
                i = int((~(ratio <= 1.0)).nonzero()[0])
                errors.append("%s%s: %.3g x the bar at flat index %d (got %r, reference %r)" %
                              (tag, k, float(ratio.nan_to_num(float("inf")).max()), i, float(got[i]), float(ref[k][i])))
            worst[k] = max(worst[k], float(ratio.nan_to_num(float("inf")).max()))
            prev[k] = got
        _check_common(errors, tag, snap, layout, pr["g"])
        ref_snap = _aligned(clip)[steps - 1]
        bitwise = bitwise and torch.equal(_bits(st[1:2]), _bits(ref_snap["state"][1:2]))
        if bitwise:
            _check_against_aligned(errors, tag, snap, ref_snap, layout)
        elif "g" not in A.AW_LAYOUTS[layout] or clip == "noclip":
            errors.append(tag + "clip factor %r, aligned run %r" % (float(st[1]), float(ref_snap["state"][1])))
    run.tables_unchanged(errors)
    print("train-glue adamw update %s %s: worst error / bar p %.3f m %.3f v %.3f; %s the aligned run" %
          (layout, clip, worst["p"], worst["m"], worst["v"], "bit for bit" if bitwise else "held to the bars, not to"))
    _report(errors)
