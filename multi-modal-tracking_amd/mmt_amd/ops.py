"""torch.library registration of the native ops: namespace `mmt`.

The reference binds its two native ops through pybind modules (MultiScaleDeformableAttention,
ops/src/vision.cpp:13-16; _prroi_pooling, prroi_pooling_gpu.c:22-113) that torch's tracer cannot see.
Here every native op of the drop-in is a `torch.library.custom_op` over libmmt_hip.so with a fake
(meta) kernel, so FakeTensor / torch.compile / torch.export trace through them, and the differentiable
ones carry `register_autograd` formulas built from the registered backward ops:

  mmt::ms_deform_attn_forward / _backward       mmt_ms_deform_attn_forward / _backward (fp32 / fp64;
                                                ms_deform_attn_func.py:22-38)
  mmt::prroi_pool_forward / _backward / _coor_backward
                                                mmt_prroi_pool_* (fp32; prroi_pool/functional.py:38-76)
  mmt::mam_attention_forward / _backward        mmt_mam_attention (with log-sum-exp) / mmt_mam_attention_bwd
                                                (bf16, the training form of mixformer.py:52-78)
  mmt::mam_attention_asym_forward / _backward   the same pair with asym = 1: the cross-modal form of
                                                asymmetric_shared.py:55-104 (search queries attend [template V |
                                                template I | own search]) on (2 Bh, ntok, 3C), RGB sequences first
  mmt::ce_select                                mmt_ce_t2s_attention_masked + mmt_ce_select: the candidate
                                                elimination's scores and sorted top-k (no autograd formula:
                                                only indices leave get_token_from_attn,
                                                asymmetric_shared_ce.py:22-46)
  mmt::ce_rows_gather / mmt::ce_index_invert    mmt_ce_rows_gather / mmt_ce_index_invert: the pruning and the
                                                recovery of the fp32 token rows in training; the backward of a
                                                row gather is the row gather by the inverted index
  mmt::depth_prepare                            mmt_depth_prepare: a raw 16-bit depth frame clipped, normalised
                                                and replicated into the tracker's (H, W, 3) uint8 frame
  mmt::train_crops                              mmt_train_crops_table: the training input's jittered crops, flips,
                                                brightness jitter and normalise from a device descriptor table

Each *_forward op has its backward registered (register_autograd over the *_backward ops), so
autograd, FakeTensor and torch.compile see one op per native call.
The implementations raise on non-CUDA or non-contiguous tensors as the reference's AT_ASSERTM does;
there is no CPU path.
"""
from typing import Optional

import torch

from ._lib import LIB, AttnBwdParams, AttnParams, MMT_BF16, MMT_F32, MMT_F64, check

_DT = {torch.float32: MMT_F32, torch.float64: MMT_F64}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _need(t, name, dtypes):
    if not t.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor" % name)
    if not t.is_contiguous():
        raise RuntimeError("%s tensor has to be contiguous" % name)
    if dtypes and t.dtype not in dtypes:
        raise RuntimeError("%s: unsupported dtype %s" % (name, t.dtype))


# ------------------------------------------------------------------------------------------- MSDA
@torch.library.custom_op("mmt::ms_deform_attn_forward", mutates_args=())
def ms_deform_attn_forward(value: torch.Tensor, spatial_shapes: torch.Tensor, level_start_index: torch.Tensor,
                           sampling_loc: torch.Tensor, attn_weight: torch.Tensor) -> torch.Tensor:
    """value (N,S,M,D), spatial_shapes (L,2) int64, level_start_index (L) int64, sampling_loc
    (N,Lq,M,L,P,2), attn_weight (N,Lq,M,L,P) -> (N,Lq,M*D)  (ms_deform_attn_cuda.cu:20-80)."""
    for t, nm in ((value, "value"), (sampling_loc, "sampling_loc"), (attn_weight, "attn_weight")):
        _need(t, nm, (torch.float32, torch.float64))
    for t, nm in ((spatial_shapes, "spatial_shapes"), (level_start_index, "level_start_index")):
        _need(t, nm, (torch.int64,))
    if not (value.dtype == sampling_loc.dtype == attn_weight.dtype):
        raise RuntimeError("value / sampling_loc / attn_weight dtypes differ")
    N, S, M, D = value.shape
    _, Lq, _, L, P, _ = sampling_loc.shape
    out = torch.empty(N, Lq, M * D, device=value.device, dtype=value.dtype)
    check(LIB.mmt_ms_deform_attn_forward(value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(),
                                         sampling_loc.data_ptr(), attn_weight.data_ptr(), out.data_ptr(), N, S, M, D,
                                         Lq, L, P, _DT[value.dtype], _stream()), "mmt_ms_deform_attn_forward")
    return out


@ms_deform_attn_forward.register_fake
def _(value, spatial_shapes, level_start_index, sampling_loc, attn_weight):
    N, S, M, D = value.shape
    return value.new_empty(N, sampling_loc.shape[1], M * D)


@torch.library.custom_op("mmt::ms_deform_attn_backward", mutates_args=())
def ms_deform_attn_backward(value: torch.Tensor, spatial_shapes: torch.Tensor, level_start_index: torch.Tensor,
                            sampling_loc: torch.Tensor, attn_weight: torch.Tensor,
                            grad_output: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(grad_value, grad_sampling_loc, grad_attn_weight)  (ms_deform_attn_cuda.cu:83-153)."""
    grad_output = grad_output.contiguous().to(value.dtype)
    N, S, M, D = value.shape
    _, Lq, _, L, P, _ = sampling_loc.shape
    gv, gl, ga = torch.empty_like(value), torch.empty_like(sampling_loc), torch.empty_like(attn_weight)
    check(LIB.mmt_ms_deform_attn_backward(value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(),
                                          sampling_loc.data_ptr(), attn_weight.data_ptr(), grad_output.data_ptr(),
                                          gv.data_ptr(), gl.data_ptr(), ga.data_ptr(), N, S, M, D, Lq, L, P,
                                          _DT[value.dtype], _stream()), "mmt_ms_deform_attn_backward")
    return gv, gl, ga


@ms_deform_attn_backward.register_fake
def _(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output):
    return torch.empty_like(value), torch.empty_like(sampling_loc), torch.empty_like(attn_weight)


def _msda_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def _msda_backward(ctx, grad):
    value, shapes, starts, loc, aw = ctx.saved_tensors
    gv, gl, ga = ms_deform_attn_backward(value, shapes, starts, loc, aw, grad)
    return gv, None, None, gl, ga


ms_deform_attn_forward.register_autograd(_msda_backward, setup_context=_msda_setup)


# --------------------------------------------------------------------------------------- PrRoIPool
@torch.library.custom_op("mmt::prroi_pool_forward", mutates_args=())
def prroi_pool_forward(features: torch.Tensor, rois: torch.Tensor, pooled_height: int, pooled_width: int,
                       spatial_scale: float) -> torch.Tensor:
    """features (B,C,H,W) fp32, rois (R,5) fp32 -> (R,C,ph,pw)  (prroi_pooling_gpu.c:22-50)."""
    _need(features, "features", (torch.float32,))
    _need(rois, "rois", (torch.float32,))
    B, C, H, W = features.shape
    R = rois.shape[0]
    ph, pw = int(pooled_height), int(pooled_width)
    out = torch.empty(R, C, ph, pw, device=features.device, dtype=torch.float32)
    check(LIB.mmt_prroi_pool_forward(features.data_ptr(), rois.data_ptr(), out.data_ptr(), R, C, H, W, C * H * W,
                                     H * W, W, 1, ph, pw, float(spatial_scale), C * ph * pw, ph * pw, 1, _stream()),
          "mmt_prroi_pool_forward")
    return out


@prroi_pool_forward.register_fake
def _(features, rois, pooled_height, pooled_width, spatial_scale):
    return features.new_empty(rois.shape[0], features.shape[1], pooled_height, pooled_width)


@torch.library.custom_op("mmt::prroi_pool_backward", mutates_args=())
def prroi_pool_backward(features: torch.Tensor, rois: torch.Tensor, grad_output: torch.Tensor, pooled_height: int,
                        pooled_width: int, spatial_scale: float) -> torch.Tensor:
    """grad_features (B,C,H,W); `features` gives the shape only (prroi_pooling_gpu.c:52-80)."""
    _need(rois, "rois", (torch.float32,))
    B, C, H, W = features.shape
    g = grad_output.contiguous().float()
    gf = torch.empty(B, C, H, W, device=rois.device, dtype=torch.float32)
    check(LIB.mmt_prroi_pool_backward(rois.data_ptr(), g.data_ptr(), gf.data_ptr(), B, rois.shape[0], C, H, W,
                                      int(pooled_height), int(pooled_width), float(spatial_scale), _stream()),
          "mmt_prroi_pool_backward")
    return gf


@prroi_pool_backward.register_fake
def _(features, rois, grad_output, pooled_height, pooled_width, spatial_scale):
    return torch.empty_like(features, dtype=torch.float32)


@torch.library.custom_op("mmt::prroi_pool_coor_backward", mutates_args=())
def prroi_pool_coor_backward(features: torch.Tensor, rois: torch.Tensor, output: torch.Tensor, grad_output: torch.Tensor,
                             pooled_height: int, pooled_width: int, spatial_scale: float) -> torch.Tensor:
    """grad_rois (R,5), column 0 = 0 (prroi_pooling_gpu.c:82-113)."""
    _need(features, "features", (torch.float32,))
    _need(rois, "rois", (torch.float32,))
    B, C, H, W = features.shape
    g = grad_output.contiguous().float()
    gr = torch.empty_like(rois)
    check(LIB.mmt_prroi_pool_coor_backward(features.data_ptr(), rois.data_ptr(), output.data_ptr(), g.data_ptr(),
                                           gr.data_ptr(), rois.shape[0], C, H, W, int(pooled_height), int(pooled_width),
                                           float(spatial_scale), _stream()), "mmt_prroi_pool_coor_backward")
    return gr


@prroi_pool_coor_backward.register_fake
def _(features, rois, output, grad_output, pooled_height, pooled_width, spatial_scale):
    return torch.empty_like(rois)


def _prroi_setup(ctx, inputs, output):
    features, rois, ph, pw, sc = inputs
    ctx.params = (ph, pw, sc)
    ctx.save_for_backward(features, rois, output)


def _prroi_backward(ctx, grad):
    features, rois, out = ctx.saved_tensors
    ph, pw, sc = ctx.params
    gf = prroi_pool_backward(features, rois, grad, ph, pw, sc) if ctx.needs_input_grad[0] else None
    gr = prroi_pool_coor_backward(features, rois, out, grad, ph, pw, sc) if ctx.needs_input_grad[1] else None
    return gf, gr, None, None, None


prroi_pool_forward.register_autograd(_prroi_backward, setup_context=_prroi_setup)


# ---------------------------------------------------------------------------------- MAM attention
@torch.library.custom_op("mmt::mam_attention_forward", mutates_args=())
def mam_attention_forward(qkv: torch.Tensor, n_t: int, heads: int) -> tuple[torch.Tensor, torch.Tensor]:
    """qkv [S][ntok][3C] bf16 (the fused qkv Linear output) -> (out [S][ntok][C] bf16, lse [S][H][ntok]
    fp32 log2-sum-exp2 of the scaled scores); template queries [0, n_t) attend template keys, search
    queries all keys (mixformer.py:52-78)."""
    _need(qkv, "qkv", (torch.bfloat16,))
    S, ntok, C3 = qkv.shape
    C = C3 // 3
    out = torch.empty(S, ntok, C, device=qkv.device, dtype=torch.bfloat16)
    lse = torch.empty(S, heads, ntok, device=qkv.device, dtype=torch.float32)
    p = AttnParams()
    p.qkv, p.out, p.S, p.Bm, p.ntok, p.n_t, p.C, p.H, p.asym = qkv.data_ptr(), out.data_ptr(), S, S, ntok, n_t, C, heads, 0
    p.scale, p.impl, p.lse = (C // heads) ** -0.5, 0, lse.data_ptr()
    check(LIB.mmt_mam_attention(p, MMT_BF16, _stream()), "mmt_mam_attention")
    return out, lse


@mam_attention_forward.register_fake
def _(qkv, n_t, heads):
    S, ntok, C3 = qkv.shape
    return qkv.new_empty(S, ntok, C3 // 3), qkv.new_empty(S, heads, ntok, dtype=torch.float32)


@torch.library.custom_op("mmt::mam_attention_backward", mutates_args=())
def mam_attention_backward(qkv: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, lse: torch.Tensor, n_t: int,
                           heads: int) -> torch.Tensor:
    """dL/dqkv [S][ntok][3C] bf16 (deterministic, mmt_mam_attention_bwd)."""
    _need(qkv, "qkv", (torch.bfloat16,))
    S, ntok, C3 = qkv.shape
    C = C3 // 3
    dout = dout.to(torch.bfloat16).contiguous()
    delta = torch.empty_like(lse)
    dqkv = torch.empty_like(qkv)
    p = AttnBwdParams()
    p.qkv, p.out, p.dout, p.lse, p.delta, p.dqkv = (qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(),
                                                    delta.data_ptr(), dqkv.data_ptr())
    p.S, p.Bm, p.ntok, p.n_t, p.C, p.H, p.asym, p.scale = S, S, ntok, n_t, C, heads, 0, (C // heads) ** -0.5
    check(LIB.mmt_mam_attention_bwd(p, MMT_BF16, _stream()), "mmt_mam_attention_bwd")
    return dqkv


@mam_attention_backward.register_fake
def _(qkv, out, dout, lse, n_t, heads):
    return torch.empty_like(qkv)


def _mam_setup(ctx, inputs, output):
    qkv, n_t, heads = inputs
    out, lse = output
    ctx.args = (n_t, heads)
    ctx.save_for_backward(qkv, out, lse)


def _mam_backward(ctx, dout, dlse):
    qkv, out, lse = ctx.saved_tensors
    n_t, heads = ctx.args
    return mam_attention_backward(qkv, out, dout, lse, n_t, heads), None, None


mam_attention_forward.register_autograd(_mam_backward, setup_context=_mam_setup)


@torch.library.custom_op("mmt::mam_attention_asym_forward", mutates_args=())
def mam_attention_asym_forward(qkv: torch.Tensor, Bh: int, n_t: int, heads: int) -> tuple[torch.Tensor, torch.Tensor]:
    """The cross-modal asymmetric form (asymmetric_shared.py:55-104) on qkv [2 Bh][ntok][3C] bf16, the Bh RGB
    sequences first -> (out [2 Bh][ntok][C] bf16, lse [2 Bh][H][ntok] fp32): template queries attend the template
    keys of their own sequence, search queries of sequence s attend [template of s % Bh | template of
    s % Bh + Bh | own search]."""
    _need(qkv, "qkv", (torch.bfloat16,))
    S, ntok, C3 = qkv.shape
    if S != 2 * Bh:
        raise RuntimeError("mam_attention_asym_forward: qkv (2 Bh, ntok, 3C) expected")
    C = C3 // 3
    out = torch.empty(S, ntok, C, device=qkv.device, dtype=torch.bfloat16)
    lse = torch.empty(S, heads, ntok, device=qkv.device, dtype=torch.float32)
    p = AttnParams()
    p.qkv, p.out, p.S, p.Bm, p.ntok, p.n_t, p.C, p.H, p.asym = qkv.data_ptr(), out.data_ptr(), S, Bh, ntok, n_t, C, heads, 1
    p.scale, p.impl, p.lse = (C // heads) ** -0.5, 0, lse.data_ptr()
    check(LIB.mmt_mam_attention(p, MMT_BF16, _stream()), "mmt_mam_attention")
    return out, lse


@mam_attention_asym_forward.register_fake
def _(qkv, Bh, n_t, heads):
    S, ntok, C3 = qkv.shape
    return qkv.new_empty(S, ntok, C3 // 3), qkv.new_empty(S, heads, ntok, dtype=torch.float32)


@torch.library.custom_op("mmt::mam_attention_asym_backward", mutates_args=())
def mam_attention_asym_backward(qkv: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, lse: torch.Tensor, Bh: int,
                                n_t: int, heads: int) -> torch.Tensor:
    """dL/dqkv [2 Bh][ntok][3C] bf16 of the cross-modal form (deterministic, mmt_mam_attention_bwd with asym = 1):
    dK / dV of a template key sum its own template queries and the search queries of both modalities."""
    _need(qkv, "qkv", (torch.bfloat16,))
    S, ntok, C3 = qkv.shape
    C = C3 // 3
    dout = dout.to(torch.bfloat16).contiguous()
    delta = torch.empty_like(lse)
    dqkv = torch.empty_like(qkv)
    p = AttnBwdParams()
    p.qkv, p.out, p.dout, p.lse, p.delta, p.dqkv = (qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(),
                                                    delta.data_ptr(), dqkv.data_ptr())
    p.S, p.Bm, p.ntok, p.n_t, p.C, p.H, p.asym, p.scale = S, Bh, ntok, n_t, C, heads, 1, (C // heads) ** -0.5
    check(LIB.mmt_mam_attention_bwd(p, MMT_BF16, _stream()), "mmt_mam_attention_bwd")
    return dqkv


@mam_attention_asym_backward.register_fake
def _(qkv, out, dout, lse, Bh, n_t, heads):
    return torch.empty_like(qkv)


def _mam_asym_setup(ctx, inputs, output):
    qkv, Bh, n_t, heads = inputs
    out, lse = output
    ctx.args = (Bh, n_t, heads)
    ctx.save_for_backward(qkv, out, lse)


def _mam_asym_backward(ctx, dout, dlse):
    qkv, out, lse = ctx.saved_tensors
    Bh, n_t, heads = ctx.args
    return mam_attention_asym_backward(qkv, out, dout, lse, Bh, n_t, heads), None, None, None


mam_attention_asym_forward.register_autograd(_mam_asym_backward, setup_context=_mam_asym_setup)


# --------------------------------------------------------------------------- candidate elimination
@torch.library.custom_op("mmt::ce_select", mutates_args=())
def ce_select(qkv: torch.Tensor, template_mask: Optional[torch.Tensor], gidx_in: Optional[torch.Tensor], n_t: int,
              heads: int, keep: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """candidate_elimination's discrete part (asymmetric_shared_ce.py:52-102) on qkv [2B][n_t + n_s][3C]
    (bf16: MFMA scores, or fp32), RGB sequences first: attn_mean [B][2 n_s] fp32 = the softmax over
    [k_s_V | k_s_I] of the template queries [q_mt_V ; q_mt_I], averaged over the heads and over the
    queries template_mask [B][2 n_t] (uint8 / bool, None = all) selects; order [2B][keep] int32 = each
    modality's search tokens by attn_mean descending (ties by index), the first `keep`; gidx_out
    [2B][keep] = gidx_in[order] (gidx_in [2B][n_s] int32, None = identity).  Not differentiable: only
    the indices leave get_token_from_attn (:31-46), so there is no autograd formula."""
    _need(qkv, "qkv", (torch.bfloat16, torch.float32))
    S, rows, C3 = qkv.shape
    C, Bm, n_s = C3 // 3, S // 2, rows - n_t
    if S % 2 or n_s <= 0 or not 0 < keep <= n_s:
        raise RuntimeError("ce_select: qkv (2B, n_t + n_s, 3C) with 0 < keep <= n_s expected")
    dev = qkv.device
    nq = 2 * n_t
    count = None
    if template_mask is not None:
        _need(template_mask, "template_mask", (torch.uint8, torch.bool))
        if tuple(template_mask.shape) != (Bm, nq):
            raise RuntimeError("ce_select: template_mask (B, 2 n_t) expected")
        template_mask = template_mask.view(torch.uint8) if template_mask.dtype == torch.bool else template_mask
        count = template_mask.sum(1, keepdim=True, dtype=torch.float32)  # on the device: capturable
    if gidx_in is not None:
        _need(gidx_in, "gidx_in", (torch.int32,))
        if tuple(gidx_in.shape) != (S, n_s):
            raise RuntimeError("ce_select: gidx_in (2B, n_s) expected")
    bf = qkv.dtype == torch.bfloat16
    nparts = heads * (nq // (16 if bf else 8))
    part = torch.empty(Bm * max(nparts, 1) * 2 * n_s, device=dev, dtype=torch.float32)
    check(LIB.mmt_ce_t2s_attention_masked(qkv.data_ptr(), part.data_ptr(),
                                          template_mask.data_ptr() if template_mask is not None else None, Bm, rows,
                                          n_t, n_s, C, heads, (C // heads) ** -0.5, MMT_BF16 if bf else MMT_F32,
                                          _stream()), "mmt_ce_t2s_attention_masked")
    order = torch.empty(S, n_s, device=dev, dtype=torch.int32)
    gidx = torch.empty(S, n_s, device=dev, dtype=torch.int32)
    mean = torch.empty(Bm, 2 * n_s, device=dev, dtype=torch.float32)
    # the sums over heads and queries times 1 / (heads * queries); with a mask the per-frame query count is
    # divided out on the device (no host read: the op can be captured)
    check(LIB.mmt_ce_select(part.data_ptr(), nparts, Bm, n_s, keep, n_s, gidx_in.data_ptr() if gidx_in is not None
                            else None, gidx.data_ptr(), order.data_ptr(), mean.data_ptr(),
                            1.0 / (heads * (nq if count is None else 1)), _stream()), "mmt_ce_select")
    if count is not None:
        mean = mean / count
    return order[:, :keep].contiguous(), gidx[:, :keep].contiguous(), mean


@ce_select.register_fake
def _(qkv, template_mask, gidx_in, n_t, heads, keep):
    S, rows, _ = qkv.shape
    return (qkv.new_empty(S, keep, dtype=torch.int32), qkv.new_empty(S, keep, dtype=torch.int32),
            qkv.new_empty(S // 2, 2 * (rows - n_t), dtype=torch.float32))


@torch.library.custom_op("mmt::ce_index_invert", mutates_args=())
def ce_index_invert(idx: torch.Tensor, n_out: int) -> torch.Tensor:
    """idx [S][n_in] int32 -> [S][n_out] int32 with out[s][idx[s][j]] = j and -1 elsewhere (entries outside
    [0, n_out) skipped): the index vector of a row gather's backward."""
    _need(idx, "idx", (torch.int32,))
    S, n_in = idx.shape
    out = torch.empty(S, n_out, device=idx.device, dtype=torch.int32)
    check(LIB.mmt_ce_index_invert(idx.data_ptr(), n_in, out.data_ptr(), n_out, S, _stream()), "mmt_ce_index_invert")
    return out


@ce_index_invert.register_fake
def _(idx, n_out):
    return idx.new_empty(idx.shape[0], n_out)


@torch.library.custom_op("mmt::ce_rows_gather", mutates_args=())
def ce_rows_gather(x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """x [S][rows][C] fp32, idx [S][n] int32 -> y [S][n][C] with y[s][r] = x[s][idx[s][r]], a zero row where
    idx is outside [0, rows): the pruning of the search tokens (idx = template rows, then the kept rows in
    sorted order) and their recovery (idx = the inverted global index), _recover_search
    asymmetric_shared_ce.py:426-447."""
    _need(x, "x", (torch.float32,))
    _need(idx, "idx", (torch.int32,))
    S, rows, C = x.shape
    if idx.dim() != 2 or idx.shape[0] != S:
        raise RuntimeError("ce_rows_gather: idx (S, n) expected")
    n = idx.shape[1]
    y = torch.empty(S, n, C, device=x.device, dtype=torch.float32)
    check(LIB.mmt_ce_rows_gather(x.data_ptr(), rows, y.data_ptr(), n, idx.data_ptr(), S, C, _stream()),
          "mmt_ce_rows_gather")
    return y


@ce_rows_gather.register_fake
def _(x, idx):
    return x.new_empty(x.shape[0], idx.shape[1], x.shape[2])


def _rows_setup(ctx, inputs, output):
    x, idx = inputs
    ctx.rows = x.shape[1]
    ctx.save_for_backward(idx)


def _rows_backward(ctx, dy):
    # distinct indices: every source row feeds at most one destination row, so the scatter is a gather by
    # the inverted index (zeros where a row was pruned), with no atomics
    idx, = ctx.saved_tensors
    return ce_rows_gather(dy.float().contiguous(), ce_index_invert(idx, ctx.rows)), None


ce_rows_gather.register_autograd(_rows_backward, setup_context=_rows_setup)


# ------------------------------------------------------------------------------------------- RGB-D input
@torch.library.custom_op("mmt::depth_prepare", mutates_args=())
def depth_prepare(depth: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """depth (H, W) uint16 (or int16 as its bit pattern) -> (frame (H, W, 3) uint8, record (7,) int32): the
    reference's get_rgbd_frame(dtype="rgb3d", depth_clip=True) on the device (mmt_depth_prepare;
    mmt_amd.depth.depth_to_3xd is its numpy restatement)."""
    from .depth import prepare_depth
    _need(depth, "depth", (torch.uint16, torch.int16))
    if depth.dim() != 2 or depth.numel() == 0:
        raise RuntimeError("depth_prepare: a non-empty (H, W) frame expected")
    return prepare_depth(depth)


@depth_prepare.register_fake
def _(depth):
    H, W = depth.shape
    return depth.new_empty(H, W, 3, dtype=torch.uint8), depth.new_empty(7, dtype=torch.int32)


# ------------------------------------------------------------------------------------------- training input
@torch.library.custom_op("mmt::train_crops", mutates_args=("images_v", "images_i", "att_v", "att_i", "crop"))
def train_crops(table: torch.Tensor, enable: Optional[torch.Tensor], out_sz: int, images_v: torch.Tensor,
                images_i: torch.Tensor, att_v: torch.Tensor, att_i: torch.Tensor, crop: torch.Tensor) -> None:
    """mmt_train_crops_table over a device table of mmt_train_crop_params (a uint8 tensor, one entry per
    sizeof(mmt_train_crop_params) bytes), enable: None or one byte per entry.  The entries' out / att pointers lie
    inside images_v / images_i (fp32) and att_v / att_i (uint8), their crop records inside crop (fp64), and their
    patch pointers are NULL: the five tensors are all this op may write
    (mmt_amd.train_input.TrainInputProcessor owns both; process_sample_reference is the host restatement)."""
    from ._lib import TrainCropParams
    import ctypes
    _need(table, "table", (torch.uint8,))
    size = ctypes.sizeof(TrainCropParams)
    if table.dim() != 1 or table.numel() == 0 or table.numel() % size:
        raise RuntimeError("train_crops: table must hold a whole number (>= 1) of %d-byte entries" % size)
    n = table.numel() // size
    if enable is not None:
        _need(enable, "enable", (torch.uint8,))
        if enable.numel() != n:
            raise RuntimeError("train_crops: enable must hold one byte per entry (%d), got %d" % (n, enable.numel()))
    for t, name, dt in ((images_v, "images_v", torch.float32), (images_i, "images_i", torch.float32),
                        (att_v, "att_v", torch.uint8), (att_i, "att_i", torch.uint8), (crop, "crop", torch.float64)):
        _need(t, name, (dt,))
    check(LIB.mmt_train_crops_table(table.data_ptr(), enable.data_ptr() if enable is not None else None, n, out_sz,
                                    torch.cuda.current_stream().cuda_stream), "mmt_train_crops_table")


@train_crops.register_fake
def _(table, enable, out_sz, images_v, images_i, att_v, att_i, crop):
    return None


def mam_attention(qkv, n_t, heads):
    """Differentiable MAM attention output (bf16): mmt::mam_attention_forward's first output."""
    return mam_attention_forward(qkv.contiguous(), n_t, heads)[0]


def mam_attention_asym(qkv, Bh, n_t, heads):
    """Differentiable cross-modal MAM attention output (bf16): mmt::mam_attention_asym_forward's first output."""
    return mam_attention_asym_forward(qkv.contiguous(), Bh, n_t, heads)[0]


def ms_deform_attn(value, spatial_shapes, level_start_index, sampling_loc, attn_weight):
    """Differentiable MSDA (MSDeformAttnFunction.apply without im2col_step)."""
    return ms_deform_attn_forward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight)


def prroi_pool2d(features, rois, pooled_height, pooled_width, spatial_scale):
    """Differentiable PrRoIPool2D (fp32)."""
    return prroi_pool_forward(features, rois, int(pooled_height), int(pooled_width), float(spatial_scale))
