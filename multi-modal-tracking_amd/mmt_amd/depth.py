"""RGB-D input: the reference's per-frame preparation of a raw 16-bit depth frame.

The reference's RGB-D evaluation (lib/test/evaluation/tracker_rgbt.py:216-218 ->
get_rgbd_frame(..., dtype="rgb3d", depth_clip=True), lib/test/evaluation/depth_utils.py:17-22, :55-60)
turns every DepthTrack depth frame, a single-channel 16-bit PNG, into the tracker's second modality on
the host: clip at three times the frame's median (capped at 10 000), cv2.normalize(NORM_MINMAX) to
0..255, uint8, replicate to three channels.

depth_to_3xd  the contract: that preparation restated in numpy, all-integer up to the affine.
prepare_depth the same on the device (csrc/depth.hip: mmt_depth_prepare), bit for bit.

cv2 is not part of this image: the normalize step restates OpenCV's conventions (float64 scale and shift,
float32 src * a + b with two roundings, saturate_cast rounding to nearest-even) and has not been run
against OpenCV; whether OpenCV's vector path fuses the multiply-add is not known.
"""
import ctypes

import numpy as np
import torch

from ._lib import DEPTH_WORK_BYTES, LIB, DepthParams, check

DEPTH_CAP = 10000
RECORD_INTS = 7  # s[k0], s[k1], capi, smin, smax, float bits of a, float bits of b
AUX_FORMATS = ("rgb8", "depth16")


def depth_cap(s0, s1):
    """uint16(trunc(min(3 * (s0 + s1) / 2, 10000.0))) in integers: the clip value from the two middle order
    statistics (numpy's median is their mean, exact in float64; assigning the float cap into a uint16 array
    truncates it)."""
    return min((3 * (int(s0) + int(s1))) >> 1, DEPTH_CAP)


def depth_record(depth):
    """(s[k0], s[k1], capi, smin, smax, a, b) of a (H, W) uint16 frame: the median's two order statistics, the
    clip value, min and max of the clipped frame, and the float32 affine of cv2.normalize(NORM_MINMAX, 0, 255)."""
    d = np.asarray(depth)
    if d.dtype != np.uint16 or d.ndim != 2 or d.size == 0:
        raise ValueError("depth must be a non-empty (H, W) uint16 array, got %s %s" % (d.dtype, d.shape))
    n = d.size
    k0, k1 = (n - 1) // 2, n // 2
    part = np.partition(d.reshape(-1), (k0, k1))
    s0, s1 = int(part[k0]), int(part[k1])
    capi = depth_cap(s0, s1)
    smin, smax = min(int(d.min()), capi), min(int(d.max()), capi)  # of the clipped frame
    span = float(smax) - float(smin)
    scale = 255.0 * (1.0 / span if span > np.finfo(np.float64).eps else 0.0)
    shift = 0.0 - float(smin) * scale
    return s0, s1, capi, smin, smax, np.float32(scale), np.float32(shift)


def depth_to_3xd(depth):
    """(H, W) uint16 depth -> (H, W, 3) uint8, the reference's get_rgbd_frame(dtype="rgb3d", depth_clip=True):
    with s the sorted pixels, k0 = (n-1)//2, k1 = n//2: capi = min((3 * (s[k0] + s[k1])) >> 1, 10000);
    d' = min(d, capi); smin, smax = min, max of d'; scale = 255 / (smax - smin) (0 when they are equal) and
    shift = -smin * scale in float64; per pixel fl32(fl32(float32(d') * float32(scale)) + float32(shift)),
    rounded half to even, saturated to 0..65535, low 8 bits; three equal channels."""
    d = np.asarray(depth)
    _, _, capi, _, _, a, b = depth_record(d)
    clipped = np.minimum(d, np.uint16(capi)).astype(np.float32)
    r = np.rint((clipped * a).astype(np.float32) + b)  # float32 throughout: product and sum round separately
    u8 = np.clip(r, 0, 65535).astype(np.uint16).astype(np.uint8)
    return np.repeat(u8[:, :, None], 3, axis=2)


def as_depth16(x, what="depth frame"):
    """A (H, W) 16-bit frame as a torch int16 tensor holding the uint16 bit pattern (host or device, no copy
    where the input allows).  Accepts numpy uint16, torch uint16, and torch int16 taken as the bit pattern of
    the uint16 values (torch's own uint16 has few operators).  ValueError otherwise."""
    if isinstance(x, np.ndarray):
        if x.dtype != np.uint16:
            raise ValueError("%s must be uint16, got %s" % (what, x.dtype))
        if x.ndim != 2:
            raise ValueError("%s must be (H, W), got shape %s" % (what, tuple(x.shape)))
        return torch.from_numpy(np.ascontiguousarray(x).view(np.int16))
    if not isinstance(x, torch.Tensor):
        raise ValueError("%s must be a numpy array or a torch tensor, got %s" % (what, type(x).__name__))
    if x.dtype not in (torch.uint16, torch.int16):
        raise ValueError("%s must be uint16 (or int16 as its bit pattern), got %s" % (what, x.dtype))
    if x.dim() != 2:
        raise ValueError("%s must be (H, W), got shape %s" % (what, tuple(x.shape)))
    x = x.contiguous()
    return x.view(torch.int16) if x.dtype == torch.uint16 else x


def check_aux_format(aux_format):
    if aux_format not in AUX_FORMATS:
        raise ValueError("aux_format must be one of %s, got %r" % (", ".join(repr(f) for f in AUX_FORMATS), aux_format))
    return aux_format


def depth_params(depth, out, work, record=None):
    """mmt_depth_params of one frame: depth (H, W) int16 / uint16, out H * W * 3 uint8 values, work
    DEPTH_WORK_BYTES bytes, record 7 int32 or None -- device tensors."""
    if depth.dim() != 2 or depth.dtype not in (torch.int16, torch.uint16) or not depth.is_contiguous() or not depth.is_cuda:
        raise ValueError("depth must be a contiguous (H, W) 16-bit device tensor")
    H, W = depth.shape
    if H <= 0 or W <= 0:
        raise ValueError("depth must be a non-empty (H, W) frame, got shape %s" % ((H, W),))
    if out.dtype != torch.uint8 or out.numel() != H * W * 3 or not out.is_contiguous() or out.device != depth.device:
        raise ValueError("out must be a contiguous (%d, %d, 3) uint8 tensor on %s" % (H, W, depth.device))
    if work.numel() * work.element_size() < DEPTH_WORK_BYTES or not work.is_contiguous() or work.device != depth.device:
        raise ValueError("work must hold %d bytes on %s" % (DEPTH_WORK_BYTES, depth.device))
    if record is not None and (record.dtype != torch.int32 or record.numel() != RECORD_INTS or not record.is_contiguous()
                               or record.device != depth.device):
        raise ValueError("record must be %d int32 values on %s" % (RECORD_INTS, depth.device))
    p = DepthParams()
    p.depth, p.H, p.W = depth.data_ptr(), H, W
    p.out, p.work = out.data_ptr(), work.data_ptr()
    p.record = record.data_ptr() if record is not None else None
    return p


def prepare_depth(depth_dev, out=None, record=None, work=None, stream=None):
    """One frame on the device: depth_dev (H, W) uint16 (or int16 as its bit pattern) -> (out, record), out
    (H, W, 3) uint8 = depth_to_3xd(depth), record 7 int32 (s[k0], s[k1], capi, smin, smax, float bits of a and
    b).  out / record / work (DEPTH_WORK_BYTES of scratch) are allocated when not given.  Five launches on the
    current stream, no host read-back."""
    if not isinstance(depth_dev, torch.Tensor) or not depth_dev.is_cuda:
        raise ValueError("prepare_depth takes a device tensor (depth_to_3xd is the host form)")
    d = as_depth16(depth_dev)
    H, W = d.shape
    dev = d.device
    if out is None:
        out = torch.empty(H, W, 3, device=dev, dtype=torch.uint8)
    if record is None:
        record = torch.empty(RECORD_INTS, device=dev, dtype=torch.int32)
    if work is None:
        work = torch.empty(DEPTH_WORK_BYTES, device=dev, dtype=torch.uint8)
    p = depth_params(d, out, work, record)
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    check(LIB.mmt_depth_prepare(ctypes.byref(p), 1, s), "mmt_depth_prepare")
    return out, record
