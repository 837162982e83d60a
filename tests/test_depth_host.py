"""Host side of the RGB-D input (no GPU): mmt_amd.depth.depth_to_3xd against a line-by-line transcription of the
reference's numpy steps (lib/test/evaluation/depth_utils.py:17-22, :55-60), the integer form of the cap, the C ABI
(symbols, struct layout, refusals before any launch) and the trackers' refusals."""
import ctypes
import importlib
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT
from depth_probes import FRAMES, SHAPES, frame

HEADER = os.path.join(ROOT, "include", "mmt_hip.h")
EBADARG = -10000
MODULES = ["mixformer_vit_rgbt", "mixformer_vit_rgbt_shared", "mixformer_vit_rgbt_unibackbone", "asymmetric_shared",
           "asymmetric_shared_online", "asymmetric_shared_ce"]


# ------------------------------------------------------------------ semantics
def _normalize_minmax_0_255(src):
    """cv2.normalize(src, None, alpha=0, beta=255, norm_type=cv2.NORM_MINMAX) on a uint16 image, the source depth
    kept: OpenCV's conventions (float64 scale and shift, convertTo in float32 src * a + b, saturate_cast by
    cvRound = round half to even)."""
    smin, smax = float(src.min()), float(src.max())
    scale = 255.0 * (1.0 / (smax - smin) if smax - smin > np.finfo(np.float64).eps else 0.0)
    shift = 0.0 - smin * scale
    a, b = np.float32(scale), np.float32(shift)
    r = np.rint(src.astype(np.float32) * a + b)
    return np.clip(r, 0, 65535).astype(np.uint16)


def _merge(channels):
    return np.stack(channels, axis=2)


def _reference_rgb3d(depth):
    """get_rgbd_frame(..., dtype="rgb3d", depth_clip=True), depth_utils.py:17-22 and :55-60, line by line."""
    dp = depth.copy()
    max_depth = min(np.median(dp) * 3, 10000)
    dp[dp > max_depth] = max_depth
    dp = _normalize_minmax_0_255(dp)
    dp = np.asarray(dp, dtype=np.uint8)
    dp = _merge((dp, dp, dp))
    return dp


def test_depth_to_3xd_equals_reference_steps_on_random_frames():
    from mmt_amd.depth import depth_to_3xd
    rng = np.random.default_rng(5)
    for i in range(200):
        H, W = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        kind = i % 4
        if kind == 0:
            d = rng.integers(0, 65536, (H, W))
        elif kind == 1:
            d = np.minimum(rng.gamma(2.0, 900.0, (H, W)), 65535)
            d[rng.random((H, W)) < 0.1] = 0
        elif kind == 2:
            lo = int(rng.integers(0, 4000))
            d = rng.integers(lo, lo + int(rng.integers(1, 600)), (H, W))
        else:
            d = rng.integers(0, 12000, (H, W)) * (rng.random((H, W)) < 0.6)
        d = d.astype(np.uint16)
        got = depth_to_3xd(d)
        assert got.dtype == np.uint8 and got.shape == (H, W, 3)
        assert np.array_equal(got, _reference_rgb3d(d)), (i, H, W)


@pytest.mark.parametrize("make", FRAMES, ids=lambda f: f.__name__[2:])
def test_depth_to_3xd_equals_reference_steps_on_edge_frames(make):
    from mmt_amd.depth import depth_to_3xd
    for H, W in SHAPES + [(360, 640)]:
        d = frame(make, H, W)
        assert d.dtype == np.uint16 and d.shape == (H, W)
        got = depth_to_3xd(d)
        assert np.array_equal(got, _reference_rgb3d(d)), (H, W)
        assert np.array_equal(got[:, :, 0], got[:, :, 1]) and np.array_equal(got[:, :, 0], got[:, :, 2])


def test_integer_cap_equals_float_cap_for_every_sum():
    """capi = min((3 * (s0 + s1)) >> 1, 10000) is numpy's uint16 assignment of min(median * 3, 10000), for every
    sum s0 + s1 of two uint16 values."""
    from mmt_amd.depth import depth_cap
    t = np.arange(0, 131071, dtype=np.int64)
    med = t.astype(np.float64) / 2.0  # np.median of an even count: the mean of the two middle values, exact
    max_depth = np.minimum(med * 3, 10000)
    cells = np.full(t.size, 65535, np.uint16)  # one far pixel per sum
    far = cells > max_depth
    assert far.all()
    cells[far] = max_depth[far]  # the reference's assignment of the float cap into the uint16 image
    got = np.minimum((3 * t) >> 1, 10000)
    assert np.array_equal(got, cells.astype(np.int64))
    one = np.array([65535], np.uint16)
    for m in (0.5, 301.5, 3333.5, 9999.5 / 3):  # the scalar form the reference uses
        one[0] = 65535
        one[one > min(m * 3, 10000)] = min(m * 3, 10000)
        assert one[0] == int(min(m * 3, 10000))
    for s0, s1 in ((0, 0), (255, 256), (100, 101), (3333, 3334), (3334, 3334), (65535, 65535)):
        assert depth_cap(s0, s1) == got[s0 + s1]
    # an odd count: s0 == s1, the median is the value itself
    assert all(depth_cap(v, v) == min(3 * v, 10000) for v in range(0, 65536, 257))


def test_depth_record_fields():
    from mmt_amd.depth import depth_record
    d = np.array([[0, 10, 20, 400]], np.uint16)  # median 15, cap 45: 400 is clipped
    s0, s1, capi, smin, smax, a, b = depth_record(d)
    assert (s0, s1, capi, smin, smax) == (10, 20, 45, 0, 45)
    assert a == np.float32(255.0 / 45.0) and b == np.float32(0.0)
    assert depth_record(np.full((3, 3), 60000, np.uint16))[2:5] == (10000, 10000, 10000)  # everything clipped


# ------------------------------------------------------------------ C ABI
def test_symbols_declared_exported_and_bound():
    from mmt_amd import _lib
    src = open(HEADER).read()
    for name in ("mmt_depth_prepare", "mmt_depth_prepare_table"):
        assert "int %s(" % name in src
        assert name in _lib.EXPORTED
        assert getattr(_lib.LIB, name).argtypes is not None
    assert _lib.LIB.mmt_depth_prepare.argtypes[0] == ctypes.POINTER(_lib.DepthParams)
    assert "#define MMT_DEPTH_WORK_BYTES %d" % _lib.DEPTH_WORK_BYTES in src


def test_depth_params_layout_matches_header(tmp_path):
    from mmt_amd import _lib
    fields = [f for f, _ in _lib.DepthParams._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HEADER, "int main(void){",
           'printf("%zu\\n", sizeof(mmt_depth_params));']
    src += ['printf("%%zu\\n", offsetof(mmt_depth_params, %s));' % f for f in fields]
    src += ["return 0;}"]
    c = tmp_path / "abi.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", str(c), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out[0] == ctypes.sizeof(_lib.DepthParams)
    assert out[1:] == [getattr(_lib.DepthParams, f).offset for f in fields]


def test_depth_prepare_rejects_bad_args_before_any_launch():
    from mmt_amd._lib import LIB, DepthParams
    fake = 1 << 20  # aligned, never dereferenced: every call below is rejected on the host

    def host(n=1, **kw):
        arr = (DepthParams * 5)()
        for p in arr:
            p.depth, p.H, p.W, p.out, p.work, p.record = fake, 4, 4, fake, fake, fake
            for k, v in kw.items():
                setattr(p, k, v)
        return LIB.mmt_depth_prepare(arr, n, None)

    assert LIB.mmt_depth_prepare(None, 1, None) == EBADARG
    assert host(n=0) == EBADARG and host(n=-1) == EBADARG and host(n=5) == EBADARG  # > MMT_MAX_CROPS
    assert host(depth=None) == EBADARG and host(out=None) == EBADARG and host(work=None) == EBADARG
    assert host(H=0) == EBADARG and host(W=0) == EBADARG and host(H=-2) == EBADARG
    assert host(H=65536, W=65536) == EBADARG  # H * W = 2^32: the counts are uint32
    assert host(depth=fake + 1) == EBADARG and host(work=fake + 2) == EBADARG and host(record=fake + 1) == EBADARG
    tab = (DepthParams * 2)()
    p = ctypes.addressof(tab)
    assert LIB.mmt_depth_prepare_table(None, None, 2, None) == EBADARG
    assert LIB.mmt_depth_prepare_table(p, None, 0, None) == EBADARG
    assert LIB.mmt_depth_prepare_table(p, None, -3, None) == EBADARG
    assert LIB.mmt_depth_prepare_table(p, None, 65536, None) == EBADARG


def test_torch_op_registered_with_fake_kernel():
    from mmt_amd import ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert hasattr(torch.ops.mmt, "depth_prepare")
    with FakeTensorMode():
        out, rec = torch.ops.mmt.depth_prepare(torch.empty(36, 64, dtype=torch.int16))
        assert out.shape == (36, 64, 3) and out.dtype == torch.uint8
        assert rec.shape == (7,) and rec.dtype == torch.int32
    with pytest.raises(RuntimeError):  # no CPU path
        torch.ops.mmt.depth_prepare(torch.zeros(4, 4, dtype=torch.int16))


# ------------------------------------------------------------------ refusals
def test_depth_frame_refusals():
    from mmt_amd.depth import as_depth16, depth_to_3xd, prepare_depth
    with pytest.raises(ValueError, match="must be uint16"):
        as_depth16(np.zeros((4, 4), np.uint8))
    with pytest.raises(ValueError, match="must be uint16"):
        as_depth16(torch.zeros(4, 4, dtype=torch.float32))
    with pytest.raises(ValueError, match=r"must be \(H, W\)"):
        as_depth16(np.zeros((4, 4, 3), np.uint16))
    with pytest.raises(ValueError, match=r"must be \(H, W\)"):
        as_depth16(torch.zeros(4, 4, 1, dtype=torch.int16))
    with pytest.raises(ValueError, match="uint16"):
        depth_to_3xd(np.zeros((4, 4), np.int32))
    with pytest.raises(ValueError, match="device tensor"):
        prepare_depth(torch.zeros(4, 4, dtype=torch.int16))
    # uint16 and int16 (the same bits) are both taken, without a copy of the values
    d = np.array([[0, 40000], [65535, 7]], np.uint16)
    for x in (d, torch.from_numpy(d.view(np.int16)), torch.from_numpy(d.view(np.int16)).view(torch.uint16)):
        t = as_depth16(x)
        assert t.dtype == torch.int16 and np.array_equal(t.numpy().view(np.uint16), d)


def test_check_depth_frame_size_mismatch_names_the_expected_shape():
    from mmt_amd.tracking import check_depth_frame
    rgb = np.zeros((36, 64, 3), np.uint8)
    assert tuple(check_depth_frame(np.zeros((36, 64), np.uint16), 36, 64).shape) == (36, 64)
    with pytest.raises(ValueError, match=r"\(36, 64\)"):
        check_depth_frame(np.zeros((64, 36), np.uint16), *rgb.shape[:2])
    with pytest.raises(ValueError, match="must be uint16"):
        check_depth_frame(np.zeros((36, 64), np.uint8), 36, 64)
    with pytest.raises(ValueError, match=r"must be \(H, W\)"):
        check_depth_frame(np.zeros((36, 64, 3), np.uint16), 36, 64)


def test_cores_refuse_an_unknown_aux_format():
    from mmt_amd.tracking import RGBTBatchTrackerCore, RGBTTrackerCore
    net = SimpleNamespace(online_size=1)
    args = (2.0, 128, 5.0, 320, [2], True)
    with pytest.raises(ValueError, match="aux_format"):
        RGBTTrackerCore(net, *args, aux_format="depth8")
    with pytest.raises(ValueError, match="aux_format"):
        RGBTBatchTrackerCore(net, *args, slots=2, aux_format="rgbd")


@pytest.mark.parametrize("module", MODULES)
def test_tracker_modules_read_aux_format(module):
    """params.aux_format is checked before the network is built, in single and batched form; without it the
    default "rgb8" passes (the construction then gets as far as the next check, made to fail here)."""
    from lib.test.tracker._rgbt import _aux_format
    assert _aux_format(SimpleNamespace()) == "rgb8" and _aux_format(SimpleNamespace(aux_format="depth16")) == "depth16"
    mod = importlib.import_module("lib.test.tracker." + module)
    for make in (lambda p: mod.get_tracker_class()(p, "x"), lambda p: mod.get_batch_tracker_class()(p, "x", 2)):
        with pytest.raises(ValueError, match="aux_format"):
            make(SimpleNamespace(aux_format="png"))
        for ok in (SimpleNamespace(online_size=0), SimpleNamespace(online_size=0, aux_format="rgb8"),
                   SimpleNamespace(online_size=0, aux_format="depth16")):
            with pytest.raises(ValueError, match="online_size"):
                make(ok)
