"""mmt_depth_prepare / mmt_depth_prepare_table (csrc/depth.hip) on the GPU against mmt_amd.depth.depth_to_3xd.

Every case compares the record (s[k0], s[k1], capi, smin, smax exactly, a and b bitwise) and the whole output
frame; the output frame and the workspace sit between guard bytes of 0xA5 that must stay intact.  The frames pin
the selection (ranks in one or two high-byte buckets, most pixels in one bin), the cap (fractional, the 10 000
limit, nothing clipped, everything clipped) and the affine (scale 0, exact products, exact rounding ties in both
directions); the shapes cover one pixel, odd and even n, sizes that are no multiple of a vector or a block's
stride, and pointers that are not 16-byte aligned."""
import numpy as np
import pytest
import torch

from depth_probes import (EVEN_MULTI_BLOCK, FRAMES, SHAPES, f_255_256, f_90pct_zero, f_all_equal, f_all_far,
                          f_all_zero, f_cap_10000, f_fractional_cap, f_gamma, f_majority_zero, f_range_255, f_range_3,
                          f_range_510, f_two_buckets, f_with_65535)
from depth_probes import frame as _frame

pytestmark = pytest.mark.gpu

GUARD = 256  # bytes, a multiple of 16
G = 0xA5


# ------------------------------------------------------------------------------------------- buffers
class _Entry:
    """One frame's device buffers: depth, and out / work / record between guard bytes.  depth_off (elements) and
    out_off (bytes) shift the pointers off their 16-byte alignment."""

    def __init__(self, d, depth_off=0, out_off=0, capacity=None):
        self.set_host(d)
        cap = d.size if capacity is None else capacity
        self.depth_off, self.out_off = depth_off, out_off
        self.depth = torch.zeros(cap + 8, dtype=torch.int16, device="cuda")
        self.out = torch.full((2 * GUARD + 16 + cap * 3,), G, dtype=torch.uint8, device="cuda")
        self.work = torch.full((2 * GUARD + 4096,), G, dtype=torch.uint8, device="cuda")
        self.record = torch.full((2 * GUARD // 4 + 7,), -1, dtype=torch.int32, device="cuda")
        self.upload()

    def set_host(self, d):
        self.d = np.ascontiguousarray(d, dtype=np.uint16)
        self.H, self.W = d.shape

    def upload(self):
        n = self.d.size
        self.depth[self.depth_off:self.depth_off + n].copy_(torch.from_numpy(self.d.reshape(-1).view(np.int16)))

    def params(self, **override):
        from mmt_amd._lib import DepthParams
        p = DepthParams()
        p.depth = self.depth.data_ptr() + 2 * self.depth_off
        p.H, p.W = self.H, self.W
        p.out = self.out.data_ptr() + GUARD + self.out_off
        p.work = self.work.data_ptr() + GUARD
        p.record = self.record.data_ptr() + GUARD
        for k, v in override.items():
            setattr(p, k, v)
        return p

    def got(self):
        n3 = self.d.size * 3
        lo = GUARD + self.out_off
        out = self.out.cpu()
        return out[lo:lo + n3].view(self.H, self.W, 3), self.record.cpu()[GUARD // 4:GUARD // 4 + 7].tolist()

    def guards_intact(self, n3=None):
        n3 = self.d.size * 3 if n3 is None else n3
        out, work, rec = self.out.cpu(), self.work.cpu(), self.record.cpu()
        lo = GUARD + self.out_off
        return bool((out[:lo] == G).all() and (out[lo + n3:] == G).all() and (work[:GUARD] == G).all()
                    and (work[GUARD + 4096:] == G).all() and (rec[:GUARD // 4] == -1).all()
                    and (rec[GUARD // 4 + 7:] == -1).all())

    def untouched(self):
        return self.guards_intact(0) and bool((self.work.cpu() == G).all() and (self.record.cpu() == -1).all())

    def check(self, tag=""):
        from mmt_amd.depth import depth_record, depth_to_3xd
        s0, s1, capi, smin, smax, a, b = depth_record(self.d)
        want = [s0, s1, capi, smin, smax, int(np.float32(a).view(np.int32)), int(np.float32(b).view(np.int32))]
        out, rec = self.got()
        assert rec == want, (tag, rec, want)
        assert torch.equal(out, torch.from_numpy(depth_to_3xd(self.d))), tag
        assert self.guards_intact(), tag
        return want


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _host(entries):
    from mmt_amd._lib import LIB, DepthParams, check
    arr = (DepthParams * len(entries))(*[e.params() for e in entries])
    check(LIB.mmt_depth_prepare(arr, len(entries), _stream()), "mmt_depth_prepare")
    torch.cuda.synchronize()


def _table(params, enable=None):
    from mmt_amd._lib import DepthParams
    arr = (DepthParams * len(params))(*params)
    tab = torch.frombuffer(arr, dtype=torch.uint8).cuda()
    en = torch.tensor(enable, dtype=torch.uint8).cuda() if enable is not None else None
    return tab, en


def _launch_table(tab, en, n):
    from mmt_amd._lib import LIB, check
    check(LIB.mmt_depth_prepare_table(tab.data_ptr(), en.data_ptr() if en is not None else None, n, _stream()),
          "mmt_depth_prepare_table")
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- host form
@pytest.mark.parametrize("make", FRAMES, ids=lambda f: f.__name__[2:])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_depth_prepare_equals_host_restatement(shape, make):
    H, W = shape
    e = _Entry(_frame(make, H, W))
    _host([e])
    s0, s1, capi, smin, smax, a_bits, b_bits = e.check((shape, make.__name__))
    n = H * W
    a = np.int32(a_bits).view(np.float32)
    out = e.got()[0]
    if make in (f_all_equal, f_all_zero, f_all_far, f_majority_zero):
        assert smax == smin and a == 0.0 and not out.any()
    if make is f_majority_zero:
        assert (s0, s1, capi) == (0, 0, 0)
    if make is f_all_far:
        assert (capi, smin, smax) == (10000, 10000, 10000)
    if n >= 8:
        if make in (f_255_256, f_two_buckets) and n % 2 == 0:
            assert (s0, s1, capi) == (255, 256, 766)
        if make is f_fractional_cap:
            assert (s0, s1, capi) == ((100, 101, 301) if n % 2 == 0 else (101, 101, 303)) and smax == capi
        if make is f_cap_10000:
            assert capi == 10000 and 3 * (s0 + s1) > 20000 and smax == 10000
        if make is f_with_65535:
            assert int(e.d.max()) == 65535 and smax == capi < 65535
        if make is f_90pct_zero:
            assert capi == 0
        if make is f_range_255:
            assert a == 1.0 and smax - smin == 255
        if make is f_range_510:
            assert a == 0.5 and smax - smin == 510
            # ties round to even: offset 1 -> 0.5 -> 0, offset 3 -> 1.5 -> 2
            flat, src = out[:, :, 0].reshape(-1), torch.from_numpy((e.d.reshape(-1) - 1000).astype(np.int64))
            odd = src % 2 == 1
            assert (n < 100 or bool(odd.any())) and bool((flat[odd] % 2 == 0).all())
            assert bool((flat[src % 4 == 1].long() == (src[src % 4 == 1] - 1) // 2).all())
            assert bool((flat[src % 4 == 3].long() == (src[src % 4 == 3] + 1) // 2).all())
        if make is f_range_3:
            assert a == 85.0 and {0, 255} <= set(out.reshape(-1).tolist()) <= {0, 85, 170, 255}


def test_depth_prepare_360x640_once():
    e = _Entry(_frame(f_gamma, 360, 640))
    _host([e])
    e.check("360x640")


@pytest.mark.parametrize("shape", EVEN_MULTI_BLOCK, ids=lambda s: "%dx%d" % s)
def test_two_rank_paths_over_several_blocks(shape):
    """Even n over several blocks, where the median is the mean of two different pixels: the two ranks in different
    high-byte buckets (the second bucket's low-byte counts of every wave and block, their merge, and the second
    selection of the finalise step), and a fractional cap (301.5 -> 301) with a tenth of the frame at capi - 1,
    capi and capi + 1.  The literal values are asserted without conditions."""
    H, W = shape
    n = H * W
    assert n % 2 == 0 and n > 256 * 8
    for make in (f_255_256, f_two_buckets):
        e = _Entry(_frame(make, H, W))
        _host([e])
        s0, s1, capi, smin, smax = e.check((shape, make.__name__))[:5]
        assert (s0, s1, capi) == (255, 256, 766) and s0 >> 8 != s1 >> 8, make.__name__
        assert smax == (256 if make is f_255_256 else 300)  # nothing clipped
    e = _Entry(_frame(f_fractional_cap, H, W))
    _host([e])
    s0, s1, capi, smin, smax = e.check((shape, "fractional_cap"))[:5]
    assert (s0, s1, capi, smin, smax) == (100, 101, 301, 100, 301)
    d, out = torch.from_numpy(e.d.astype(np.int64)), e.got()[0][:, :, 0].long()
    for v in (300, 301, 302):
        assert int((d == v).sum()) >= n // 30
    assert bool((out[d >= 301] == 255).all()) and bool((out[d == 300] < 255).all()) and bool((out[d == 100] == 0).all())


def test_shapes_reach_the_two_rank_cases():
    """The parametrised cases above assert the literal two-bucket and fractional-cap records only at even n >= 8:
    such shapes, spanning several blocks, are in SHAPES."""
    even = [(H, W) for H, W in SHAPES if H * W % 2 == 0 and H * W > 256 * 8]
    assert len(even) >= 2 and set(even) <= set(EVEN_MULTI_BLOCK)


@pytest.mark.parametrize("depth_off,out_off", [(1, 0), (0, 1), (3, 5), (4, 8)])
@pytest.mark.parametrize("shape", [(37, 53), (257, 129)], ids=lambda s: "%dx%d" % s)
def test_depth_prepare_unaligned_pointers(shape, depth_off, out_off):
    """depth and out off their 16-byte alignment: the scalar head of the counting passes and the scalar form of
    the per-pixel pass."""
    H, W = shape
    for make in (f_gamma, f_range_510):
        e = _Entry(_frame(make, H, W), depth_off=depth_off, out_off=out_off)
        _host([e])
        e.check((shape, make.__name__, depth_off, out_off))


def test_depth_prepare_four_entries_one_launch():
    es = [_Entry(_frame(f, H, W)) for f, (H, W) in ((f_gamma, (37, 53)), (f_255_256, (2, 3)), (f_cap_10000, (257, 129)),
                                                   (f_range_510, (3, 5)))]
    _host(es)
    for i, e in enumerate(es):
        e.check(i)


def test_torch_op_and_prepare_depth():
    from mmt_amd import ops  # noqa: F401
    from mmt_amd.depth import depth_record, depth_to_3xd, prepare_depth
    d = _frame(f_gamma, 37, 53)
    want = torch.from_numpy(depth_to_3xd(d))
    dev = torch.from_numpy(d.view(np.int16)).cuda()
    for x in (dev, dev.view(torch.uint16)):
        out, rec = torch.ops.mmt.depth_prepare(x)
        assert torch.equal(out.cpu(), want) and rec.cpu().tolist()[:5] == list(depth_record(d)[:5])
    out = torch.empty(37, 53, 3, dtype=torch.uint8, device="cuda")
    got, _ = prepare_depth(dev, out=out)
    assert got is out and torch.equal(out.cpu(), want)
    torch.library.opcheck(torch.ops.mmt.depth_prepare.default, (dev,))


# ------------------------------------------------------------------------------------------- table form
TABLE_CASES = [(f_gamma, (37, 53)), (f_255_256, (1, 2)), (f_cap_10000, (257, 129)), (f_range_510, (3, 5)),
               (f_90pct_zero, (64, 48))]


def test_depth_prepare_table_sizes_skips_and_rewrite():
    """5 entries of different sizes in one launch, one disabled and one with a NULL depth (their out, work and
    record stay untouched); then the entries are re-sized and re-filled in device memory and the same call, with
    the same launch geometry, prepares the new frames."""
    cap = 257 * 129
    es = [_Entry(_frame(f, H, W), capacity=cap) for f, (H, W) in TABLE_CASES]
    params = [e.params() for e in es]
    params[3].depth = None
    tab, en = _table(params, [1, 0, 1, 1, 1])
    _launch_table(tab, en, 5)
    for i in (0, 2, 4):
        es[i].check(i)
    assert es[1].untouched() and es[3].untouched()
    # rewrite: other sizes (odd n, even n, one larger than before), all five live
    second = [(f_fractional_cap, (53, 37)), (f_gamma, (257, 129)), (f_range_255, (5, 3)), (f_with_65535, (129, 200)),
              (f_all_equal, (1, 1))]
    for e, (f, (H, W)) in zip(es, second):
        e.set_host(_frame(f, H, W))
        e.upload()
        e.out.fill_(G)
    from mmt_amd._lib import DepthParams
    arr = (DepthParams * 5)(*[e.params() for e in es])
    tab.copy_(torch.frombuffer(arr, dtype=torch.uint8))
    en.fill_(1)
    _launch_table(tab, en, 5)
    for i, e in enumerate(es):
        e.check(("second", i))


def test_depth_prepare_table_other_skip_rules():
    es = [_Entry(_frame(f_gamma, 9, 11)) for _ in range(6)]
    params = [es[0].params(), es[1].params(H=0), es[2].params(W=-3), es[3].params(out=None), es[4].params(work=None),
              es[5].params(H=65536, W=65536)]
    tab, _ = _table(params)
    _launch_table(tab, None, 6)  # NULL enable: every entry is considered
    es[0].check(0)
    for i in range(1, 6):
        assert es[i].untouched(), i


def test_depth_prepare_table_equals_host_form():
    hs = [_Entry(_frame(f, H, W)) for f, (H, W) in TABLE_CASES[:4]]
    ts = [_Entry(_frame(f, H, W)) for f, (H, W) in TABLE_CASES[:4]]
    _host(hs)
    tab, _ = _table([e.params() for e in ts])
    _launch_table(tab, None, 4)
    for h, t in zip(hs, ts):
        (ho, hr), (to, tr) = h.got(), t.got()
        assert hr == tr and torch.equal(ho, to)
        t.check()


def test_depth_prepare_bad_arguments_launch_nothing():
    from mmt_amd._lib import LIB, DepthParams
    e = _Entry(_frame(f_gamma, 9, 11))
    bad = -10000

    def host(n=1, **kw):
        arr = (DepthParams * 5)(*[e.params(**kw)] * 5)
        return LIB.mmt_depth_prepare(arr, n, _stream())

    assert LIB.mmt_depth_prepare(None, 1, _stream()) == bad
    assert host(n=0) == bad and host(n=5) == bad
    assert host(depth=None) == bad and host(out=None) == bad and host(work=None) == bad
    assert host(H=0) == bad and host(W=-1) == bad and host(H=65536, W=65536) == bad
    assert host(depth=e.depth.data_ptr() + 1) == bad and host(work=e.work.data_ptr() + GUARD + 2) == bad
    tab, _ = _table([e.params()])
    assert LIB.mmt_depth_prepare_table(None, None, 1, _stream()) == bad
    assert LIB.mmt_depth_prepare_table(tab.data_ptr(), None, 0, _stream()) == bad
    assert LIB.mmt_depth_prepare_table(tab.data_ptr(), None, -2, _stream()) == bad
    torch.cuda.synchronize()
    assert e.untouched()
