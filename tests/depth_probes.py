"""Depth frames for the RGB-D input tests (tests/test_depth_host.py, tests/test_gpu_depth_probes.py): each maker
returns a (H, W) uint16 frame that pins one property of the preparation (mmt_amd/depth.py), at any shape."""
import numpy as np

# n = 1, 2, 6, 15; 37x53 and 257x129 odd and no multiple of a vector or a block's stride; 38x54 and 256x130 the same
# sizes with an even n (the median is a mean of two pixels: the two-rank paths) over several blocks
SHAPES = [(1, 1), (1, 2), (2, 3), (3, 5), (37, 53), (38, 54), (257, 129), (256, 130)]
EVEN_MULTI_BLOCK = [(38, 54), (256, 130), (360, 640)]  # even n, more than one block's stride of pixels


def _shuffled(vals, H, W, rng):
    return rng.permutation(np.asarray(vals, dtype=np.uint16)).reshape(H, W)


def _ends(v, lo, hi):
    """Make sure both ends of a value range occur (frames of two pixels or more)."""
    if v.size >= 2:
        v.reshape(-1)[0], v.reshape(-1)[-1] = lo, hi
    return v


def f_all_equal(H, W, rng):
    return np.full((H, W), 1234, np.uint16)


def f_all_zero(H, W, rng):
    return np.zeros((H, W), np.uint16)


def f_all_far(H, W, rng):  # every pixel above the 10 000 limit: all clipped, smin == smax == 10000
    return np.full((H, W), 60000, np.uint16)


def f_majority_zero(H, W, rng):  # median 0, cap 0, output all 0
    n = H * W
    v = np.zeros(n, np.uint16)
    pos = (n - 1) // 2  # fewer than half
    v[:pos] = rng.integers(1, 5000, pos)
    return _shuffled(v, H, W, rng)


def f_255_256(H, W, rng):  # even n: ranks k0 and k1 in different high-byte buckets, capi 766
    n = H * W
    return _shuffled([255] * (n // 2) + [256] * (n - n // 2), H, W, rng)


def f_fractional_cap(H, W, rng):  # even n: median 100.5, cap 301.5 -> 301; pixels at capi - 1, capi, capi + 1
    from mmt_amd.depth import depth_cap
    n = H * W
    v = [100] * (n // 2) + [101] * (n - n // 2)
    if n >= 8:  # a tenth of the frame (three pixels at least) around the cap, all from the upper half
        capi = depth_cap(v[(n - 1) // 2], v[n // 2])
        cnt = max(3, n // 10)
        v[-cnt:] = [capi - 1 + j % 3 for j in range(cnt)]
    return _shuffled(v, H, W, rng)


def f_two_buckets(H, W, rng):  # even n: the lower half spread over 200..255, the upper over 256..300; capi 766
    n = H * W
    lo, hi = rng.integers(200, 256, n // 2), rng.integers(256, 301, n - n // 2)
    if n >= 2:
        lo[0], hi[0] = 255, 256
    return _shuffled(np.concatenate([lo, hi]), H, W, rng)


def f_cap_10000(H, W, rng):  # 3 * median > 10000
    v = rng.integers(4000, 9000, H * W)
    v[::5] = rng.integers(9990, 30000, v[::5].size)
    return _shuffled(v, H, W, rng)


def f_with_65535(H, W, rng):
    v = rng.integers(300, 2000, H * W)
    v[::7] = 65535
    return _shuffled(v, H, W, rng)


def f_90pct_zero(H, W, rng):
    v = rng.integers(1, 3000, H * W)
    v[rng.random(H * W) < 0.9] = 0
    return v.astype(np.uint16).reshape(H, W)


def f_range_255(H, W, rng):  # a == 1: every product exact
    return _ends(rng.integers(1000, 1256, (H, W)).astype(np.uint16), 1000, 1255)


def f_range_510(H, W, rng):  # a == 0.5: odd offsets are exact ties, half of them round down, half up
    return _ends(rng.integers(1000, 1511, (H, W)).astype(np.uint16), 1000, 1510)


def f_range_3(H, W, rng):  # a == 85
    return _ends(rng.integers(500, 504, (H, W)).astype(np.uint16), 500, 503)


def f_gamma(H, W, rng):  # what depth frames look like: a gamma-distributed range with 10 % holes
    v = np.minimum(rng.gamma(2.0, 900.0, (H, W)), 65535).astype(np.uint16)
    v[rng.random((H, W)) < 0.1] = 0
    return v


FRAMES = [f_all_equal, f_all_zero, f_all_far, f_majority_zero, f_255_256, f_fractional_cap, f_cap_10000, f_with_65535,
          f_90pct_zero, f_range_255, f_range_510, f_range_3, f_gamma, f_two_buckets]


def frame(make, H, W):
    return make(H, W, np.random.default_rng(1000 * H + W + 17 * FRAMES.index(make)))
