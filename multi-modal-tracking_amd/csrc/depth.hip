// RGB-D input: a raw 16-bit depth frame prepared on the GPU into the tracker's second-modality frame.
//
//   mmt_depth_prepare / mmt_depth_prepare_table
//       the reference's per-frame host preparation of DepthTrack depth frames
//       (lib/test/evaluation/depth_utils.py:17-22, :55-60 with dtype="rgb3d", depth_clip=True): clip at
//       min(3 * median, 10000), cv2.normalize(NORM_MINMAX, 0..255), uint8, replicate to three channels.
//       mmt_amd/depth.py:depth_to_3xd restates it in numpy; both are bit-exact to each other.
//
// The median is an exact selection over all n = H * W pixels by integer counts (two-level radix):
//   depth_clear_kernel     zeroes the entry's 4 KiB workspace (a launch of the sequence: capturable)
//   depth_hist_kernel      256-bin histogram of the high byte, per wave in LDS, merged per block into the
//                          workspace's uint32 bins; min and max of the frame in the same pass
//   depth_count_kernel     every block finds the buckets of the ranks k0 = (n-1)/2 and k1 = n/2 from the bins
//                          (one wave, prefix sums), then counts the low bytes inside those one or two buckets
//   depth_finalise_kernel  one wave per entry: s[k0], s[k1], the cap, smin / smax, and the affine's a and b from
//                          float64 arithmetic; writes the record
//   depth_apply_kernel     clip, float32 d * a + b (two roundings: contraction is off in this file), round half to
//                          even, saturate, low 8 bits, three equal channels
// Counts are integers, so the result does not depend on the order the atomics arrive in.  Every grid is
// (DEPTH_BLOCKS, n entries) with grid-stride loops over H * W: nothing depends on the frame size or contents.
// cv2 is not part of this image: the normalize step restates OpenCV's conventions (float32 src * a + b,
// saturate_cast rounding to nearest-even) and has not been run against OpenCV.
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int DEPTH_BLOCKS = 64;  // workgroups per entry in the three pixel passes
constexpr int NT = 256;

// workspace layout, uint32 words (MMT_DEPTH_WORK_BYTES = 4096)
constexpr int W_HI = 0;      // [256] high-byte histogram
constexpr int W_LO = 256;    // [2][256] low-byte counts inside the buckets of ranks k0 and k1 (the second unused when equal)
constexpr int W_INVMIN = 768;  // max of (65535 - d): zero-initialised like the rest
constexpr int W_MAX = 769;
constexpr int W_SEL = 770;   // bucket of k0, rank of k0 inside it, bucket of k1, rank of k1 inside it
constexpr int W_CAP = 774;   // capi, float bits of a, float bits of b
constexpr int W_WORDS = 1024;
static_assert(W_WORDS * 4 == MMT_DEPTH_WORK_BYTES, "workspace layout");

struct DepthBatch {
    mmt_depth_params c[MMT_MAX_CROPS];
};

// The entry of block row e: from the by-value batch (host form) or the device table.  Every condition the host
// form rejects makes the entry dead here, before any store.
MMT_DEV bool load_entry(const DepthBatch& cb, const mmt_depth_params* __restrict__ table,
                        const uint8_t* __restrict__ enable, int e, mmt_depth_params& p) {
    if (table) {
        p = table[e];
        if (enable && !enable[e]) return false;
    } else {
        p = cb.c[e];
    }
    if (!p.depth || !p.out || !p.work || p.H <= 0 || p.W <= 0) return false;
    if (((uintptr_t)p.depth & 1) || ((uintptr_t)p.work & 3) || ((uintptr_t)p.record & 3)) return false;
    return (int64_t)p.H * p.W < ((int64_t)1 << 32);
}

MMT_DEV int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// A run of equal bins inside one thread's pixels becomes one LDS add: depth frames have 10-30 % of their pixels at
// exactly 0, mostly in runs, so the bin of 0 would otherwise take one add per pixel.
struct RunAdder {
    uint32_t* h;
    int cur, cnt;
    MMT_DEV explicit RunAdder(uint32_t* hist) : h(hist), cur(-1), cnt(0) {}
    MMT_DEV void add(int bin) {
        if (bin == cur) {
            ++cnt;
            return;
        }
        flush();
        cur = bin;
        cnt = 1;
    }
    MMT_DEV void flush() {
        if (cur >= 0 && cnt) atomicAdd(&h[cur], (uint32_t)cnt);
        cnt = 0;
    }
};

// Pixels [0, n) of `d` split for 16-byte loads: `head` pixels up to the first 16-byte boundary, nv vectors of 8,
// then the tail.  f(pixel value) is called once per pixel, by exactly one thread of the entry's DEPTH_BLOCKS blocks.
template <typename F>
MMT_DEV void for_each_pixel(const uint16_t* __restrict__ d, int64_t n, F&& f) {
    const int64_t gid = (int64_t)blockIdx.x * NT + threadIdx.x, total = (int64_t)DEPTH_BLOCKS * NT;
    int64_t head = ((16 - ((uintptr_t)d & 15)) & 15) >> 1;
    if (head > n) head = n;
    const int64_t nv = (n - head) >> 3, tail0 = head + nv * 8;
    if (gid < head) f((int)d[gid]);
    const uint4* __restrict__ v = (const uint4*)(d + head);
    for (int64_t i = gid; i < nv; i += total) {
        const uint4 q = v[i];
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f((int)(w[j] & 0xffffu));
            f((int)(w[j] >> 16));
        }
    }
    if (gid < n - tail0) f((int)d[tail0 + gid]);
}

__global__ __launch_bounds__(NT) void depth_clear_kernel(const DepthBatch cb, const mmt_depth_params* __restrict__ table,
                                                         const uint8_t* __restrict__ enable) {
    mmt_depth_params p;
    if (!load_entry(cb, table, enable, blockIdx.x, p)) return;
    uint32_t* w = (uint32_t*)p.work;
    for (int i = threadIdx.x; i < W_WORDS; i += NT) w[i] = 0u;
}

__global__ __launch_bounds__(NT) void depth_hist_kernel(const DepthBatch cb, const mmt_depth_params* __restrict__ table,
                                                        const uint8_t* __restrict__ enable) {
    __shared__ uint32_t hist[NT / 64][256];
    __shared__ int red[2][NT / 64];
    mmt_depth_params p;
    if (!load_entry(cb, table, enable, blockIdx.y, p)) return;  // uniform over the block
    const int t = threadIdx.x, wv = t >> 6;
#pragma unroll
    for (int k = 0; k < NT / 64; ++k) hist[k][t] = 0u;
    __syncthreads();
    int mn = 65535, mx = 0;
    RunAdder run(hist[wv]);
    for_each_pixel(p.depth, (int64_t)p.H * p.W, [&](int v) {
        mn = min(mn, v);
        mx = max(mx, v);
        run.add(v >> 8);
    });
    run.flush();
    mx = wave_max_i(mx);
    const int inv = wave_max_i(65535 - mn);
    if ((t & 63) == 0) red[0][wv] = mx, red[1][wv] = inv;
    __syncthreads();
    uint32_t* w = (uint32_t*)p.work;
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < NT / 64; ++k) c += hist[k][t];
    if (c) atomicAdd(&w[W_HI + t], c);
    if (t == 0) {
        int a = 0, b = 0;
#pragma unroll
        for (int k = 0; k < NT / 64; ++k) a = max(a, red[0][k]), b = max(b, red[1][k]);
        atomicMax(&w[W_MAX], (uint32_t)a);
        atomicMax(&w[W_INVMIN], (uint32_t)b);
    }
}

// One wave: the bin of `bins[256]` that holds rank k (0-based, in ascending bin order) and k's rank inside that
// bin.  The bins sum to more than k.  Every lane returns the same pair.
MMT_DEV void wave_select(const uint32_t* __restrict__ bins, uint32_t k, int lane, int& bin, uint32_t& within) {
    uint32_t c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = bins[4 * lane + j];
    const uint32_t s = c[0] + c[1] + c[2] + c[3];
    uint32_t incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(incl, o, 64);
        if (lane >= o) incl += u;
    }
    uint32_t excl = incl - s;
    const bool mine = k >= excl && k < incl;  // at most one lane
    int b = 0;
    uint32_t r = 0;
    if (mine) {
        bool found = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!found) {
                if (k < excl + c[j]) {
                    b = 4 * lane + j;
                    r = k - excl;
                    found = true;
                } else {
                    excl += c[j];
                }
            }
        }
    }
    const unsigned long long m = __ballot(mine);
    const int src = m ? __ffsll((long long)m) - 1 : 0;
    bin = __shfl(b, src, 64);
    within = __shfl(r, src, 64);
}

__global__ __launch_bounds__(NT) void depth_count_kernel(const DepthBatch cb, const mmt_depth_params* __restrict__ table,
                                                         const uint8_t* __restrict__ enable) {
    __shared__ uint32_t hist[NT / 64][512];
    __shared__ int sel[2];
    mmt_depth_params p;
    if (!load_entry(cb, table, enable, blockIdx.y, p)) return;
    const int t = threadIdx.x, wv = t >> 6;
    uint32_t* w = (uint32_t*)p.work;
    const int64_t n = (int64_t)p.H * p.W;
#pragma unroll
    for (int k = 0; k < NT / 64; ++k) hist[k][t] = 0u, hist[k][256 + t] = 0u;
    if (wv == 0) {
        int b0, b1;
        uint32_t r0, r1;
        wave_select(w + W_HI, (uint32_t)((n - 1) >> 1), t, b0, r0);
        wave_select(w + W_HI, (uint32_t)(n >> 1), t, b1, r1);
        if (t == 0) {
            sel[0] = b0, sel[1] = b1;
            if (blockIdx.x == 0) w[W_SEL] = b0, w[W_SEL + 1] = r0, w[W_SEL + 2] = b1, w[W_SEL + 3] = r1;
        }
    }
    __syncthreads();
    const int b0 = sel[0], b1 = sel[1];
    RunAdder run(hist[wv]);
    for_each_pixel(p.depth, n, [&](int v) {
        const int hi = v >> 8;
        run.add(hi == b0 ? (v & 255) : (hi == b1 ? 256 + (v & 255) : -1));
    });
    run.flush();
    __syncthreads();
    uint32_t c0 = 0, c1 = 0;
#pragma unroll
    for (int k = 0; k < NT / 64; ++k) c0 += hist[k][t], c1 += hist[k][256 + t];
    if (c0) atomicAdd(&w[W_LO + t], c0);
    if (c1) atomicAdd(&w[W_LO + 256 + t], c1);
}

__global__ __launch_bounds__(64) void depth_finalise_kernel(const DepthBatch cb, const mmt_depth_params* __restrict__ table,
                                                            const uint8_t* __restrict__ enable) {
    mmt_depth_params p;
    if (!load_entry(cb, table, enable, blockIdx.x, p)) return;
    uint32_t* w = (uint32_t*)p.work;
    const int lane = threadIdx.x;
    const int b0 = (int)w[W_SEL], b1 = (int)w[W_SEL + 2];
    const uint32_t r0 = w[W_SEL + 1], r1 = w[W_SEL + 3];
    int l0, l1;
    uint32_t unused;
    wave_select(w + W_LO, r0, lane, l0, unused);
    wave_select(w + W_LO + (b1 == b0 ? 0 : 256), r1, lane, l1, unused);
    if (lane != 0) return;
    const int s0 = b0 * 256 + l0, s1 = b1 * 256 + l1;
    const int capi = min((3 * (s0 + s1)) >> 1, 10000);  // trunc(min(3 * (s0 + s1) / 2, 10000.0))
    const int dmin = 65535 - (int)w[W_INVMIN], dmax = (int)w[W_MAX];
    const int smin = min(dmin, capi), smax = min(dmax, capi);  // min / max of the clipped frame
    // cv2.normalize(NORM_MINMAX, 0, 255): float64, then float32 a and b for the per-pixel pass
    const double span = (double)smax - (double)smin;
    const double scale = 255.0 * (span > 2.220446049250313e-16 ? 1.0 / span : 0.0);
    const double shift = 0.0 - (double)smin * scale;
    const float a = (float)scale, b = (float)shift;
    w[W_CAP] = (uint32_t)capi;
    w[W_CAP + 1] = __float_as_uint(a);
    w[W_CAP + 2] = __float_as_uint(b);
    if (p.record) {
        p.record[0] = s0;
        p.record[1] = s1;
        p.record[2] = capi;
        p.record[3] = smin;
        p.record[4] = smax;
        p.record[5] = (int32_t)__float_as_uint(a);
        p.record[6] = (int32_t)__float_as_uint(b);
    }
}

// saturate_cast<ushort>(cvRound(float32(d') * a + b)) & 255: the product and the sum round separately
MMT_DEV uint32_t depth_px(uint32_t v, uint32_t capi, float a, float b) {
    const uint32_t c = v > capi ? capi : v;
    // Two roundings, never one fma.  The file-scope `#pragma clang fp contract(off)` gives that under hipcc's default
    // (-ffp-contract=fast-honor-pragmas) but NOT under a plain -ffp-contract=fast on the command line, which fuses
    // across the pragma (checked in the disassembly); and __fmul_rn / __fadd_rn do not help either: they are header
    // inlines compiled under the default contraction and were fused after inlining.  So the product also passes
    // through an empty asm that the optimiser cannot see through: no flag can fuse it with the add.
    float prod = (float)c * a;
    asm volatile("" : "+v"(prod));
    const float r = rintf(prod + b);  // rintf: round half to even
    const int q = r < 0.f ? 0 : (r > 65535.f ? 65535 : (int)r);
    return (uint32_t)q & 255u;
}

__global__ __launch_bounds__(NT) void depth_apply_kernel(const DepthBatch cb, const mmt_depth_params* __restrict__ table,
                                                         const uint8_t* __restrict__ enable) {
    mmt_depth_params p;
    if (!load_entry(cb, table, enable, blockIdx.y, p)) return;
    const uint32_t* w = (const uint32_t*)p.work;
    const uint32_t capi = w[W_CAP];
    const float a = __uint_as_float(w[W_CAP + 1]), b = __uint_as_float(w[W_CAP + 2]);
    const int64_t n = (int64_t)p.H * p.W;
    const int64_t gid = (int64_t)blockIdx.x * NT + threadIdx.x, total = (int64_t)DEPTH_BLOCKS * NT;
    const uint16_t* __restrict__ d = p.depth;
    uint8_t* __restrict__ o = p.out;
    int64_t done = 0;
    if ((((uintptr_t)d | (uintptr_t)o) & 15) == 0) {
        // 16 pixels: two 16-byte loads, 48 output bytes = three 16-byte stores
        const int64_t nc = n >> 4;
        const uint4* __restrict__ src = (const uint4*)d;
        uint4* __restrict__ dst = (uint4*)o;
        for (int64_t i = gid; i < nc; i += total) {
            const uint4 q0 = src[2 * i], q1 = src[2 * i + 1];
            const uint32_t in[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
            uint32_t px[16];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                px[2 * j] = depth_px(in[j] & 0xffffu, capi, a, b);
                px[2 * j + 1] = depth_px(in[j] >> 16, capi, a, b);
            }
            uint32_t ow[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) {  // output byte 4 k + j is pixel (4 k + j) / 3
                ow[k] = px[(4 * k) / 3] | (px[(4 * k + 1) / 3] << 8) | (px[(4 * k + 2) / 3] << 16) | (px[(4 * k + 3) / 3] << 24);
            }
            dst[3 * i] = uint4{ow[0], ow[1], ow[2], ow[3]};
            dst[3 * i + 1] = uint4{ow[4], ow[5], ow[6], ow[7]};
            dst[3 * i + 2] = uint4{ow[8], ow[9], ow[10], ow[11]};
        }
        done = nc << 4;
    }
    for (int64_t i = done + gid; i < n; i += total) {  // the scalar tail, or a frame that is not 16-byte aligned
        const uint8_t v = (uint8_t)depth_px(d[i], capi, a, b);
        o[3 * i] = v;
        o[3 * i + 1] = v;
        o[3 * i + 2] = v;
    }
}

int launch_all(const DepthBatch& cb, const mmt_depth_params* table, const uint8_t* enable, int n, hipStream_t st) {
    const dim3 per_entry(n), pixels(DEPTH_BLOCKS, n);
    hipLaunchKernelGGL(depth_clear_kernel, per_entry, dim3(NT), 0, st, cb, table, enable);
    hipLaunchKernelGGL(depth_hist_kernel, pixels, dim3(NT), 0, st, cb, table, enable);
    hipLaunchKernelGGL(depth_count_kernel, pixels, dim3(NT), 0, st, cb, table, enable);
    hipLaunchKernelGGL(depth_finalise_kernel, per_entry, dim3(64), 0, st, cb, table, enable);
    hipLaunchKernelGGL(depth_apply_kernel, pixels, dim3(NT), 0, st, cb, table, enable);
    return launch_status();
}

}  // namespace

extern "C" int mmt_depth_prepare(const mmt_depth_params* p, int n, void* stream) {
    if (!p || n <= 0 || n > MMT_MAX_CROPS) return MMT_EBADARG;
    DepthBatch cb = {};
    for (int i = 0; i < n; ++i) {
        const mmt_depth_params& c = p[i];
        if (!c.depth || !c.out || !c.work || c.H <= 0 || c.W <= 0) return MMT_EBADARG;
        if ((int64_t)c.H * c.W >= ((int64_t)1 << 32)) return MMT_EBADARG;  // uint32 counts
        if (((uintptr_t)c.depth & 1) || ((uintptr_t)c.work & 3) || ((uintptr_t)c.record & 3)) return MMT_EBADARG;
        cb.c[i] = c;
    }
    return launch_all(cb, nullptr, nullptr, n, (hipStream_t)stream);
}

extern "C" int mmt_depth_prepare_table(const mmt_depth_params* table_dev, const uint8_t* enable_dev, int n, void* stream) {
    if (!table_dev || n <= 0 || n > 65535) return MMT_EBADARG;  // the entry index is the grid's y
    if ((uintptr_t)table_dev & 7) return MMT_EBADARG;
    const DepthBatch cb = {};
    return launch_all(cb, table_dev, enable_dev, n, (hipStream_t)stream);
}
