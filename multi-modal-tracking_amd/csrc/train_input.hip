// Training input on the GPU: the per-sample pixel passes of the reference's MixformerProcessing
// (lib/train/data/processing_rgbt.py:143-228 with the transform chain of
// lib/train/base_functions.py:177-183), one launch per output size.
//
//   mmt_train_crops_table   per table entry: the joint grayscale / flip of the full frame (applied to the
//                           source taps, the frame stays as stored), sample_target's crop / zero padding /
//                           cv2.resize, the brightness jitter (RGB: on the float tensor; TIR: on uint8
//                           before the JET map), the crop's own flip, the ImageNet normalise, and the
//                           attention mask (ones on padding through cv2.resize's float path, != 0).
//
// The crop geometry, the resize and the colour map are crop_common.hpp's, shared with the tracker's
// mmt_sample_target*: the same bits.  What differs from the tracker's kernel is the arithmetic after the
// resize, which here is torch's on CPU tensors (transforms_rgbt.py:221-243): x.float().mul(bf / 255.0)
// for RGB -- one product with the float32 scalar -- and x.float().div(255.0) for TIR -- a true division,
// not the GPU tensor's multiply by the reciprocal.  mmt_amd/train_input.py restates all of it on the
// host; kernel and restatement are bit-exact to each other.
#include "crop_common.hpp"

// Parity is bit-exact against separately rounded torch / numpy / Python ops: no FMA contraction.
#pragma clang fp contract(off)

namespace {

// padded crop pixel (row r, col c) of the jointly transformed frame, three channels: column ix of the
// mirrored frame is stored column W - 1 - ix; gray is cvtColor(COLOR_RGB2GRAY) replicated
MMT_DEV Px3 src_px(const mmt_train_crop_params& p, const Geo& g, int r, int c) {
    const int iy = g.y1 + r, ix = g.x1 + c;
    if (iy < 0 || ix < 0 || iy >= g.ylim || ix >= g.xlim) return Px3{{0, 0, 0}};
    const int sx = p.src_flip ? p.W - 1 - ix : ix;
    const uint8_t* q = p.image + ((int64_t)iy * p.W + sx) * 3;
    Px3 v{{q[0], q[1], q[2]}};
    if (p.src_gray) v.v[0] = v.v[1] = v.v[2] = (v.v[0] * 4899 + v.v[1] * 9617 + v.v[2] * 1868 + (1 << 13)) >> 14;
    return v;
}

MMT_DEV bool row_pad(const Geo& g, int r) { return g.y1 + r < 0 || g.y1 + r >= g.ylim; }
MMT_DEV bool col_pad(const Geo& g, int c) { return g.x1 + c < 0 || g.x1 + c >= g.xlim; }

// cv2.resize of the float mask (ones on padding) != 0: the mask is rows OR columns, every weight is
// >= 0, so the resized value is non-zero iff a tap of non-zero weight lies on padding.  The first tap's
// weight 1 - f is never 0 (f < 1); the second tap's is f.
MMT_DEV int att_pixel(const Geo& g, int os, int dy, int dx) {
    if (g.crop < 1) return 1;
    const double inv = (double)os / g.crop, scale = 1.0 / inv;
    if (is_area2(scale))
        return row_pad(g, 2 * dy) || row_pad(g, 2 * dy + 1) || col_pad(g, 2 * dx) || col_pad(g, 2 * dx + 1);
    const Taps tx = linear_taps(dx, scale, g.crop, true), ty = linear_taps(dy, scale, g.crop, false);
    return row_pad(g, ty.s0) || (ty.f != 0.f && row_pad(g, ty.s1)) || col_pad(g, tx.s0) ||
           (tx.f != 0.f && col_pad(g, tx.s1));
}

// One output pixel (idx = dy * out_sz + dx) of entry p with geometry g.
MMT_DEV void train_pixel(const mmt_train_crop_params& p, const Geo& g, int idx) {
    const int os = p.out_sz;
    const int dy = idx / os, dx = idx - dy * os;
    if (idx == 0 && p.crop) {
        p.crop[0] = g.x1;
        p.crop[1] = g.y1;
        p.crop[2] = g.crop;
        p.crop[3] = (double)os / g.crop;  // resize_factor = output_sz / crop_sz
    }
    int v[3];
    resize_pixel([&](int r, int c) { return src_px(p, g, r, c); }, g.crop, os, dy, dx, v);
    const int64_t o = (int64_t)dy * os + (p.out_flip ? os - 1 - dx : dx);
    if (p.patch) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) p.patch[o * 3 + ch] = (uint8_t)v[ch];
    }
    if (p.att) p.att[o] = (uint8_t)att_pixel(g, os, dy, dx);
    if (!p.out) return;
    float x[3];
    if (p.lut) {
        // (crop * tf).clip(0.0, 255.0).astype(np.uint8): a float64 product, truncated; then the JET map
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[ch] = (int)fmin((double)v[ch] * p.gain, 255.0);
        colour_map(p.lut, v);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) x[ch] = (float)v[ch] / 255.0f;
    } else {
        const float gf = (float)p.gain;  // the Python scalar bf / 255.0 enters torch's float32 kernel rounded
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) x[ch] = (float)v[ch] * gf;
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float c01 = fminf(fmaxf(x[ch], 0.0f), 1.0f);
        p.out[(int64_t)ch * os * os + o] = (c01 - p.mean[ch]) / p.std[ch];
    }
}

// mmt_sample_target_table's structure: block b works on entry b / tiles, pixels [(b % tiles) * 256, +256);
// the entry and its fp64 geometry are read / computed by one thread and shared through LDS; everything
// the host cannot check in a device-resident entry makes the block return before any store.
__global__ __launch_bounds__(256) void train_crops_table_kernel(const mmt_train_crop_params* __restrict__ table,
                                                                const uint8_t* __restrict__ enable, int tiles,
                                                                int out_sz) {
    __shared__ mmt_train_crop_params sp;
    __shared__ Geo sg;
    __shared__ int live;
    const int e = blockIdx.x / tiles, tile = blockIdx.x - e * tiles;
    if (threadIdx.x == 0) {
        sp = table[e];
        const int on = enable ? enable[e] : 1;
        const int ok = on && sp.image && sp.box && (sp.out || sp.att || sp.patch) && sp.H > 0 && sp.W > 0 &&
                       sp.out_sz == out_sz && sp.factor > 0.0 && sp.gain >= 0.0 && sp.gain <= 1.7976931348623157e308;
        if (ok) sg = crop_geometry(sp.box, sp.factor, sp.H, sp.W);
        live = ok;
    }
    __syncthreads();
    if (!live) return;
    const int idx = tile * 256 + threadIdx.x;
    if (idx >= out_sz * out_sz) return;
    train_pixel(sp, sg, idx);
}

}  // namespace

extern "C" int mmt_train_crops_table(const mmt_train_crop_params* table_dev, const uint8_t* enable_dev, int n,
                                     int out_sz, void* stream) {
    if (!table_dev || n <= 0 || out_sz <= 0 || out_sz > 16384) return MMT_EBADARG;
    if (((uintptr_t)table_dev) & 7) return MMT_EBADARG;
    const int64_t tiles = ((int64_t)out_sz * out_sz + 255) / 256;
    if (tiles * n > 0x7fffffff) return MMT_EBADARG;  // one block per (entry, 256 pixels): the grid's x limit
    hipLaunchKernelGGL(train_crops_table_kernel, dim3((unsigned)(tiles * n)), dim3(256), 0, (hipStream_t)stream,
                       table_dev, enable_dev, (int)tiles, out_sz);
    return launch_status();
}
