// Tracker-side pre/post-processing on the GPU.
//
//   mmt_sample_target   sample_target (lib/train/data/processing_utils.py:15-77: square crop of
//                       area factor^2 * w*h centred on the box, zero padding, cv2.resize to
//                       output_sz) followed by the tracker's preprocessor
//                       (lib/test/tracker/tracker_utils.py:24-48: optional cv2.applyColorMap for the
//                       TIR crop, HWC uint8 -> CHW fp32, /255, -mean, /std), straight into the
//                       model's fp32 input buffer.  The crop box is computed on the device from the
//                       device-resident tracker state, so a tracking step needs no host round trip.
//   mmt_track_update    the per-frame box post-processing of the trackers
//                       (lib/test/tracker/mixformer_vit_rgbt.py:92-95, :124-131: scale the predicted
//                       cxcywh back to image pixels, map_box_back, lib/utils/box_ops.py:155-164
//                       clip_box with margin 10), updating the device-resident state in place.
//   mmt_sample_target_table / mmt_track_update_slots
//                       the same two for the batched tracker (N sequences per step): the crop
//                       descriptors in a device table of any length, a frame size and an active
//                       flag per slot.  Same device functions, same bits.
//   mmt_sample_target_packed / mmt_track_update_packed
//                       the batched tracker's packed step: a slot list in device memory picks the
//                       table entries (crops go to packed row j) and the slots that prediction
//                       row j updates.  Same device functions, same bits.
//
// cv2 is not part of this image, so the resize arithmetic restates OpenCV's 8-bit INTER_LINEAR
// path (imgproc resize.cpp: float source coordinate (d+0.5)*scale-0.5, 11-bit fixed-point weights
// rounded half-to-even, the horizontal pass in int, the vertical pass as VResizeLinearVec_32s8u
// computes it: ((h0>>4)*b0>>16) + ((h1>>4)*b1>>16), +2, >>2, saturate; rows clamped, columns past
// the edges taken with weight 2048) and its exact-2x INTER_AREA shortcut ((a+b+c+d+2)>>2); the
// colour map is cvtColor(BGR2GRAY) fixed point (1868, 9617, 4899, >>14) then a 256x3 LUT passed in.
// The oracle (oracle/preprocess.py) restates the same arithmetic; both are bit-exact to each other.
#include "crop_common.hpp"  // the crop geometry, the resize and the colour map, shared with train_input.hip

// Parity is bit-exact against separately rounded torch / numpy / Python ops: no FMA contraction.
#pragma clang fp contract(off)

namespace {

struct CropBatch {
    mmt_crop_params c[MMT_MAX_CROPS];
};

MMT_DEV Geo crop_geometry(const mmt_crop_params& p) { return ::crop_geometry(p.box, p.factor, p.H, p.W); }

// padded crop pixel (row r, col c), three channels: image pixel or the constant border 0
MMT_DEV Px3 src_px(const mmt_crop_params& p, const Geo& g, int r, int c) {
    const int iy = g.y1 + r, ix = g.x1 + c;
    if (iy < 0 || ix < 0 || iy >= g.ylim || ix >= g.xlim) return Px3{{0, 0, 0}};
    const uint8_t* q = p.image + ((int64_t)iy * p.W + ix) * 3;
    return Px3{{q[0], q[1], q[2]}};
}

// One output pixel (idx = dy * out_sz + dx) of crop p with geometry g: resize, optional colour map,
// normalise.  Shared by the by-value launch (sample_target_kernel) and the device-table launch
// (sample_target_table_kernel), so both compute the same bits.
MMT_DEV void sample_pixel(const mmt_crop_params& p, const Geo& g, int idx) {
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
    const int64_t o = (int64_t)dy * os + dx;
    if (p.patch) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) p.patch[o * 3 + ch] = (uint8_t)v[ch];
    }
    if (p.lut) colour_map(p.lut, v);
    if (p.out) {
        const float inv255 = 1.0f / 255.0f;  // torch: tensor / python scalar = tensor * (1 / scalar)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) p.out[(int64_t)ch * os * os + o] = ((float)v[ch] * inv255 - p.mean[ch]) / p.std[ch];
    }
}

__global__ __launch_bounds__(256) void sample_target_kernel(const CropBatch cb) {
    const mmt_crop_params& p = cb.c[blockIdx.y];
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.out_sz * p.out_sz) return;
    sample_pixel(p, crop_geometry(p), idx);
}

// The descriptors live in device memory (the captured tracking step holds only the table pointer,
// so the host re-points an entry at another frame with a small copy).  Block b works on entry
// b / tiles, pixels [(b % tiles) * 256, +256).  Nothing in a device-resident entry can be checked
// by the host, so every condition mmt_sample_target rejects on the host makes the block return
// here, before any store.  The entry and its fp64 geometry are read / computed by one thread and
// shared through LDS: same device function, same operands, same results as the per-pixel call.
__global__ __launch_bounds__(256) void sample_target_table_kernel(const mmt_crop_params* __restrict__ table,
                                                                  const uint8_t* __restrict__ enable, int tiles,
                                                                  int out_sz) {
    __shared__ mmt_crop_params sp;
    __shared__ Geo sg;
    __shared__ int live;
    const int e = blockIdx.x / tiles, tile = blockIdx.x - e * tiles;
    if (threadIdx.x == 0) {
        // the entry is read whether enabled or not (it is in bounds): its load and the enable byte's are
        // in flight together, one step less in the chain enable -> entry -> box -> geometry
        sp = table[e];
        const int on = enable ? enable[e] : 1;
        const int ok = on && sp.image && sp.box && (sp.out || sp.patch) && sp.H > 0 && sp.W > 0 && sp.out_sz == out_sz &&
                       sp.factor > 0.0;
        if (ok) sg = crop_geometry(sp);
        live = ok;
    }
    __syncthreads();
    if (!live) return;
    const int idx = tile * 256 + threadIdx.x;
    if (idx >= out_sz * out_sz) return;
    sample_pixel(sp, sg, idx);
}

// The packed form: block b works on list position j = b / (per_slot * tiles), modality m and one
// 256-pixel tile; its entry is slot_list[j] * per_slot + m.  The list is read here only, so the grid
// depends on n and never on the list; a position whose index is not in [0, slots) returns before the
// entry is read.  The entry's own `out` is replaced by packed row j of the caller's buffer; crop and
// patch stay the entry's, so the crop geometry stays slot-indexed.
__global__ __launch_bounds__(256) void sample_target_packed_kernel(const mmt_crop_params* __restrict__ table,
                                                                   const uint8_t* __restrict__ enable,
                                                                   const int32_t* __restrict__ slot_list, int slots,
                                                                   int per_slot, int tiles, int out_sz,
                                                                   float* __restrict__ out, int64_t mod_stride,
                                                                   int64_t row_stride) {
    __shared__ mmt_crop_params sp;
    __shared__ Geo sg;
    __shared__ int live;
    const int pos = blockIdx.x / tiles, tile = blockIdx.x - pos * tiles;
    const int j = pos / per_slot, m = pos - j * per_slot;
    if (threadIdx.x == 0) {
        const int s = slot_list[j];
        int ok = s >= 0 && s < slots;
        if (ok) {
            const int64_t e = (int64_t)s * per_slot + m;
            sp = table[e];
            const int on = enable ? enable[e] : 1;
            ok = on && sp.image && sp.box && (sp.out || sp.patch) && sp.H > 0 && sp.W > 0 && sp.out_sz == out_sz &&
                 sp.factor > 0.0;
            if (ok) {
                sp.out = out + m * mod_stride + j * row_stride;
                sg = crop_geometry(sp);
            }
        }
        live = ok;
    }
    __syncthreads();
    if (!live) return;
    const int idx = tile * 256 + threadIdx.x;
    if (idx >= out_sz * out_sz) return;
    sample_pixel(sp, sg, idx);
}

// map_box_back + clip_box of one tracker: pred (cx, cy, w, h) normalised to the search crop, rf the
// crop's resize factor, s the state (x, y, w, h) updated in place.
MMT_DEV void track_update_one(const float* __restrict__ pred, double rf, double* __restrict__ s, int H, int W,
                              int search_size, double margin) {
    const float inv = 1.0f / (float)rf;  // torch: fp32 tensor / python float = tensor * (1 / (float)scalar)
    double b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = (double)((pred[j] * (float)search_size) * inv);
    const double cx_prev = s[0] + 0.5 * s[2], cy_prev = s[1] + 0.5 * s[3];
    const double half = 0.5 * search_size / rf;
    const double cx = b[0] + (cx_prev - half), cy = b[1] + (cy_prev - half);
    double x1 = cx - 0.5 * b[2], y1 = cy - 0.5 * b[3];
    double x2 = x1 + b[2], y2 = y1 + b[3];
    x1 = fmin(fmax(0.0, x1), W - margin);
    x2 = fmin(fmax(margin, x2), (double)W);
    y1 = fmin(fmax(0.0, y1), H - margin);
    y2 = fmin(fmax(margin, y2), (double)H);
    s[0] = x1;
    s[1] = y1;
    s[2] = fmax(margin, x2 - x1);
    s[3] = fmax(margin, y2 - y1);
}

__global__ void track_update_kernel(const float* __restrict__ pred, const double* __restrict__ crop,
                                    double* __restrict__ state, int n, int H, int W, int search_size, double margin) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    track_update_one(pred + i * 4, crop[i * 4 + 3], state + i * 4, H, W, search_size, margin);
}

// Per-slot frame size, a stride between the crop records, and a mask: an inactive slot (or one whose
// frame size is not set) keeps its state untouched.
__global__ void track_update_slots_kernel(const float* __restrict__ pred, const double* __restrict__ crop,
                                          int crop_stride, double* __restrict__ state, const int32_t* __restrict__ hw,
                                          const uint8_t* __restrict__ active, int n, int search_size, double margin) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (active && !active[i]) return;
    const int H = hw[i * 2], W = hw[i * 2 + 1];
    if (H <= 0 || W <= 0) return;
    track_update_one(pred + i * 4, crop[(int64_t)i * crop_stride + 3], state + i * 4, H, W, search_size, margin);
}

// Prediction row j updates slot slot_list[j]: state, hw, the crop record and the active byte are the
// slot's.  A position outside [0, slots), an inactive slot or one without a frame size writes nothing.
__global__ void track_update_packed_kernel(const float* __restrict__ pred, const double* __restrict__ crop,
                                           int crop_stride, double* __restrict__ state, const int32_t* __restrict__ hw,
                                           const uint8_t* __restrict__ active, const int32_t* __restrict__ slot_list,
                                           int n, int slots, int search_size, double margin) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int s = slot_list[j];
    if (s < 0 || s >= slots) return;
    if (active && !active[s]) return;
    const int H = hw[(int64_t)s * 2], W = hw[(int64_t)s * 2 + 1];
    if (H <= 0 || W <= 0) return;
    track_update_one(pred + (int64_t)j * 4, crop[(int64_t)s * crop_stride + 3], state + (int64_t)s * 4, H, W, search_size,
                     margin);
}

}  // namespace

extern "C" int mmt_sample_target(const mmt_crop_params* p, int n, void* stream) {
    if (!p || n <= 0 || n > MMT_MAX_CROPS) return MMT_EBADARG;
    CropBatch cb;
    int os = 0;
    for (int i = 0; i < n; ++i) {
        const mmt_crop_params& c = p[i];
        if (!c.image || !c.box || c.H <= 0 || c.W <= 0 || c.out_sz <= 0 || !(c.factor > 0.0)) return MMT_EBADARG;
        if (!c.out && !c.patch) return MMT_EBADARG;
        if (i > 0 && c.out_sz != os) return MMT_EBADARG;  // one grid per launch
        os = c.out_sz;
        cb.c[i] = c;
    }
    dim3 grid((os * os + 255) / 256, n);
    hipLaunchKernelGGL(sample_target_kernel, grid, dim3(256), 0, (hipStream_t)stream, cb);
    return launch_status();
}

extern "C" int mmt_track_update(const float* pred_cxcywh, const double* crop, double* state, int n, int H, int W,
                                int search_size, double margin, void* stream) {
    if (!pred_cxcywh || !crop || !state || n <= 0 || H <= 0 || W <= 0 || search_size <= 0) return MMT_EBADARG;
    hipLaunchKernelGGL(track_update_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, pred_cxcywh, crop,
                       state, n, H, W, search_size, margin);
    return launch_status();
}

extern "C" int mmt_sample_target_table(const mmt_crop_params* table_dev, const uint8_t* enable_dev, int n, int out_sz,
                                       void* stream) {
    if (!table_dev || n <= 0 || out_sz <= 0 || out_sz > 16384) return MMT_EBADARG;
    const int64_t tiles = ((int64_t)out_sz * out_sz + 255) / 256;
    if (tiles * n > 0x7fffffff) return MMT_EBADARG;  // one block per (entry, 256 pixels): the grid's x limit
    hipLaunchKernelGGL(sample_target_table_kernel, dim3((unsigned)(tiles * n)), dim3(256), 0, (hipStream_t)stream,
                       table_dev, enable_dev, (int)tiles, out_sz);
    return launch_status();
}

extern "C" int mmt_track_update_slots(const float* pred_cxcywh, const double* crop, int crop_stride, double* state,
                                      const int32_t* hw, const uint8_t* active, int n, int search_size, double margin,
                                      void* stream) {
    if (!pred_cxcywh || !crop || !state || !hw || n <= 0 || search_size <= 0 || crop_stride < 4) return MMT_EBADARG;
    hipLaunchKernelGGL(track_update_slots_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, pred_cxcywh,
                       crop, crop_stride, state, hw, active, n, search_size, margin);
    return launch_status();
}

extern "C" int mmt_sample_target_packed(const mmt_crop_params* table_dev, const uint8_t* enable_dev,
                                        const int32_t* slot_list_dev, int n, int slots, int per_slot, int out_sz,
                                        float* out, int64_t mod_stride, int64_t row_stride, void* stream) {
    if (!table_dev || !slot_list_dev || !out || n <= 0 || slots <= 0 || per_slot < 1 || per_slot > MMT_MAX_CROPS ||
        out_sz <= 0 || out_sz > 16384)
        return MMT_EBADARG;
    if (mod_stride < 0 || row_stride < 0) return MMT_EBADARG;
    const int64_t tiles = ((int64_t)out_sz * out_sz + 255) / 256;
    if (tiles * n * per_slot > 0x7fffffff) return MMT_EBADARG;  // one block per (position, modality, 256 pixels)
    hipLaunchKernelGGL(sample_target_packed_kernel, dim3((unsigned)(tiles * n * per_slot)), dim3(256), 0,
                       (hipStream_t)stream, table_dev, enable_dev, slot_list_dev, slots, per_slot, (int)tiles, out_sz, out,
                       mod_stride, row_stride);
    return launch_status();
}

extern "C" int mmt_track_update_packed(const float* pred_cxcywh, const double* crop, int crop_stride, double* state,
                                       const int32_t* hw, const uint8_t* active, const int32_t* slot_list_dev, int n,
                                       int slots, int search_size, double margin, void* stream) {
    if (!pred_cxcywh || !crop || !state || !hw || !slot_list_dev || n <= 0 || slots <= 0 || search_size <= 0 ||
        crop_stride < 4)
        return MMT_EBADARG;
    hipLaunchKernelGGL(track_update_packed_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, pred_cxcywh,
                       crop, crop_stride, state, hw, active, slot_list_dev, n, slots, search_size, margin);
    return launch_status();
}
