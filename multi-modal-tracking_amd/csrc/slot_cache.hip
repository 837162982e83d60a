// Slot-indexed row copy for the batched tracker's per-slot template K/V cache (mmt_slot_copy).
//
// The template pass of the slots whose templates changed runs on a compact D-slot staging layout; this
// kernel moves the listed slots' rows between that layout and the N-slot one: template crops in (gather),
// the per-layer K / V columns and the score head's KV1 rows out (scatter).  Segments and slot lists live in
// device memory, so one captured graph serves every slot list.  Pure bandwidth: 16 B per lane per access,
// each lane keeps 4 loads in flight before its 4 stores; no LDS.
//
// grid = (ceil(max chunks of a segment / 1024), nseg, n): block (x, s, j) copies 16-B chunks x * 256 + tid,
// + gridDim.x * 256, ... of segment s for list entry j.  The loop is grid-stride over the segment's own
// chunk count, so a segment smaller than the largest one idles some blocks and nothing else.
#include "common.hpp"

namespace {

constexpr int SC_THREADS = 256, SC_UNROLL = 4;

__global__ __launch_bounds__(SC_THREADS) void slot_copy_kernel(const mmt_slot_copy_seg* __restrict__ segs,
                                                               const int32_t* __restrict__ src_slot, int src_slots,
                                                               const int32_t* __restrict__ dst_slot, int dst_slots) {
    const int j = blockIdx.z;
    const int ss = src_slot ? src_slot[j] : j, ds = dst_slot ? dst_slot[j] : j;
    if (ss < 0 || ss >= src_slots || ds < 0 || ds >= dst_slots) return;  // skipped entry: no read, no write
    const mmt_slot_copy_seg sg = segs[blockIdx.y];
    if (!sg.src || !sg.dst || sg.rows <= 0 || sg.row_bytes < 16) return;
    const uint32_t cpr = (uint32_t)sg.row_bytes >> 4;  // 16-B chunks per row
    const uint64_t total64 = (uint64_t)sg.rows * cpr;
    if (total64 > 0x7fffffffu) return;  // past the documented segment bound (32 GiB per slot)
    const uint32_t total = (uint32_t)total64;
    const char* src = (const char*)sg.src + (int64_t)ss * sg.src_slot_stride;
    char* dst = (char*)sg.dst + (int64_t)ds * sg.dst_slot_stride;
    // chunk c = (row, col); the grid stride as (rows, cols) too, so the loop needs no division
    const uint32_t stride = gridDim.x * SC_THREADS;
    uint32_t c = blockIdx.x * SC_THREADS + threadIdx.x;
    uint32_t row = c / cpr, col = c - row * cpr;
    const uint32_t srow = stride / cpr, scol = stride - srow * cpr;
    while (c < total) {
        u32x4 v[SC_UNROLL];
        int64_t doff[SC_UNROLL];
        bool ok[SC_UNROLL];
#pragma unroll
        for (int k = 0; k < SC_UNROLL; ++k) {
            ok[k] = c < total;
            doff[k] = (int64_t)row * sg.dst_row_pitch + (int64_t)col * 16;
            if (ok[k]) v[k] = *(const u32x4*)(src + (int64_t)row * sg.src_row_pitch + (int64_t)col * 16);
            c += stride;
            row += srow;
            col += scol;
            if (col >= cpr) col -= cpr, ++row;
        }
#pragma unroll
        for (int k = 0; k < SC_UNROLL; ++k)
            if (ok[k]) *(u32x4*)(dst + doff[k]) = v[k];
    }
}

}  // namespace

extern "C" int mmt_slot_copy(const mmt_slot_copy_seg* segs_dev, int nseg, const int32_t* src_slot_dev, int src_slots,
                             const int32_t* dst_slot_dev, int dst_slots, int n, int64_t max_seg_bytes, void* stream) {
    if (!segs_dev || nseg <= 0 || n <= 0 || src_slots <= 0 || dst_slots <= 0) return MMT_EBADARG;
    if (!src_slot_dev && !dst_slot_dev && src_slots != dst_slots) return MMT_EBADARG;
    if (nseg > 65535 || n > 65535) return MMT_EBADARG;  // grid y / z limits
    if (max_seg_bytes < 16 || (max_seg_bytes & 15) || (max_seg_bytes >> 4) > INT32_MAX) return MMT_EBADARG;
    if (((uintptr_t)segs_dev & 7) || ((uintptr_t)src_slot_dev & 3) || ((uintptr_t)dst_slot_dev & 3)) return MMT_EBADARG;
    const int64_t per_block = (int64_t)SC_THREADS * SC_UNROLL;
    int64_t bx = ((max_seg_bytes >> 4) + per_block - 1) / per_block;
    if (bx > 65535) bx = 65535;  // the kernel's loop is grid-stride
    hipLaunchKernelGGL(slot_copy_kernel, dim3((unsigned)bx, (unsigned)nseg, (unsigned)n), dim3(SC_THREADS), 0,
                       (hipStream_t)stream, segs_dev, src_slot_dev, src_slots, dst_slot_dev, dst_slots);
    return launch_status();
}
