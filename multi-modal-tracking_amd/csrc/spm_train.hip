// Score-head training (TRAIN.TRAIN_SCORE, train_script_mixformer.py:138-140, actors/mixformer_rgbt.py:150-152):
// the ScoreDecoder's single-query attention (score_decoder.py:32-66) with the softmax rows kept for its
// backward, that backward, and the BCE-with-logits loss both ways.
//
//   mmt_spm_attention_train_fwd  mmt_spm_attention (head.hip) that also stores prob [B][H][Lk]; same arithmetic in
//                                the same order, so `out` has the inference kernel's bits
//   mmt_spm_attention_bwd        dp_j = dout_h . v_j, ds_j = prob_j (dp_j - sum_i prob_i dp_i);
//                                dv_j = prob_j dout_h, dk_j = scale ds_j q_h, dq_h = scale sum_j ds_j k_j
//   mmt_spm_dq_sum              the shared query's gradient: the B rows of dq summed in row order
//   mmt_bce_logits / _bwd        weight * mean_i BCEWithLogits(x_i, y_i) and its gradient
//
// fp32 throughout.  One 256-thread workgroup per (head, batch row) as in the forward; every output element has
// one writer (no atomics, no pre-zeroing) and every sum runs in a fixed order: two launches give the same bits.
#include "common.hpp"

namespace {

constexpr int SPM_MAXK = 2048;  // keys: head.hip's SPM_MAXK (the LDS score row of the forward)

// spm_attention_kernel of head.hip statement for statement, plus the store of the normalised rows.
__global__ __launch_bounds__(256) void spm_attention_train_kernel(const float* __restrict__ q, int64_t q_stride,
                                                                  const float* __restrict__ kv, float* __restrict__ out,
                                                                  float* __restrict__ prob, int Lk, int C, float scale) {
    __shared__ float sc[SPM_MAXK];  // Lk scores
    __shared__ __attribute__((aligned(16))) float qs[64];
    __shared__ float red[4];
    __shared__ float part[4][64];
    const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid < 64) qs[tid] = q[b * q_stride + h * 64 + tid];
    __syncthreads();
    const float* kb = kv + (int64_t)b * Lk * 2 * C + h * 64;
    float mx = -INFINITY;
    for (int t = tid; t < Lk; t += 256) {
        const float* kr = kb + (int64_t)t * 2 * C;
        float acc = 0.f;
#pragma unroll
        for (int d = 0; d < 64; d += 4) {
            const float4 kv4 = *(const float4*)(kr + d);
            const float4 q4 = *(const float4*)(qs + d);
            acc = fmaf(q4.x, kv4.x, fmaf(q4.y, kv4.y, fmaf(q4.z, kv4.z, fmaf(q4.w, kv4.w, acc))));
        }
        acc *= scale;
        sc[t] = acc;
        mx = fmaxf(mx, acc);
    }
    mx = wave_max(mx);
    if (lane == 0) red[w] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float se = 0.f;
    for (int t = tid; t < Lk; t += 256) {
        const float e = expf(sc[t] - mx);
        sc[t] = e;
        se += e;
    }
    se = wave_sum(se);
    if (lane == 0) red[w] = se;
    __syncthreads();
    const float inv = 1.f / (red[0] + red[1] + red[2] + red[3]);
    float* pr = prob + ((int64_t)b * gridDim.x + h) * Lk;
    for (int t = tid; t < Lk; t += 256) pr[t] = sc[t] * inv;
    float acc = 0.f;
    for (int t = w; t < Lk; t += 4) acc = fmaf(sc[t], kb[(int64_t)t * 2 * C + C + lane], acc);
    part[w][lane] = acc;
    __syncthreads();
    if (w == 0) out[(int64_t)b * C + h * 64 + lane] = (part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane]) * inv;
}

// Backward.  Pass 1, a thread per key (t, t + 256, ..): dp_t = dout_h . v_t by 16-B loads against dout_h in LDS,
// and the row's sum_t prob_t dp_t (wave reduction, then the four waves' sums in order).  Pass 2, a wave per key
// row (t = w, w + 4, ..), lane = channel: the coalesced 256-B stores of dk_t and dv_t, and dq's per-wave partial
// sums, combined in order as the forward combines part[4][64].
__global__ __launch_bounds__(256) void spm_attention_bwd_kernel(const float* __restrict__ q, int64_t q_stride,
                                                                const float* __restrict__ kv,
                                                                const float* __restrict__ prob,
                                                                const float* __restrict__ dout, float* __restrict__ dq,
                                                                float* __restrict__ dkv, int Lk, int C, float scale) {
    __shared__ float ps[SPM_MAXK];   // prob_t
    __shared__ float dsb[SPM_MAXK];  // dp_t, then ds_t
    __shared__ __attribute__((aligned(16))) float dos[64];
    __shared__ float red[4];
    __shared__ float part[4][64];
    const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid < 64) dos[tid] = dout[(int64_t)b * C + h * 64 + tid];
    __syncthreads();
    const float* kb = kv + (int64_t)b * Lk * 2 * C + h * 64;
    const float* pr = prob + ((int64_t)b * gridDim.x + h) * Lk;
    float s = 0.f;
    for (int t = tid; t < Lk; t += 256) {
        const float* vr = kb + (int64_t)t * 2 * C + C;
        float acc = 0.f;
#pragma unroll
        for (int d = 0; d < 64; d += 4) {
            const float4 v4 = *(const float4*)(vr + d);
            const float4 g4 = *(const float4*)(dos + d);
            acc = fmaf(g4.x, v4.x, fmaf(g4.y, v4.y, fmaf(g4.z, v4.z, fmaf(g4.w, v4.w, acc))));
        }
        const float p = pr[t];
        ps[t] = p;
        dsb[t] = acc;
        s = fmaf(p, acc, s);
    }
    s = wave_sum(s);
    if (lane == 0) red[w] = s;
    __syncthreads();
    s = (red[0] + red[1]) + (red[2] + red[3]);
    for (int t = tid; t < Lk; t += 256) dsb[t] = ps[t] * (dsb[t] - s);  // each thread its own keys again
    __syncthreads();
    const float qc = q[b * q_stride + h * 64 + lane], gc = dos[lane];
    float* db = dkv + (int64_t)b * Lk * 2 * C + h * 64;
    float acc = 0.f;
    for (int t = w; t < Lk; t += 4) {
        const float ds = dsb[t];
        const int64_t row = (int64_t)t * 2 * C;
        acc = fmaf(ds, kb[row + lane], acc);
        db[row + lane] = (scale * ds) * qc;
        db[row + C + lane] = ps[t] * gc;
    }
    part[w][lane] = acc;
    __syncthreads();
    if (w == 0) dq[(int64_t)b * C + h * 64 + lane] = (part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane]) * scale;
}

// The shared query of decoder layer 0 is one learnable row: its gradient is the sum of the backward's B rows
// of dq, added in row order.
__global__ __launch_bounds__(256) void spm_dq_sum_kernel(const float* __restrict__ dq, float* __restrict__ out, int B,
                                                         int C) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += dq[(int64_t)b * C + c];
    out[c] = s;
}

constexpr int BCE_MAXB = 65536;

// log(1 + exp(-|x|)) + max(-x, 0) = -log_sigmoid(x): the overflow-free form of
// max(-x, 0) + log(exp(-m) + exp(-x - m)), m = max(-x, 0)
MMT_DEV float bce_elem(float x, float y) { return (1.f - y) * x + (fmaxf(-x, 0.f) + log1pf(expf(-fabsf(x)))); }

__global__ __launch_bounds__(256) void bce_logits_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                         float weight, float* __restrict__ loss, int B) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < B; i += 256) s += bce_elem(x[i], y[i]);
    s = block_sum<256>(s, red);
    if (threadIdx.x == 0) loss[0] = weight * (s / (float)B);
}

__global__ __launch_bounds__(256) void bce_logits_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                             const float* __restrict__ dloss, float weight,
                                                             float* __restrict__ dx, int B) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    const float g = dloss[0] * weight;
    dx[i] = g * (1.f / (1.f + expf(-x[i])) - y[i]) / (float)B;
}

bool spm_args_ok(const void* q, const void* kv, int B, int Lk, int C, int H) {
    if (!q || !kv || B <= 0 || H <= 0 || Lk <= 0 || Lk > SPM_MAXK || C != H * 64) return false;
    return !(((uintptr_t)kv & 15) || ((uintptr_t)q & 3));
}

}  // namespace

extern "C" int mmt_spm_attention_train_fwd(const float* q, int64_t q_stride, const float* kv, float* out, float* prob,
                                           int B, int Lk, int C, int H, float scale, void* stream) {
    if (!out || !prob || !spm_args_ok(q, kv, B, Lk, C, H) || (q_stride != 0 && q_stride != C)) return MMT_EBADARG;
    hipLaunchKernelGGL(spm_attention_train_kernel, dim3(H, B), dim3(256), 0, (hipStream_t)stream, q, q_stride, kv, out,
                       prob, Lk, C, scale);
    return launch_status();
}

extern "C" int mmt_spm_attention_bwd(const float* q, int64_t q_stride, const float* kv, const float* prob,
                                     const float* dout, float* dq, float* dkv, int B, int Lk, int C, int H, float scale,
                                     void* stream) {
    if (!prob || !dout || !dq || !dkv || !spm_args_ok(q, kv, B, Lk, C, H) || (q_stride != 0 && q_stride != C))
        return MMT_EBADARG;
    if ((uintptr_t)dout & 3) return MMT_EBADARG;
    hipLaunchKernelGGL(spm_attention_bwd_kernel, dim3(H, B), dim3(256), 0, (hipStream_t)stream, q, q_stride, kv, prob,
                       dout, dq, dkv, Lk, C, scale);
    return launch_status();
}

extern "C" int mmt_spm_dq_sum(const float* dq, float* out, int B, int C, void* stream) {
    if (!dq || !out || B <= 0 || C <= 0) return MMT_EBADARG;
    hipLaunchKernelGGL(spm_dq_sum_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, dq, out, B, C);
    return launch_status();
}

extern "C" int mmt_bce_logits(const float* logits, const float* labels, float weight, float* loss, int B, void* stream) {
    if (!logits || !labels || !loss || B <= 0 || B > BCE_MAXB) return MMT_EBADARG;
    hipLaunchKernelGGL(bce_logits_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, labels, weight, loss, B);
    return launch_status();
}

extern "C" int mmt_bce_logits_bwd(const float* logits, const float* labels, const float* dloss, float weight,
                                  float* dlogits, int B, void* stream) {
    if (!logits || !labels || !dloss || !dlogits || B <= 0 || B > BCE_MAXB) return MMT_EBADARG;
    hipLaunchKernelGGL(bce_logits_bwd_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, logits, labels,
                       dloss, weight, dlogits, B);
    return launch_status();
}
