// Internal (non-ABI) entry points shared between the GEMM translation units.
//
// A GEMM call is two steps: gemm_select (host arithmetic on the parameter set alone: no HIP call, no global state,
// pointers read for null-ness and alignment only) names the kernel, and gemm_launch issues it from that answer.
// gemm.hip holds the entry points, the argument checks, the GEMV and register-tile families; gemm_glds.hip the
// LDS-DMA family (its gate, cost model and lean forms, and the only launches of its kernels).
#pragma once
#include "common.hpp"

// The chosen kernel, completely: the exported struct (include/mmt_hip.h documents the fields).
using gemm_choice = mmt_gemm_choice;

constexpr int GEMV_MAXM = 16;  // rows the fp32 GEMV kernel takes

// LDS-DMA large-tile 16-bit GEMM (gemm_glds.hip).  p.impl: -1 never, 0 pick a tile shape, 1..9 force one, 10 as 0
// without the lean frame kernels (include/mmt_hip.h).  false when the shape or layout is not one it takes (the
// caller then falls back to gemm.hip's register tiles); true with c filled in.
bool gemm_glds_select(const mmt_gemm_params& p, gemm_choice& c);

// n (1..4) independent problems of one LDS-DMA configuration in one launch (mmt_gemm_multi); impl 10 as 0 without
// the lean multi kernel.  false when some problem does not qualify (the caller launches them one by one).
bool gemm_glds_select_multi(const mmt_gemm_params* ps, int n, gemm_choice& c);

// Launches what the two functions above chose (c.family == MMT_GEMM_LDS_DMA; c.joint problems), T = bf16_t or f16_t.
template <typename T>
void gemm_glds_launch(const mmt_gemm_params* ps, const gemm_choice& c, hipStream_t st);
