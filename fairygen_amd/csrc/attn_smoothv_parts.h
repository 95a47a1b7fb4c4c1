// What the smoothing V producer (attn_pv8.hip, include/fairygen_hip_smoothv.h) and the producers of a token shard in the smoothing form
// (attn_shard8s.hip, include/fairygen_hip_shard8s.h) share, so that both write the same bytes: the walk over v rows that leaves per
// channel and row stride an fp64 sum, a minimum and a maximum (one text for both), and the expressions of mu and sv from a channel's total.
#pragma once
#include "common.h"
#include "attn_qk8_quant.h"

#include <math.h>

namespace {

// The records of a launch: rsum [parts][C] fp64, rlo and rhi [parts][C] fp32 each.  Workgroup (x, y) of 4 waves as attn_v_stats_body
// (attn_pv8_parts.h): wave w adds its rows 4 x + w + 4 gridDim.x i in that order in fp64, and the record of the stride is
// (wave 0 + wave 1) + (wave 2 + wave 3); minimum and maximum do not depend on an order.
__device__ __forceinline__ void attn_v_stats_smooth_body(const bf16* __restrict__ v, int64_t ldv, double* __restrict__ rsum,
                                                         float* __restrict__ rlo, float* __restrict__ rhi, int64_t N, int C) {
    __shared__ double sum_s[3][8][64];
    __shared__ float lo_s[3][8][64];
    __shared__ float hi_s[3][8][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunk = blockIdx.y * 64 + lane;
    const bool live = chunk * 8 < C;
    double sum[8];
    float lo[8], hi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        sum[j] = 0.0;
        lo[j] = INFINITY;
        hi[j] = -INFINITY;
    }
    if (live) {
        for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < N; row += (int64_t)gridDim.x * 4) {
            const bf16x8 x = *reinterpret_cast<const bf16x8*>(v + row * ldv + (int64_t)chunk * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float f = (float)x[j];
                sum[j] += (double)f;
                lo[j] = fminf(lo[j], f);
                hi[j] = fmaxf(hi[j], f);
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            sum_s[wave - 1][j][lane] = sum[j];
            lo_s[wave - 1][j][lane] = lo[j];
            hi_s[wave - 1][j][lane] = hi[j];
        }
    }
    __syncthreads();
    if (wave > 0 || !live) return;
    const int64_t at = (int64_t)blockIdx.x * C + (int64_t)chunk * 8;
    f32x4 l4[2], h4[2];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        rsum[at + j] = (sum[j] + sum_s[0][j][lane]) + (sum_s[1][j][lane] + sum_s[2][j][lane]);
        l4[j >> 2][j & 3] = fminf(fminf(lo[j], lo_s[0][j][lane]), fminf(lo_s[1][j][lane], lo_s[2][j][lane]));
        h4[j >> 2][j & 3] = fmaxf(fmaxf(hi[j], hi_s[0][j][lane]), fmaxf(hi_s[1][j][lane], hi_s[2][j][lane]));
    }
    *reinterpret_cast<f32x4*>(rlo + at) = l4[0];
    *reinterpret_cast<f32x4*>(rlo + at + 4) = l4[1];
    *reinterpret_cast<f32x4*>(rhi + at) = h4[0];
    *reinterpret_cast<f32x4*>(rhi + at + 4) = h4[1];
}

// mu and sv of one channel from the fp64 sum, the minimum and the maximum of its v over all n keys: the largest |fl32(v - mu)| is at
// one of the extremes, fl32(v - mu) being monotone in v.  The expressions of attn_quant_vt_body.inc's smoothing branch, which keeps its
// own copy of these three lines: routing it through this function reorders that kernel's instructions (tools/isa_diff.py).
__device__ __forceinline__ void smoothv_scale(double sum, float lo, float hi, int64_t n, float& mu, float& sv) {
    const float m = (float)(sum / (double)n);
    const float dmax = fmaxf(hi - m, m - lo);
    sv = fmaxf(dmax / kE4M3Max, kScaleFloor);
    mu = m;
}

}  // namespace
