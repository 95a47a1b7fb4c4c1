// e4m3 operands of the opt-in 8-bit Q K^T self-attention (fg_attn_fwd_qk8_bf16), for gfx950.
//
// The reference's flash_attention calls sageattn(q, k, v) when that package is present (models/wan_video_dit.py:48-52): 8-bit Q K^T with K
// mean-smoothing, P V in 16 bits.  The recipe here, per head, q and k (N, 128) bf16 after RMSNorm and RoPE:
//   kbar = mean over the N keys of k (per channel; the fp64 sum rounded once to fp32),  k' = k - kbar  (q . kbar is constant along a
//          softmax row, so the softmax is unchanged),
//   sk   = max(max|k'| / 448, 2^-20)  one scale per head,          k8 = e4m3(k' / sk)   round-to-nearest-even, saturating,
//   sq[r] = max(max|q[r]| / 448, 2^-20)  one per row and head,     q8 = e4m3(q / sq[r]).
// Two stream-ordered launches: the column mean and |k'| maximum of every head (one workgroup per head: the maximum needs the finished
// mean), then the quantise pass over 16 rows x 1 head per workgroup.  HBM-bound: q and k are read once by the second pass and k twice
// more by the first, 1.5 bytes written per 4 read.
#include "common.h"
#include "../../include/fairygen_hip_batch8.h"
#include "attn_qk8_quant.h"

namespace {

// One workgroup of 1024 per head.  Thread t: 16-byte chunk t & 15 of the rows (t >> 4) + 64 i.
__global__ __launch_bounds__(1024) void attn_k_stats_kernel(const bf16* __restrict__ k, int64_t ldk, float* __restrict__ kbar,
                                                            float* __restrict__ sk, int64_t N) {
#include "attn_k_stats_body.inc"
}

// 16 rows of one head per workgroup of 256: 16 lanes x 8 channels cover a row.
__device__ __forceinline__ void attn_quant_qk_body(const bf16* __restrict__ q, int64_t ldq, const bf16* __restrict__ k, int64_t ldk,
                                                   const float* __restrict__ kbar, const float* __restrict__ sk, uint8_t* __restrict__ q8,
                                                   uint8_t* __restrict__ k8, float* __restrict__ sq, int64_t N, int H) {
    const int h = blockIdx.y, tid = threadIdx.x, c = tid & 15;
    const int64_t row = (int64_t)blockIdx.x * 16 + (tid >> 4);
    const bool valid = row < N;
    const int64_t rr = valid ? row : N - 1;
    const bf16x8 qv = *reinterpret_cast<const bf16x8*>(q + rr * ldq + (int64_t)h * kD + c * 8);
    const bf16x8 kv = *reinterpret_cast<const bf16x8*>(k + rr * ldk + (int64_t)h * kD + c * 8);
    const f32x4 m0 = *reinterpret_cast<const f32x4*>(kbar + h * kD + c * 8), m1 = *reinterpret_cast<const f32x4*>(kbar + h * kD + c * 8 + 4);
    const float s_k = sk[h];
    float qf[8], kf[8], amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        qf[j] = (float)qv[j];
        kf[j] = (float)kv[j] - (j < 4 ? m0[j & 3] : m1[j & 3]);
        amax = fmaxf(amax, fabsf(qf[j]));
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    const float s_q = fmaxf(amax / kE4M3Max, kScaleFloor);
    if (!valid) return;
    const u32x2 wq = quant8_e4m3(qf, s_q), wk = quant8_e4m3(kf, s_k);
    const int64_t o = (row * H + h) * kD + c * 8;
    *reinterpret_cast<u32x2*>(q8 + o) = wq;
    *reinterpret_cast<u32x2*>(k8 + o) = wk;
    if (c == 0) sq[row * H + h] = s_q;
}

__global__ __launch_bounds__(256) void attn_quant_qk_kernel(const bf16* __restrict__ q, int64_t ldq, const bf16* __restrict__ k, int64_t ldk,
                                                            const float* __restrict__ kbar, const float* __restrict__ sk,
                                                            uint8_t* __restrict__ q8, uint8_t* __restrict__ k8, float* __restrict__ sq,
                                                            int64_t N, int H) {
    attn_quant_qk_body(q, ldq, k, ldk, kbar, sk, q8, k8, sq, N, H);
}

// The batched forms (include/fairygen_hip_batch8.h): one more grid dimension picks the batch element, whose pointers the strides give;
// the element then runs the body of the single-element kernel.
struct QuantQkStrides {
    int64_t q, k, q8, k8, sq, sk, kbar;
};

__global__ __launch_bounds__(1024) void attn_k_stats_b_kernel(const bf16* __restrict__ k, int64_t ldk, float* __restrict__ kbar,
                                                              float* __restrict__ sk, int64_t N, const QuantQkStrides bs) {
    const int64_t b = blockIdx.y;
    k += b * bs.k; kbar += b * bs.kbar; sk += b * bs.sk;
#include "attn_k_stats_body.inc"
}

__global__ __launch_bounds__(256) void attn_quant_qk_b_kernel(const bf16* __restrict__ q, int64_t ldq, const bf16* __restrict__ k, int64_t ldk,
                                                              const float* __restrict__ kbar, const float* __restrict__ sk,
                                                              uint8_t* __restrict__ q8, uint8_t* __restrict__ k8, float* __restrict__ sq,
                                                              int64_t N, int H, const QuantQkStrides bs) {
    const int64_t b = blockIdx.z;
    attn_quant_qk_body(q + b * bs.q, ldq, k + b * bs.k, ldk, kbar + b * bs.kbar, sk + b * bs.sk, q8 + b * bs.q8, k8 + b * bs.k8,
                       sq + b * bs.sq, N, H);
}

}  // namespace

extern "C" int fg_attn_qk8_version(void) { return 1; }

extern "C" int fg_attn_quant_qk_bf16(const void* q, int64_t ldq, const void* k, int64_t ldk, void* q8, void* k8, float* sq, float* sk,
                                     void* scratch, int64_t scratch_bytes, int64_t N, int H, int D, fg_stream_t stream) {
    FG_CHECK_ARG(q && k && q8 && k8 && sq && sk && scratch, "fg_attn_quant_qk_bf16: null pointer");
    FG_CHECK_ARG(D == kD, "fg_attn_quant_qk_bf16: only head_dim 128 is supported (got %d)", D);
    FG_CHECK_ARG(N > 0 && H > 0 && H <= 65535, "fg_attn_quant_qk_bf16: N must be positive, H in 1..65535");
    const int64_t hd = (int64_t)H * D;
    FG_CHECK_ARG(ldq >= hd && ldk >= hd && ldq % 8 == 0 && ldk % 8 == 0, "fg_attn_quant_qk_bf16: leading dimensions must be >= H*D and multiples of 8");
    FG_CHECK_ARG(FG_ALIGNED16(q) && FG_ALIGNED16(k) && FG_ALIGNED16(scratch) && (((uintptr_t)q8 | (uintptr_t)k8) & 7) == 0 &&
                     (((uintptr_t)sq | (uintptr_t)sk) & 3) == 0,
                 "fg_attn_quant_qk_bf16: q, k, scratch must be 16-byte aligned (q8, k8: 8; sq, sk: 4)");
    FG_CHECK_ARG(scratch_bytes >= hd * 4, "fg_attn_quant_qk_bf16: scratch must hold H*D floats (%lld bytes, got %lld)", (long long)(hd * 4),
                 (long long)scratch_bytes);
    FG_CHECK_ARG((N + 15) / 16 < (1ll << 31), "fg_attn_quant_qk_bf16: grid too large");
    hipLaunchKernelGGL(attn_k_stats_kernel, dim3((unsigned)H), dim3(1024), 0, (hipStream_t)stream, (const bf16*)k, ldk, (float*)scratch, sk, N);
    if (int e = fg_launch_status("fg_attn_quant_qk_bf16 (k statistics)")) return e;
    hipLaunchKernelGGL(attn_quant_qk_kernel, dim3((unsigned)((N + 15) / 16), (unsigned)H), dim3(256), 0, (hipStream_t)stream, (const bf16*)q, ldq,
                       (const bf16*)k, ldk, (const float*)scratch, (const float*)sk, (uint8_t*)q8, (uint8_t*)k8, sq, N, H);
    return fg_launch_status("fg_attn_quant_qk_bf16");
}

extern "C" int fg_attn_batch8_version(void) { return 1; }

extern "C" int fg_attn_quant_qk_bf16_b(const void* q, int64_t ldq, int64_t bs_q, const void* k, int64_t ldk, int64_t bs_k, void* q8,
                                       int64_t bs_q8, void* k8, int64_t bs_k8, float* sq, int64_t bs_sq, float* sk, int64_t bs_sk,
                                       void* scratch, int64_t scratch_bytes, int64_t bs_scratch, int B, int64_t N, int H, int D,
                                       fg_stream_t stream) {
    FG_CHECK_ARG(q && k && q8 && k8 && sq && sk && scratch, "fg_attn_quant_qk_bf16_b: null pointer");
    FG_CHECK_ARG(D == kD, "fg_attn_quant_qk_bf16_b: only head_dim 128 is supported (got %d)", D);
    FG_CHECK_ARG(B >= 1 && B <= 65535, "fg_attn_quant_qk_bf16_b: B must be in 1..65535 (got %d)", B);
    FG_CHECK_ARG(N > 0 && H > 0 && H <= 65535, "fg_attn_quant_qk_bf16_b: N must be positive, H in 1..65535");
    const int64_t hd = (int64_t)H * D;
    FG_CHECK_ARG(ldq >= hd && ldk >= hd && ldq % 8 == 0 && ldk % 8 == 0,
                 "fg_attn_quant_qk_bf16_b: leading dimensions must be >= H*D and multiples of 8");
    FG_CHECK_ARG(FG_ALIGNED16(q) && FG_ALIGNED16(k) && FG_ALIGNED16(scratch) && (((uintptr_t)q8 | (uintptr_t)k8) & 7) == 0 &&
                     (((uintptr_t)sq | (uintptr_t)sk) & 3) == 0,
                 "fg_attn_quant_qk_bf16_b: q, k, scratch must be 16-byte aligned (q8, k8: 8; sq, sk: 4)");
    FG_CHECK_ARG(scratch_bytes >= hd * 4, "fg_attn_quant_qk_bf16_b: scratch must hold H*D floats per element (%lld bytes, got %lld)",
                 (long long)(hd * 4), (long long)scratch_bytes);
    FG_CHECK_ARG(bs_q >= (N - 1) * ldq + hd && bs_k >= (N - 1) * ldk + hd && bs_q8 >= N * hd && bs_k8 >= N * hd && bs_sq >= N * H &&
                     bs_sk >= H && bs_scratch >= hd * 4,
                 "fg_attn_quant_qk_bf16_b: a batch stride is smaller than one element of its operand");
    FG_CHECK_ARG(bs_q % 8 == 0 && bs_k % 8 == 0 && bs_q8 % 8 == 0 && bs_k8 % 8 == 0 && bs_scratch % 16 == 0,
                 "fg_attn_quant_qk_bf16_b: batch strides must keep the alignment (q, k: 8 elements; q8, k8: 8 bytes; scratch: 16 bytes)");
    FG_CHECK_ARG((N + 15) / 16 < (1ll << 31), "fg_attn_quant_qk_bf16_b: grid too large");
    const QuantQkStrides bs{bs_q, bs_k, bs_q8, bs_k8, bs_sq, bs_sk, bs_scratch / 4};
    hipLaunchKernelGGL(attn_k_stats_b_kernel, dim3((unsigned)H, (unsigned)B), dim3(1024), 0, (hipStream_t)stream, (const bf16*)k, ldk,
                       (float*)scratch, sk, N, bs);
    if (int e = fg_launch_status("fg_attn_quant_qk_bf16_b (k statistics)")) return e;
    hipLaunchKernelGGL(attn_quant_qk_b_kernel, dim3((unsigned)((N + 15) / 16), (unsigned)H, (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                       (const bf16*)q, ldq, (const bf16*)k, ldk, (const float*)scratch, (const float*)sk, (uint8_t*)q8, (uint8_t*)k8, sq, N, H,
                       bs);
    return fg_launch_status("fg_attn_quant_qk_bf16_b");
}
