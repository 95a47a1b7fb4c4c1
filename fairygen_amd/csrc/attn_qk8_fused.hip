// The e4m3 operands of fg_attn_fwd_qk8_bf16 written by the RMSNorm+RoPE pass (include/fairygen_hip.h), for gfx950.
//
// rmsnorm_rope_kernel (dit_elementwise.hip) holds every post-RoPE q and k row in registers, one wave per row; with head_dim 128 a head
// is 16 adjacent lanes of one vector slot.  The stand-alone quantise pass (attn_qk8.hip) reads that kernel's bf16 k twice for the key
// statistics and q and k once more to convert them.  Here, with the recipe of attn_qk8.hip unchanged and the same bytes out:
//   q: the row leaves the norm as e4m3 + one scale per head and never exists as bf16;
//   k: the norm writes bf16 k as before and keeps, per channel, the fp64 sum, the minimum and the maximum of the values it wrote —
//      P workgroups walk the rows and leave one partial record each; a small launch reduces the P records to the mean and the head's
//      scale; one pass over k converts it.
// The mean: where the fp64 sum of the bf16 values is exact, its order cannot show, so P partial sums give the one-workgroup kernel's
// mean.  The scale: fl(v - m) is monotone in v, so max over rows of |fl(v - m)| is max(fl(vmax - m), fl(m - vmin)).
// Per q/k element pair 10 bytes of HBM traffic (q 2 in 1 out, k 2 in 2 out, then 2 in 1 out) where the two-step path moves 18.
#include "common.h"
#include "../../include/fairygen_hip_batch8.h"
#include "rmsnorm_rope_row.h"
#include "attn_qk8_quant.h"

#include <math.h>

namespace {

// Workgroups of the key producer = partial records per channel: a function of the row count alone, 16 rows a workgroup until one
// workgroup per CU is reached
constexpr int kMinParts = 8, kMaxParts = 256;
inline int64_t stat_parts(int64_t rows) {
    const int64_t p = (rows + 15) / 16;
    return p < kMinParts ? kMinParts : (p > kMaxParts ? kMaxParts : p);
}
// partials: (P, C) fp64 sums, then (P, C) fp32 minima, then (P, C) fp32 maxima
inline int64_t partials_bytes_for(int64_t rows, int C) { return stat_parts(rows) * C * 16; }

// The norm of rmsnorm_rope_kernel, 4 rows per workgroup, head_dim 128; each head of a row leaves as 128 e4m3 bytes and a scale.
template <bool F32TAB>
__global__ __launch_bounds__(256, 4) void rmsnorm_rope_q8_kernel(const bf16* __restrict__ x, int64_t ldx, const bf16* __restrict__ w,
                                                                 const void* __restrict__ ctv, const void* __restrict__ stv,
                                                                 uint8_t* __restrict__ q8, float* __restrict__ sq, int64_t rows, int C,
                                                                 float eps) {
#include "rmsnorm_rope_q8_body.inc"
}

// The batched forms (include/fairygen_hip_batch8.h): the last grid dimension picks the batch element — `rows` rows of the one matrix x,
// the table rows 0 .. rows - 1 — and the element runs the body of the single-element kernel on its own pointers.
template <bool F32TAB>
__global__ __launch_bounds__(256, 4) void rmsnorm_rope_q8_b_kernel(const bf16* __restrict__ x, int64_t ldx, const bf16* __restrict__ w,
                                                                   const void* __restrict__ ctv, const void* __restrict__ stv,
                                                                   uint8_t* __restrict__ q8, float* __restrict__ sq, int64_t rows, int C,
                                                                   float eps) {
    const int64_t r0 = (int64_t)blockIdx.y * rows;
    x += r0 * ldx; q8 += r0 * C; sq += r0 * (C >> 7);
#include "rmsnorm_rope_q8_body.inc"
}

// The norm of rmsnorm_rope_kernel over the rows 4 (blockIdx + gridDim i) + wave, NV = ceil(C / 512) vectors a lane: every lane keeps
// the statistics of its own channels over the rows its wave walked; at the end the four waves' are combined through LDS (waves 1..3
// in turn, wave 0 adds) and wave 0 writes the workgroup's record.
template <bool F32TAB, int NV>
__global__ __launch_bounds__(256) void rmsnorm_rope_kstats_kernel(const bf16* __restrict__ x, int64_t ldx, const bf16* __restrict__ w,
                                                                  const void* __restrict__ ctv, const void* __restrict__ stv,
                                                                  bf16* __restrict__ out, double* __restrict__ psum,
                                                                  float* __restrict__ pmin, float* __restrict__ pmax, int64_t rows,
                                                                  int C, float eps) {
#include "rmsnorm_rope_kstats_body.inc"
}

// batched: element blockIdx.y; its partials block (gridDim.x records: sums, minima, maxima) lies bs_partials bytes behind the previous one
template <bool F32TAB, int NV>
__global__ __launch_bounds__(256) void rmsnorm_rope_kstats_b_kernel(const bf16* __restrict__ x, int64_t ldx, const bf16* __restrict__ w,
                                                                    const void* __restrict__ ctv, const void* __restrict__ stv,
                                                                    bf16* __restrict__ out, char* __restrict__ partials,
                                                                    int64_t bs_partials, int64_t rows, int C, float eps) {
    const int64_t r0 = (int64_t)blockIdx.y * rows, pc = (int64_t)gridDim.x * C;
    double* __restrict__ psum = reinterpret_cast<double*>(partials + (int64_t)blockIdx.y * bs_partials);
    float* __restrict__ pmin = reinterpret_cast<float*>(psum + pc);
    float* __restrict__ pmax = pmin + pc;
    x += r0 * ldx; out += r0 * C;
#include "rmsnorm_rope_kstats_body.inc"
}

// One workgroup of 1024 per head: thread t reduces channel t & 127 over the records (t >> 7) + 8 i, LDS joins the 8 groups.
__global__ __launch_bounds__(1024) void attn_k_finalise_kernel(const double* __restrict__ psum, const float* __restrict__ pmin,
                                                               const float* __restrict__ pmax, int P, int C, float* __restrict__ kbar,
                                                               float* __restrict__ sk, int64_t N) {
#include "attn_k_finalise_body.inc"
}

struct QuantKStrides {
    int64_t k, partials, k8, sk, kbar;
};

__global__ __launch_bounds__(1024) void attn_k_finalise_b_kernel(const char* __restrict__ partials, int P, int C, float* __restrict__ kbar,
                                                                 float* __restrict__ sk, int64_t N, const QuantKStrides bs) {
    const int64_t b = blockIdx.y, pc = (int64_t)P * C;
    const double* __restrict__ psum = reinterpret_cast<const double*>(partials + b * bs.partials);
    const float* __restrict__ pmin = reinterpret_cast<const float*>(psum + pc);
    const float* __restrict__ pmax = pmin + pc;
    kbar += b * bs.kbar; sk += b * bs.sk;
#include "attn_k_finalise_body.inc"
}

// The k half of attn_quant_qk_kernel: 16 rows of one head per workgroup of 256, 16 lanes x 8 channels cover a row.
__device__ __forceinline__ void attn_quant_k_body(const bf16* __restrict__ k, int64_t ldk, const float* __restrict__ kbar,
                                                  const float* __restrict__ sk, uint8_t* __restrict__ k8, int64_t N, int H) {
    const int h = blockIdx.y, tid = threadIdx.x, c = tid & 15;
    const int64_t row = (int64_t)blockIdx.x * 16 + (tid >> 4);
    if (row >= N) return;
    const bf16x8 kv = *reinterpret_cast<const bf16x8*>(k + row * ldk + (int64_t)h * kD + c * 8);
    const f32x4 m0 = *reinterpret_cast<const f32x4*>(kbar + h * kD + c * 8), m1 = *reinterpret_cast<const f32x4*>(kbar + h * kD + c * 8 + 4);
    const float s_k = sk[h];
    float kf[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) kf[j] = (float)kv[j] - (j < 4 ? m0[j & 3] : m1[j & 3]);
    *reinterpret_cast<u32x2*>(k8 + (row * H + h) * kD + c * 8) = quant8_e4m3(kf, s_k);
}

__global__ __launch_bounds__(256) void attn_quant_k_kernel(const bf16* __restrict__ k, int64_t ldk, const float* __restrict__ kbar,
                                                           const float* __restrict__ sk, uint8_t* __restrict__ k8, int64_t N, int H) {
    attn_quant_k_body(k, ldk, kbar, sk, k8, N, H);
}

__global__ __launch_bounds__(256) void attn_quant_k_b_kernel(const bf16* __restrict__ k, int64_t ldk, const float* __restrict__ kbar,
                                                             const float* __restrict__ sk, uint8_t* __restrict__ k8, int64_t N, int H,
                                                             const QuantKStrides bs) {
    const int64_t b = blockIdx.z;
    attn_quant_k_body(k + b * bs.k, ldk, kbar + b * bs.kbar, sk + b * bs.sk, k8 + b * bs.k8, N, H);
}

// The checks the two producers share; C = num_heads * 128 <= 4096.
int check_producer(const char* fn, const void* x, int64_t ldx, const void* weight, const void* cos_tab, const void* sin_tab, int table_f32,
                   int64_t rows, int C, int num_heads) {
    FG_CHECK_ARG(x && weight, "%s: null pointer", fn);
    FG_CHECK_ARG(rows > 0 && (rows + kRowsPerBlock - 1) / kRowsPerBlock < (1ll << 31), "%s: rows must be positive (got %lld)", fn, (long long)rows);
    FG_CHECK_ARG(num_heads > 0 && num_heads <= kMaxVec * 4 && C == num_heads * kD,
                 "%s: only head_dim 128 is supported: C must be num_heads * 128, at most %d (got C=%d, num_heads=%d)", fn, kMaxVec * 512, C,
                 num_heads);
    FG_CHECK_ARG(table_f32 ? (cos_tab != nullptr && sin_tab == nullptr) : ((cos_tab == nullptr) == (sin_tab == nullptr)),
                 "%s: fp64 mode takes both tables or neither, fp32 mode ONE interleaved table in cos_tab", fn);
    FG_CHECK_ARG(ldx >= C && ldx % 8 == 0, "%s: ldx must be >= C and a multiple of 8", fn);
    FG_CHECK_ARG(FG_ALIGNED16(x) && FG_ALIGNED16(weight) && FG_ALIGNED16(cos_tab) && FG_ALIGNED16(sin_tab),
                 "%s: x, weight and the tables must be 16-byte aligned", fn);
    return FG_OK;
}

}  // namespace

extern "C" int fg_attn_qk8_fused_version(void) { return 1; }

extern "C" int64_t fg_attn_qk8_fused_scratch_bytes(int64_t rows, int C) {
    if (rows < 1 || C < kD || C % kD != 0 || C > kMaxVec * 512) {
        fg_set_error("fg_attn_qk8_fused_scratch_bytes: rows must be positive, C a multiple of 128 up to %d (got rows=%lld C=%d)", kMaxVec * 512,
                     (long long)rows, C);
        return -1;
    }
    return partials_bytes_for(rows, C);
}

extern "C" int fg_rmsnorm_rope_q8_bf16(const void* x, int64_t ldx, const void* weight, const void* cos_tab, const void* sin_tab,
                                       int table_f32, void* q8, float* sq, int64_t rows, int C, int num_heads, float eps,
                                       fg_stream_t stream) {
    FG_CHECK_ARG(q8 && sq, "fg_rmsnorm_rope_q8_bf16: null pointer");
    if (int e = check_producer("fg_rmsnorm_rope_q8_bf16", x, ldx, weight, cos_tab, sin_tab, table_f32, rows, C, num_heads)) return e;
    FG_CHECK_ARG((((uintptr_t)q8) & 7) == 0 && (((uintptr_t)sq) & 3) == 0, "fg_rmsnorm_rope_q8_bf16: q8 must be 8-byte aligned (sq: 4)");
    const dim3 grid((unsigned)((rows + kRowsPerBlock - 1) / kRowsPerBlock));
    if (table_f32)
        hipLaunchKernelGGL(rmsnorm_rope_q8_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)x, ldx, (const bf16*)weight,
                           cos_tab, sin_tab, (uint8_t*)q8, sq, rows, C, eps);
    else
        hipLaunchKernelGGL(rmsnorm_rope_q8_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)x, ldx, (const bf16*)weight,
                           cos_tab, sin_tab, (uint8_t*)q8, sq, rows, C, eps);
    return fg_launch_status("fg_rmsnorm_rope_q8_bf16");
}

extern "C" int fg_rmsnorm_rope_kstats_bf16(const void* x, int64_t ldx, const void* weight, const void* cos_tab, const void* sin_tab,
                                           int table_f32, void* k_out, void* partials, int64_t partials_bytes, int64_t rows, int C,
                                           int num_heads, float eps, fg_stream_t stream) {
    FG_CHECK_ARG(k_out && partials, "fg_rmsnorm_rope_kstats_bf16: null pointer");
    if (int e = check_producer("fg_rmsnorm_rope_kstats_bf16", x, ldx, weight, cos_tab, sin_tab, table_f32, rows, C, num_heads)) return e;
    FG_CHECK_ARG(FG_ALIGNED16(k_out) && FG_ALIGNED16(partials), "fg_rmsnorm_rope_kstats_bf16: k_out and partials must be 16-byte aligned");
    FG_CHECK_ARG(partials_bytes >= partials_bytes_for(rows, C), "fg_rmsnorm_rope_kstats_bf16: partials must hold %lld bytes (got %lld)",
                 (long long)partials_bytes_for(rows, C), (long long)partials_bytes);
    const int64_t P = stat_parts(rows);
    double* psum = (double*)partials;
    float* pmin = (float*)(psum + P * C);
    float* pmax = pmin + P * C;
#define FG_KSTATS_LAUNCH(TAB, NV)                                                                                                       \
    hipLaunchKernelGGL((rmsnorm_rope_kstats_kernel<TAB, NV>), dim3((unsigned)P), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, ldx, \
                       (const bf16*)weight, cos_tab, sin_tab, (bf16*)k_out, psum, pmin, pmax, rows, C, eps)
#define FG_KSTATS_CASE(NV)                                            \
    case NV:                                                          \
        if (table_f32) FG_KSTATS_LAUNCH(true, NV);                    \
        else FG_KSTATS_LAUNCH(false, NV);                             \
        break;
    switch ((C + 511) / 512) {
        FG_KSTATS_CASE(1) FG_KSTATS_CASE(2) FG_KSTATS_CASE(3) FG_KSTATS_CASE(4)
        FG_KSTATS_CASE(5) FG_KSTATS_CASE(6) FG_KSTATS_CASE(7) FG_KSTATS_CASE(8)
    }
#undef FG_KSTATS_CASE
#undef FG_KSTATS_LAUNCH
    return fg_launch_status("fg_rmsnorm_rope_kstats_bf16");
}

extern "C" int fg_attn_quant_k_bf16(const void* k, int64_t ldk, const void* partials, int64_t partials_bytes, void* k8, float* sk,
                                    float* kbar, int64_t N, int H, int D, fg_stream_t stream) {
    FG_CHECK_ARG(k && partials && k8 && sk && kbar, "fg_attn_quant_k_bf16: null pointer");
    FG_CHECK_ARG(D == kD, "fg_attn_quant_k_bf16: only head_dim 128 is supported (got %d)", D);
    FG_CHECK_ARG(N > 0 && H > 0 && H <= kMaxVec * 4, "fg_attn_quant_k_bf16: N must be positive, H in 1..%d", kMaxVec * 4);
    const int C = H * kD;
    FG_CHECK_ARG(ldk >= C && ldk % 8 == 0, "fg_attn_quant_k_bf16: ldk must be >= H*D and a multiple of 8");
    FG_CHECK_ARG(FG_ALIGNED16(k) && FG_ALIGNED16(partials) && FG_ALIGNED16(kbar) && (((uintptr_t)k8) & 7) == 0 && (((uintptr_t)sk) & 3) == 0,
                 "fg_attn_quant_k_bf16: k, partials, kbar must be 16-byte aligned (k8: 8; sk: 4)");
    FG_CHECK_ARG(partials_bytes >= partials_bytes_for(N, C), "fg_attn_quant_k_bf16: partials must hold %lld bytes (got %lld)",
                 (long long)partials_bytes_for(N, C), (long long)partials_bytes);
    FG_CHECK_ARG((N + 15) / 16 < (1ll << 31), "fg_attn_quant_k_bf16: grid too large");
    const int64_t P = stat_parts(N);
    const double* psum = (const double*)partials;
    const float* pmin = (const float*)(psum + P * C);
    const float* pmax = pmin + P * C;
    hipLaunchKernelGGL(attn_k_finalise_kernel, dim3((unsigned)H), dim3(1024), 0, (hipStream_t)stream, psum, pmin, pmax, (int)P, C, kbar, sk, N);
    if (int e = fg_launch_status("fg_attn_quant_k_bf16 (k statistics)")) return e;
    hipLaunchKernelGGL(attn_quant_k_kernel, dim3((unsigned)((N + 15) / 16), (unsigned)H), dim3(256), 0, (hipStream_t)stream, (const bf16*)k, ldk,
                       (const float*)kbar, (const float*)sk, (uint8_t*)k8, N, H);
    return fg_launch_status("fg_attn_quant_k_bf16");
}

// ---- the batched forms (include/fairygen_hip_batch8.h): the same launches with the batch as one more grid dimension
extern "C" int fg_rmsnorm_rope_q8_bf16_b(const void* x, int64_t ldx, const void* weight, const void* cos_tab, const void* sin_tab,
                                         int table_f32, void* q8, float* sq, int B, int64_t rows, int C, int num_heads, float eps,
                                         fg_stream_t stream) {
    FG_CHECK_ARG(q8 && sq, "fg_rmsnorm_rope_q8_bf16_b: null pointer");
    FG_CHECK_ARG(B >= 1 && B <= 65535, "fg_rmsnorm_rope_q8_bf16_b: B must be in 1..65535 (got %d)", B);
    if (int e = check_producer("fg_rmsnorm_rope_q8_bf16_b", x, ldx, weight, cos_tab, sin_tab, table_f32, rows, C, num_heads)) return e;
    FG_CHECK_ARG((((uintptr_t)q8) & 7) == 0 && (((uintptr_t)sq) & 3) == 0, "fg_rmsnorm_rope_q8_bf16_b: q8 must be 8-byte aligned (sq: 4)");
    const dim3 grid((unsigned)((rows + kRowsPerBlock - 1) / kRowsPerBlock), (unsigned)B);
    if (table_f32)
        hipLaunchKernelGGL(rmsnorm_rope_q8_b_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)x, ldx, (const bf16*)weight,
                           cos_tab, sin_tab, (uint8_t*)q8, sq, rows, C, eps);
    else
        hipLaunchKernelGGL(rmsnorm_rope_q8_b_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)x, ldx, (const bf16*)weight,
                           cos_tab, sin_tab, (uint8_t*)q8, sq, rows, C, eps);
    return fg_launch_status("fg_rmsnorm_rope_q8_bf16_b");
}

extern "C" int fg_rmsnorm_rope_kstats_bf16_b(const void* x, int64_t ldx, const void* weight, const void* cos_tab, const void* sin_tab,
                                             int table_f32, void* k_out, void* partials, int64_t partials_bytes, int64_t bs_partials, int B,
                                             int64_t rows, int C, int num_heads, float eps, fg_stream_t stream) {
    FG_CHECK_ARG(k_out && partials, "fg_rmsnorm_rope_kstats_bf16_b: null pointer");
    FG_CHECK_ARG(B >= 1 && B <= 65535, "fg_rmsnorm_rope_kstats_bf16_b: B must be in 1..65535 (got %d)", B);
    if (int e = check_producer("fg_rmsnorm_rope_kstats_bf16_b", x, ldx, weight, cos_tab, sin_tab, table_f32, rows, C, num_heads)) return e;
    FG_CHECK_ARG(FG_ALIGNED16(k_out) && FG_ALIGNED16(partials), "fg_rmsnorm_rope_kstats_bf16_b: k_out and partials must be 16-byte aligned");
    FG_CHECK_ARG(partials_bytes >= partials_bytes_for(rows, C),
                 "fg_rmsnorm_rope_kstats_bf16_b: partials must hold %lld bytes per element (got %lld)", (long long)partials_bytes_for(rows, C),
                 (long long)partials_bytes);
    FG_CHECK_ARG(bs_partials >= partials_bytes_for(rows, C) && bs_partials % 16 == 0,
                 "fg_rmsnorm_rope_kstats_bf16_b: the batch stride of partials must cover one element's block and be a multiple of 16");
    const int64_t P = stat_parts(rows);
#define FG_KSTATS_LAUNCH(TAB, NV)                                                                                                      \
    hipLaunchKernelGGL((rmsnorm_rope_kstats_b_kernel<TAB, NV>), dim3((unsigned)P, (unsigned)B), dim3(256), 0, (hipStream_t)stream,      \
                       (const bf16*)x, ldx, (const bf16*)weight, cos_tab, sin_tab, (bf16*)k_out, (char*)partials, bs_partials, rows, C, eps)
#define FG_KSTATS_CASE(NV)                                            \
    case NV:                                                          \
        if (table_f32) FG_KSTATS_LAUNCH(true, NV);                    \
        else FG_KSTATS_LAUNCH(false, NV);                             \
        break;
    switch ((C + 511) / 512) {
        FG_KSTATS_CASE(1) FG_KSTATS_CASE(2) FG_KSTATS_CASE(3) FG_KSTATS_CASE(4)
        FG_KSTATS_CASE(5) FG_KSTATS_CASE(6) FG_KSTATS_CASE(7) FG_KSTATS_CASE(8)
    }
#undef FG_KSTATS_CASE
#undef FG_KSTATS_LAUNCH
    return fg_launch_status("fg_rmsnorm_rope_kstats_bf16_b");
}

extern "C" int fg_attn_quant_k_bf16_b(const void* k, int64_t ldk, int64_t bs_k, const void* partials, int64_t partials_bytes,
                                      int64_t bs_partials, void* k8, int64_t bs_k8, float* sk, int64_t bs_sk, float* kbar, int64_t bs_kbar,
                                      int B, int64_t N, int H, int D, fg_stream_t stream) {
    FG_CHECK_ARG(k && partials && k8 && sk && kbar, "fg_attn_quant_k_bf16_b: null pointer");
    FG_CHECK_ARG(D == kD, "fg_attn_quant_k_bf16_b: only head_dim 128 is supported (got %d)", D);
    FG_CHECK_ARG(B >= 1 && B <= 65535, "fg_attn_quant_k_bf16_b: B must be in 1..65535 (got %d)", B);
    FG_CHECK_ARG(N > 0 && H > 0 && H <= kMaxVec * 4, "fg_attn_quant_k_bf16_b: N must be positive, H in 1..%d", kMaxVec * 4);
    const int C = H * kD;
    FG_CHECK_ARG(ldk >= C && ldk % 8 == 0, "fg_attn_quant_k_bf16_b: ldk must be >= H*D and a multiple of 8");
    FG_CHECK_ARG(FG_ALIGNED16(k) && FG_ALIGNED16(partials) && FG_ALIGNED16(kbar) && (((uintptr_t)k8) & 7) == 0 && (((uintptr_t)sk) & 3) == 0,
                 "fg_attn_quant_k_bf16_b: k, partials, kbar must be 16-byte aligned (k8: 8; sk: 4)");
    FG_CHECK_ARG(partials_bytes >= partials_bytes_for(N, C), "fg_attn_quant_k_bf16_b: partials must hold %lld bytes per element (got %lld)",
                 (long long)partials_bytes_for(N, C), (long long)partials_bytes);
    FG_CHECK_ARG(bs_k >= (N - 1) * ldk + C && bs_partials >= partials_bytes_for(N, C) && bs_k8 >= N * C && bs_sk >= H && bs_kbar >= C,
                 "fg_attn_quant_k_bf16_b: a batch stride is smaller than one element of its operand");
    FG_CHECK_ARG(bs_k % 8 == 0 && bs_partials % 16 == 0 && bs_k8 % 8 == 0 && bs_kbar % 4 == 0,
                 "fg_attn_quant_k_bf16_b: batch strides must keep the alignment (k: 8 elements; partials: 16 bytes; k8: 8 bytes; kbar: 4 floats)");
    FG_CHECK_ARG((N + 15) / 16 < (1ll << 31), "fg_attn_quant_k_bf16_b: grid too large");
    const int64_t P = stat_parts(N);
    const QuantKStrides bs{bs_k, bs_partials, bs_k8, bs_sk, bs_kbar};
    hipLaunchKernelGGL(attn_k_finalise_b_kernel, dim3((unsigned)H, (unsigned)B), dim3(1024), 0, (hipStream_t)stream, (const char*)partials,
                       (int)P, C, kbar, sk, N, bs);
    if (int e = fg_launch_status("fg_attn_quant_k_bf16_b (k statistics)")) return e;
    hipLaunchKernelGGL(attn_quant_k_b_kernel, dim3((unsigned)((N + 15) / 16), (unsigned)H, (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                       (const bf16*)k, ldk, (const float*)kbar, (const float*)sk, (uint8_t*)k8, N, H, bs);
    return fg_launch_status("fg_attn_quant_k_bf16_b");
}
