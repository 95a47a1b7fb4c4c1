// The e4m3 operands of the 8-bit self-attention with V mean-smoothed on a token shard (include/fairygen_hip_shard8s.h), for gfx950:
// attn_shard8.hip with a record that carries for v what it carries for k.
//
// The N keys are sharded by rows over W ranks; the key mean, sk, mu (the key mean of v) and sv are statistics over all of them.  Per rank
// and block:
//   1. fg_attn_shard8s_stats: the rank's partial key records (fg_rmsnorm_rope_kstats_bf16) and ONE walk over its v rows (the pass 1 of the
//      smoothing V producer, attn_smoothv_parts.h) -> ONE record: per channel the fp64 sum, the minimum and the maximum of k, and of v;
//   2. the W records are all-gathered by the host (W * 32 * C bytes);
//   3. fg_attn_shard8s_quant: every rank reduces the W records in rank order — for k with the expressions of shard8_finalise_kernel
//      (attn_shard8.hip), for v with smoothv_scale (attn_smoothv_parts.h: the expressions of attn_quant_vt_smooth_kernel) — then converts its
//      rows: k8 as shard8_quant_kernel, v8 = e4m3(fl32(v - mu) / sv) row-major, the division of attn_quant_vt_body.inc;
//   4. the host all-gathers k8 and v8; 5. fg_attn_shard8_vt (attn_shard8.hip) transposes the gathered v8 into tiles.
// An exact fp64 sum, a minimum and a maximum do not depend on the order, so the bytes are those of the unsharded producers.
// The row walks are HBM-bound; no atomics, nothing waits on another workgroup.
#include "common.h"
#include "../../include/fairygen_hip_shard8s.h"
#include "attn_qk8_quant.h"
#include "attn_pv8_parts.h"
#include "attn_smoothv_parts.h"

#include <math.h>

namespace {

constexpr int kMaxHeads = 32;      // C <= 4096, the fused producers' limit
constexpr int kRecordBytes = 32;   // per channel: two of (fp64 sum, fp32 minimum, fp32 maximum)

__global__ __launch_bounds__(256) void shard8s_v_stats_kernel(const bf16* __restrict__ v, int64_t ldv, double* __restrict__ rsum,
                                                              float* __restrict__ rlo, float* __restrict__ rhi, int64_t rows, int C) {
    attn_v_stats_smooth_body(v, ldv, rsum, rlo, rhi, rows, C);
}

// One statistic triple (fp64 sum, minimum, maximum) of channel c of head h over the `n` records of a [n][C] layout: thread group g of 8
// takes the records g, g + 8, .. in that order, LDS joins the groups in the order 0, 1, .., 7.  Every thread of the 1024 calls it; the
// result is valid in the first 128.
__device__ __forceinline__ void join8(const double* __restrict__ psum, const float* __restrict__ pmin, const float* __restrict__ pmax,
                                      int n, int C, int ch, int c, int g, double& s, float& lo, float& hi) {
    __shared__ double sum_s[8][kD];
    __shared__ float min_s[8][kD], max_s[8][kD];
    s = 0.0;
    lo = INFINITY;
    hi = -INFINITY;
    for (int p = g; p < n; p += 8) {
        const int64_t o = (int64_t)p * C + ch;
        s += psum[o];
        lo = fminf(lo, pmin[o]);
        hi = fmaxf(hi, pmax[o]);
    }
    __syncthreads();      // the previous call's reads of the three arrays are done
    sum_s[g][c] = s;
    min_s[g][c] = lo;
    max_s[g][c] = hi;
    __syncthreads();
    if (g) return;
#pragma unroll
    for (int i = 1; i < 8; ++i) {
        s += sum_s[i][c];
        lo = fminf(lo, min_s[i][c]);
        hi = fmaxf(hi, max_s[i][c]);
    }
}

// One workgroup of 1024 per head, as shard8_record_kernel: the P key partials, then the VP row strides of v, into the head's slices of the
// six fields of the record.
__global__ __launch_bounds__(1024) void shard8s_record_kernel(const double* __restrict__ psum, const float* __restrict__ pmin,
                                                              const float* __restrict__ pmax, int P, const double* __restrict__ vsum,
                                                              const float* __restrict__ vmin, const float* __restrict__ vmax, int VP, int C,
                                                              uint8_t* __restrict__ record) {
    const int h = blockIdx.x, tid = threadIdx.x, c = tid & (kD - 1), g = tid >> 7, ch = h * kD + c;
    double s;
    float lo, hi;
    join8(psum, pmin, pmax, P, C, ch, c, g, s, lo, hi);
    if (g == 0) {
        reinterpret_cast<double*>(record)[ch] = s;
        reinterpret_cast<float*>(record + (int64_t)8 * C)[ch] = lo;
        reinterpret_cast<float*>(record + (int64_t)12 * C)[ch] = hi;
    }
    join8(vsum, vmin, vmax, VP, C, ch, c, g, s, lo, hi);
    if (g == 0) {
        reinterpret_cast<double*>(record + (int64_t)16 * C)[ch] = s;
        reinterpret_cast<float*>(record + (int64_t)24 * C)[ch] = lo;
        reinterpret_cast<float*>(record + (int64_t)28 * C)[ch] = hi;
    }
}

// One workgroup of 128 per head: thread c walks the W records in rank order.  k: the expressions of shard8_finalise_kernel; v: smoothv_scale.
__global__ __launch_bounds__(128) void shard8s_finalise_kernel(const uint8_t* __restrict__ records, int W, int C, int64_t N,
                                                               float* __restrict__ kbar, float* __restrict__ sk, float* __restrict__ sv,
                                                               float* __restrict__ mu) {
    __shared__ float amax_s[2];
    const int h = blockIdx.x, tid = threadIdx.x, ch = h * kD + tid;
    double s = 0.0, vs = 0.0;
    float lo = INFINITY, hi = -INFINITY, vlo = INFINITY, vhi = -INFINITY;
    for (int w = 0; w < W; ++w) {
        const uint8_t* r = records + (int64_t)w * kRecordBytes * C;
        s += reinterpret_cast<const double*>(r)[ch];
        lo = fminf(lo, reinterpret_cast<const float*>(r + (int64_t)8 * C)[ch]);
        hi = fmaxf(hi, reinterpret_cast<const float*>(r + (int64_t)12 * C)[ch]);
        vs += reinterpret_cast<const double*>(r + (int64_t)16 * C)[ch];
        vlo = fminf(vlo, reinterpret_cast<const float*>(r + (int64_t)24 * C)[ch]);
        vhi = fmaxf(vhi, reinterpret_cast<const float*>(r + (int64_t)28 * C)[ch]);
    }
    const float m = (float)(s / (double)N);
    kbar[ch] = m;
    float vm, vscale;
    smoothv_scale(vs, vlo, vhi, N, vm, vscale);
    mu[ch] = vm;
    sv[ch] = vscale;
    const float amax = wave_max(fmaxf(hi - m, m - lo));
    if ((tid & 63) == 0) amax_s[tid >> 6] = amax;
    __syncthreads();
    if (tid == 0) sk[h] = fmaxf(fmaxf(amax_s[0], amax_s[1]) / kE4M3Max, kScaleFloor);
}

// shard8_quant_kernel with the mean of v taken out: 16 rows of one head per workgroup of 256, 16 lanes x 8 channels cover a row.
__global__ __launch_bounds__(256) void shard8s_quant_kernel(const bf16* __restrict__ k, int64_t ldk, const bf16* __restrict__ v, int64_t ldv,
                                                            const float* __restrict__ kbar, const float* __restrict__ sk,
                                                            const float* __restrict__ sv, const float* __restrict__ mu,
                                                            uint8_t* __restrict__ k8, uint8_t* __restrict__ v8, int64_t rows, int H) {
    const int h = blockIdx.y, tid = threadIdx.x, c = tid & 15;
    const int64_t row = (int64_t)blockIdx.x * 16 + (tid >> 4);
    if (row >= rows) return;
    const int ch = h * kD + c * 8;
    const bf16x8 kv = *reinterpret_cast<const bf16x8*>(k + row * ldk + ch);
    const f32x4 m0 = *reinterpret_cast<const f32x4*>(kbar + ch), m1 = *reinterpret_cast<const f32x4*>(kbar + ch + 4);
    const float s_k = sk[h];
    float kf[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) kf[j] = (float)kv[j] - (j < 4 ? m0[j & 3] : m1[j & 3]);
    const int64_t o = (row * H + h) * kD + c * 8;
    *reinterpret_cast<u32x2*>(k8 + o) = quant8_e4m3(kf, s_k);
    const bf16x8 vv = *reinterpret_cast<const bf16x8*>(v + row * ldv + ch);
    const f32x4 s0 = *reinterpret_cast<const f32x4*>(sv + ch), s1 = *reinterpret_cast<const f32x4*>(sv + ch + 4);
    const f32x4 u0 = *reinterpret_cast<const f32x4*>(mu + ch), u1 = *reinterpret_cast<const f32x4*>(mu + ch + 4);
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float d = (float)vv[j] - (j < 4 ? u0[j & 3] : u1[j & 3]);
        f[j] = d / (j < 4 ? s0[j & 3] : s1[j & 3]);
    }
    u32x2 w;
    w[0] = cvt2_e4m3(f[0], f[1]) | (cvt2_e4m3(f[2], f[3]) << 16);
    w[1] = cvt2_e4m3(f[4], f[5]) | (cvt2_e4m3(f[6], f[7]) << 16);
    *reinterpret_cast<u32x2*>(v8 + o) = w;
}

bool channels_ok(int C) { return C >= kD && C % kD == 0 && C <= kMaxHeads * kD; }

}  // namespace

extern "C" int fg_attn_shard8s_version(void) { return 1; }

extern "C" int64_t fg_attn_shard8s_record_bytes(int C) {
    if (!channels_ok(C)) {
        fg_set_error("fg_attn_shard8s_record_bytes: C must be a multiple of 128 up to %d (got %d)", kMaxHeads * kD, C);
        return -1;
    }
    return (int64_t)kRecordBytes * C;
}

extern "C" int64_t fg_attn_shard8s_scratch_bytes(int64_t rows, int C) {
    if (rows < 1 || !channels_ok(C)) {
        fg_set_error("fg_attn_shard8s_scratch_bytes: rows must be positive, C a multiple of 128 up to %d (got rows=%lld C=%d)", kMaxHeads * kD,
                     (long long)rows, C);
        return -1;
    }
    return v_stat_parts(rows) * C * 16;
}

extern "C" int fg_attn_shard8s_stats(const void* partials, int64_t partials_bytes, const void* v, int64_t ldv, void* record,
                                     int64_t record_bytes, void* scratch, int64_t scratch_bytes, int64_t rows, int H, int D,
                                     fg_stream_t stream) {
    FG_CHECK_ARG(partials && record && v && scratch, "fg_attn_shard8s_stats: null pointer");
    FG_CHECK_ARG(D == kD, "fg_attn_shard8s_stats: only head_dim 128 is supported (got %d)", D);
    FG_CHECK_ARG(rows > 0 && H > 0 && H <= kMaxHeads, "fg_attn_shard8s_stats: rows must be positive, H in 1..%d", kMaxHeads);
    const int C = H * kD;
    const int64_t need = fg_attn_qk8_fused_scratch_bytes(rows, C);      // P records of 16 C bytes: the layout of the key producer
    FG_CHECK_ARG(need > 0 && partials_bytes >= need, "fg_attn_shard8s_stats: partials must hold %lld bytes (got %lld)", (long long)need,
                 (long long)partials_bytes);
    FG_CHECK_ARG(record_bytes >= (int64_t)kRecordBytes * C, "fg_attn_shard8s_stats: the record must hold %lld bytes (got %lld)",
                 (long long)kRecordBytes * C, (long long)record_bytes);
    FG_CHECK_ARG(FG_ALIGNED16(partials) && FG_ALIGNED16(record) && FG_ALIGNED16(v) && FG_ALIGNED16(scratch),
                 "fg_attn_shard8s_stats: partials, v, record and scratch must be 16-byte aligned");
    FG_CHECK_ARG(ldv >= C && ldv % 8 == 0, "fg_attn_shard8s_stats: ldv must be >= H*D and a multiple of 8");
    const int64_t P = need / ((int64_t)16 * C), VP = v_stat_parts(rows);
    FG_CHECK_ARG(scratch_bytes >= VP * C * 16, "fg_attn_shard8s_stats: scratch must hold %lld bytes (got %lld)", (long long)(VP * C * 16),
                 (long long)scratch_bytes);
    double* vsum = (double*)scratch;
    float* vmin = (float*)(vsum + VP * C);
    float* vmax = vmin + VP * C;
    hipLaunchKernelGGL(shard8s_v_stats_kernel, dim3((unsigned)VP, (unsigned)((C / 8 + 63) / 64)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16*)v, ldv, vsum, vmin, vmax, rows, C);
    if (int e = fg_launch_status("fg_attn_shard8s_stats (v statistics)")) return e;
    const double* psum = (const double*)partials;
    const float* pmin = (const float*)(psum + P * C);
    hipLaunchKernelGGL(shard8s_record_kernel, dim3((unsigned)H), dim3(1024), 0, (hipStream_t)stream, psum, pmin, pmin + P * C, (int)P,
                       (const double*)vsum, (const float*)vmin, (const float*)vmax, (int)VP, C, (uint8_t*)record);
    return fg_launch_status("fg_attn_shard8s_stats");
}

extern "C" int fg_attn_shard8s_quant(const void* records, int64_t records_bytes, int W, int64_t N, const void* k, int64_t ldk, const void* v,
                                     int64_t ldv, void* k8, void* v8, float* sk, float* kbar, float* sv, float* mu, int64_t rows, int H,
                                     int D, fg_stream_t stream) {
    FG_CHECK_ARG(records && k && v && k8 && v8 && sk && kbar && sv && mu, "fg_attn_shard8s_quant: null pointer");
    FG_CHECK_ARG(D == kD, "fg_attn_shard8s_quant: only head_dim 128 is supported (got %d)", D);
    FG_CHECK_ARG(H > 0 && H <= kMaxHeads, "fg_attn_shard8s_quant: H in 1..%d", kMaxHeads);
    FG_CHECK_ARG(W >= 1 && N >= 1, "fg_attn_shard8s_quant: W and N must be positive (got W=%d N=%lld)", W, (long long)N);
    FG_CHECK_ARG(rows >= 1 && rows <= N, "fg_attn_shard8s_quant: 1 <= rows <= N (got rows=%lld N=%lld)", (long long)rows, (long long)N);
    const int C = H * kD;
    FG_CHECK_ARG(records_bytes >= (int64_t)W * kRecordBytes * C, "fg_attn_shard8s_quant: records must hold W * 32 * C = %lld bytes (got %lld)",
                 (long long)W * kRecordBytes * C, (long long)records_bytes);
    FG_CHECK_ARG(ldk >= C && ldk % 8 == 0 && ldv >= C && ldv % 8 == 0,
                 "fg_attn_shard8s_quant: leading dimensions must be >= H*D and multiples of 8");
    FG_CHECK_ARG(FG_ALIGNED16(records) && FG_ALIGNED16(k) && FG_ALIGNED16(v) && FG_ALIGNED16(kbar) && FG_ALIGNED16(sv) && FG_ALIGNED16(mu) &&
                     (((uintptr_t)k8 | (uintptr_t)v8) & 7) == 0 && (((uintptr_t)sk) & 3) == 0,
                 "fg_attn_shard8s_quant: records, k, v, kbar, sv, mu must be 16-byte aligned (k8, v8: 8; sk: 4)");
    FG_CHECK_ARG((rows + 15) / 16 < (1ll << 31), "fg_attn_shard8s_quant: grid too large");
    hipLaunchKernelGGL(shard8s_finalise_kernel, dim3((unsigned)H), dim3(128), 0, (hipStream_t)stream, (const uint8_t*)records, W, C, N, kbar, sk,
                       sv, mu);
    if (int e = fg_launch_status("fg_attn_shard8s_quant (scales)")) return e;
    hipLaunchKernelGGL(shard8s_quant_kernel, dim3((unsigned)((rows + 15) / 16), (unsigned)H), dim3(256), 0, (hipStream_t)stream, (const bf16*)k,
                       ldk, (const bf16*)v, ldv, (const float*)kbar, (const float*)sk, (const float*)sv, (const float*)mu, (uint8_t*)k8,
                       (uint8_t*)v8, rows, H);
    return fg_launch_status("fg_attn_shard8s_quant");
}
