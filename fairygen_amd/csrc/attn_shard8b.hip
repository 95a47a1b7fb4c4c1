// The producers of a token shard (attn_shard8.hip, attn_shard8s.hip) on a batch of B elements that share the row count
// (include/fairygen_hip_shard8b.h), for gfx950: the stacked CFG forward on a rank of the K / V all-gather layout.
//
// Every kernel here is the body of its single-element form with the element in the grid (blockIdx.z, or blockIdx.y where the single form
// has a one-dimensional grid) and the element's operands found by a stride: one launch sequence per batch, the same expressions in the
// same order per element, so element b's bytes are those of the single-element entry point on element b alone
// (tests/test_attention_shard8b.py).  Every statistic is per element and head.  The single forms' files are not touched.
// Layouts: one record per element, (B, 20 C) or (B, 32 C); the gathered records (W, B, record bytes); kbar, sk, sv, mu with a leading B.
// The row walks are HBM-bound; no atomics, nothing waits on another workgroup.
#include "common.h"
#include "../../include/fairygen_hip_shard8b.h"
#include "attn_qk8_quant.h"
#include "attn_pv8_parts.h"
#include "attn_smoothv_parts.h"

#include <math.h>

namespace {

constexpr int kMaxHeads = 32;      // C <= 4096, the fused producers' limit
constexpr int kMaxTileBlocks = 32;
constexpr int kMaxBatch = 65535;   // the element is a grid dimension

// ---- pass 1 over v: attn_v_stats_kernel / shard8s_v_stats_kernel with the element in blockIdx.z
__global__ __launch_bounds__(256) void shard8b_v_stats_kernel(const bf16* __restrict__ v, int64_t ldv, int64_t bs_v, float* __restrict__ rec,
                                                              int64_t bs_rec, int64_t N, int C) {
    const int64_t e = blockIdx.z;
    attn_v_stats_body(v + e * bs_v, ldv, rec + e * bs_rec, N, C);
}

// scratch of one element: rsum [VP][C] fp64, rlo [VP][C] fp32, rhi [VP][C] fp32; bs_scr in bytes
__global__ __launch_bounds__(256) void shard8sb_v_stats_kernel(const bf16* __restrict__ v, int64_t ldv, int64_t bs_v, uint8_t* __restrict__ scr,
                                                               int64_t bs_scr, int64_t VP, int64_t N, int C) {
    const int64_t e = blockIdx.z;
    double* rsum = reinterpret_cast<double*>(scr + e * bs_scr);
    float* rlo = reinterpret_cast<float*>(rsum + VP * C);
    attn_v_stats_smooth_body(v + e * bs_v, ldv, rsum, rlo, rlo + VP * C, N, C);
}

// ---- the record: shard8_record_kernel, workgroup (h, e)
__global__ __launch_bounds__(1024) void shard8b_record_kernel(const uint8_t* __restrict__ partials, int64_t bs_partials, int P,
                                                              const uint8_t* __restrict__ vscr, int64_t bs_vscr, int VP, int C,
                                                              uint8_t* __restrict__ records) {
    __shared__ double sum_s[8][kD];
    __shared__ float min_s[8][kD], max_s[8][kD], vmax_s[8][kD];
    const int h = blockIdx.x, tid = threadIdx.x, c = tid & (kD - 1), g = tid >> 7;
    const int64_t e = blockIdx.y;
    const double* psum = reinterpret_cast<const double*>(partials + e * bs_partials);
    const float* pmin = reinterpret_cast<const float*>(psum + (int64_t)P * C);
    const float* pmax = pmin + (int64_t)P * C;
    const float* vrec = reinterpret_cast<const float*>(vscr + e * bs_vscr);      // not read when VP == 0
    uint8_t* record = records + e * 20 * C;
    double s = 0.0;
    float lo = INFINITY, hi = -INFINITY, vm = 0.f;
    for (int p = g; p < P; p += 8) {
        const int64_t o = (int64_t)p * C + h * kD + c;
        s += psum[o];
        lo = fminf(lo, pmin[o]);
        hi = fmaxf(hi, pmax[o]);
    }
    for (int p = g; p < VP; p += 8) vm = fmaxf(vm, vrec[(int64_t)p * C + h * kD + c]);
    sum_s[g][c] = s;
    min_s[g][c] = lo;
    max_s[g][c] = hi;
    vmax_s[g][c] = vm;
    __syncthreads();
    if (tid >= kD) return;
#pragma unroll
    for (int i = 1; i < 8; ++i) {
        s += sum_s[i][c];
        lo = fminf(lo, min_s[i][c]);
        hi = fmaxf(hi, max_s[i][c]);
        vm = fmaxf(vm, vmax_s[i][c]);
    }
    const int ch = h * kD + c;
    reinterpret_cast<double*>(record)[ch] = s;
    reinterpret_cast<float*>(record + (int64_t)8 * C)[ch] = lo;
    reinterpret_cast<float*>(record + (int64_t)12 * C)[ch] = hi;
    reinterpret_cast<float*>(record + (int64_t)16 * C)[ch] = vm;
}

// join8 of attn_shard8s.hip, word for word
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

// shard8s_record_kernel, workgroup (h, e)
__global__ __launch_bounds__(1024) void shard8sb_record_kernel(const uint8_t* __restrict__ partials, int64_t bs_partials, int P,
                                                               const uint8_t* __restrict__ vscr, int64_t bs_vscr, int VP, int C,
                                                               uint8_t* __restrict__ records) {
    const int h = blockIdx.x, tid = threadIdx.x, c = tid & (kD - 1), g = tid >> 7, ch = h * kD + c;
    const int64_t e = blockIdx.y;
    const double* psum = reinterpret_cast<const double*>(partials + e * bs_partials);
    const float* pmin = reinterpret_cast<const float*>(psum + (int64_t)P * C);
    const double* vsum = reinterpret_cast<const double*>(vscr + e * bs_vscr);
    const float* vmin = reinterpret_cast<const float*>(vsum + (int64_t)VP * C);
    uint8_t* record = records + e * 32 * C;
    double s;
    float lo, hi;
    join8(psum, pmin, pmin + (int64_t)P * C, P, C, ch, c, g, s, lo, hi);
    if (g == 0) {
        reinterpret_cast<double*>(record)[ch] = s;
        reinterpret_cast<float*>(record + (int64_t)8 * C)[ch] = lo;
        reinterpret_cast<float*>(record + (int64_t)12 * C)[ch] = hi;
    }
    join8(vsum, vmin, vmin + (int64_t)VP * C, VP, C, ch, c, g, s, lo, hi);
    if (g == 0) {
        reinterpret_cast<double*>(record + (int64_t)16 * C)[ch] = s;
        reinterpret_cast<float*>(record + (int64_t)24 * C)[ch] = lo;
        reinterpret_cast<float*>(record + (int64_t)28 * C)[ch] = hi;
    }
}

// ---- the scales: shard8_finalise_kernel / shard8s_finalise_kernel, workgroup (h, e); record of rank w and element e at (w B + e)
template <bool SMOOTH>
__global__ __launch_bounds__(128) void shard8b_finalise_kernel(const uint8_t* __restrict__ records, int W, int B, int C, int64_t N,
                                                               float* __restrict__ kbar, float* __restrict__ sk, float* __restrict__ sv,
                                                               float* __restrict__ mu) {
    __shared__ float amax_s[2];
    const int h = blockIdx.x, tid = threadIdx.x, ch = h * kD + tid;
    const int64_t e = blockIdx.y, rb = SMOOTH ? 32 : 20;
    double s = 0.0, vs = 0.0;
    float lo = INFINITY, hi = -INFINITY, vm = 0.f, vlo = INFINITY, vhi = -INFINITY;
    for (int w = 0; w < W; ++w) {
        const uint8_t* r = records + ((int64_t)w * B + e) * rb * C;
        s += reinterpret_cast<const double*>(r)[ch];
        lo = fminf(lo, reinterpret_cast<const float*>(r + (int64_t)8 * C)[ch]);
        hi = fmaxf(hi, reinterpret_cast<const float*>(r + (int64_t)12 * C)[ch]);
        if (SMOOTH) {
            vs += reinterpret_cast<const double*>(r + (int64_t)16 * C)[ch];
            vlo = fminf(vlo, reinterpret_cast<const float*>(r + (int64_t)24 * C)[ch]);
            vhi = fmaxf(vhi, reinterpret_cast<const float*>(r + (int64_t)28 * C)[ch]);
        } else {
            vm = fmaxf(vm, reinterpret_cast<const float*>(r + (int64_t)16 * C)[ch]);
        }
    }
    const float m = (float)(s / (double)N);
    kbar[e * C + ch] = m;
    if (SMOOTH) {
        float vmean, vscale;
        smoothv_scale(vs, vlo, vhi, N, vmean, vscale);
        mu[e * C + ch] = vmean;
        sv[e * C + ch] = vscale;
    } else if (sv) {
        sv[e * C + ch] = fmaxf(vm / kE4M3Max, kScaleFloor);
    }
    const float amax = wave_max(fmaxf(hi - m, m - lo));
    if ((tid & 63) == 0) amax_s[tid >> 6] = amax;
    __syncthreads();
    if (tid == 0) sk[e * (C / kD) + h] = fmaxf(fmaxf(amax_s[0], amax_s[1]) / kE4M3Max, kScaleFloor);
}

// ---- the rows: shard8_quant_kernel<HAS_V> (MODE 0, 1) / shard8s_quant_kernel (MODE 2), workgroup (row block, h, e)
template <int MODE>
__global__ __launch_bounds__(256) void shard8b_quant_kernel(const bf16* __restrict__ k, int64_t ldk, int64_t bs_k, const bf16* __restrict__ v,
                                                            int64_t ldv, int64_t bs_v, const float* __restrict__ kbar,
                                                            const float* __restrict__ sk, const float* __restrict__ sv,
                                                            const float* __restrict__ mu, uint8_t* __restrict__ k8, uint8_t* __restrict__ v8,
                                                            int64_t rows, int H) {
    const int h = blockIdx.y, tid = threadIdx.x, c = tid & 15;
    const int64_t e = blockIdx.z, C = (int64_t)H * kD;
    const int64_t row = (int64_t)blockIdx.x * 16 + (tid >> 4);
    if (row >= rows) return;
    const int ch = h * kD + c * 8;
    kbar += e * C;
    const bf16x8 kv = *reinterpret_cast<const bf16x8*>(k + e * bs_k + row * ldk + ch);
    const f32x4 m0 = *reinterpret_cast<const f32x4*>(kbar + ch), m1 = *reinterpret_cast<const f32x4*>(kbar + ch + 4);
    const float s_k = sk[e * H + h];
    float kf[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) kf[j] = (float)kv[j] - (j < 4 ? m0[j & 3] : m1[j & 3]);
    const int64_t o = ((e * rows + row) * H + h) * kD + c * 8;
    *reinterpret_cast<u32x2*>(k8 + o) = quant8_e4m3(kf, s_k);
    if (MODE == 0) return;
    sv += e * C;
    const bf16x8 vv = *reinterpret_cast<const bf16x8*>(v + e * bs_v + row * ldv + ch);
    const f32x4 s0 = *reinterpret_cast<const f32x4*>(sv + ch), s1 = *reinterpret_cast<const f32x4*>(sv + ch + 4);
    float f[8];
    if (MODE == 2) {
        mu += e * C;
        const f32x4 u0 = *reinterpret_cast<const f32x4*>(mu + ch), u1 = *reinterpret_cast<const f32x4*>(mu + ch + 4);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float d = (float)vv[j] - (j < 4 ? u0[j & 3] : u1[j & 3]);
            f[j] = d / (j < 4 ? s0[j & 3] : s1[j & 3]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = (float)vv[j] / (j < 4 ? s0[j & 3] : s1[j & 3]);
    }
    u32x2 w;
    w[0] = cvt2_e4m3(f[0], f[1]) | (cvt2_e4m3(f[2], f[3]) << 16);
    w[1] = cvt2_e4m3(f[4], f[5]) | (cvt2_e4m3(f[6], f[7]) << 16);
    *reinterpret_cast<u32x2*>(v8 + o) = w;
}

// ---- the tiles: shard8_vt_kernel, workgroup (x, h, e); element e's rows start bs_v8 bytes behind element e - 1's
__global__ __launch_bounds__(256) void shard8b_vt_kernel(const uint8_t* __restrict__ v8, int64_t bs_v8, uint8_t* __restrict__ v8t, int64_t N,
                                                         int64_t Nkp, int H) {
    __shared__ __attribute__((aligned(16))) uint32_t img[kD][16];
    const int h = blockIdx.y, tid = threadIdx.x, cl = tid & 15, kg = tid >> 4;
    const int64_t C = (int64_t)H * kD, e = blockIdx.z;
    v8 += e * bs_v8;
    v8t += e * C * Nkp;
    const int wr = pv8_dword(kg) ^ cl;
    const int64_t nt = Nkp / kTileKeys;
    for (int64_t t = blockIdx.x; t < nt; t += gridDim.x) {
        u32x2 x[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t key = t * kTileKeys + 4 * kg + i;
            x[i] = u32x2{0u, 0u};      // the padding keys of the last tile: zero bytes
            if (key < N) x[i] = *reinterpret_cast<const u32x2*>(v8 + key * C + h * kD + cl * 8);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int sh = 8 * (j & 3);
            img[cl * 8 + j][wr] = ((x[0][j >> 2] >> sh) & 0xffu) | (((x[1][j >> 2] >> sh) & 0xffu) << 8) |
                                  (((x[2][j >> 2] >> sh) & 0xffu) << 16) | (((x[3][j >> 2] >> sh) & 0xffu) << 24);
        }
        __syncthreads();
        pv8_store_tile(img, v8t, h, Nkp, t, tid);
        __syncthreads();
    }
}

// The checks the two stats entry points share; returns the key-partials bytes of one element, or sets the error and returns -1 (FG_EINVAL).
int64_t stats_checks(const char* who, const void* partials, int64_t partials_bytes, int64_t bs_partials, const void* v, int64_t ldv, int64_t bs_v,
                     const void* record, int64_t record_bytes, int record_unit, const void* scratch, int B, int64_t rows, int H, int D) {
    FG_CHECK_ARG(partials && record, "%s: null pointer", who);
    FG_CHECK_ARG(D == kD, "%s: only head_dim 128 is supported (got %d)", who, D);
    FG_CHECK_ARG(B >= 1 && B <= kMaxBatch, "%s: B in 1..%d (got %d)", who, kMaxBatch, B);
    FG_CHECK_ARG(rows > 0 && H > 0 && H <= kMaxHeads, "%s: rows must be positive, H in 1..%d", who, kMaxHeads);
    const int C = H * kD;
    const int64_t need = fg_attn_qk8_fused_scratch_bytes(rows, C);      // P records of 16 C bytes: the layout of the key producer
    FG_CHECK_ARG(need > 0 && partials_bytes >= need, "%s: partials must hold %lld bytes per element (got %lld)", who, (long long)need,
                       (long long)partials_bytes);
    FG_CHECK_ARG(bs_partials >= need && bs_partials % 16 == 0, "%s: the element stride of partials must be >= %lld and a multiple of 16", who,
                       (long long)need);
    FG_CHECK_ARG(record_bytes >= (int64_t)B * record_unit * C, "%s: the records must hold B * %d * C = %lld bytes (got %lld)", who, record_unit,
                       (long long)B * record_unit * C, (long long)record_bytes);
    FG_CHECK_ARG(FG_ALIGNED16(partials) && FG_ALIGNED16(record) && FG_ALIGNED16(v) && FG_ALIGNED16(scratch),
                       "%s: partials, v, record and scratch must be 16-byte aligned", who);
    if (v) {
        FG_CHECK_ARG(ldv >= C && ldv % 8 == 0, "%s: ldv must be >= H*D and a multiple of 8", who);
        FG_CHECK_ARG(bs_v >= (rows - 1) * ldv + C && bs_v % 8 == 0, "%s: the element stride of v must cover its rows and be a multiple of 8", who);
    }
    return need;
}

// mode 0: shard8 without v, 1: shard8 with v, 2: shard8s
int quant_launch(const char* who, int mode, const void* records, int64_t records_bytes, int W, int64_t N, const void* k, int64_t ldk, int64_t bs_k,
                 const void* v, int64_t ldv, int64_t bs_v, void* k8, void* v8, float* sk, float* kbar, float* sv, float* mu, int B, int64_t rows,
                 int H, int D, fg_stream_t stream) {
    const int unit = mode == 2 ? 32 : 20;
    FG_CHECK_ARG(records && k && k8 && sk && kbar, "%s: null pointer", who);
    FG_CHECK_ARG(mode == 0 || (v && v8 && sv), "%s: v needs v8 and sv", who);
    FG_CHECK_ARG(mode != 2 || mu, "%s: null pointer", who);
    FG_CHECK_ARG(D == kD, "%s: only head_dim 128 is supported (got %d)", who, D);
    FG_CHECK_ARG(B >= 1 && B <= kMaxBatch, "%s: B in 1..%d (got %d)", who, kMaxBatch, B);
    FG_CHECK_ARG(H > 0 && H <= kMaxHeads, "%s: H in 1..%d", who, kMaxHeads);
    FG_CHECK_ARG(W >= 1 && N >= 1, "%s: W and N must be positive (got W=%d N=%lld)", who, W, (long long)N);
    FG_CHECK_ARG(rows >= 1 && rows <= N, "%s: 1 <= rows <= N (got rows=%lld N=%lld)", who, (long long)rows, (long long)N);
    const int C = H * kD;
    FG_CHECK_ARG(records_bytes >= (int64_t)W * B * unit * C, "%s: records must hold W * B * %d * C = %lld bytes (got %lld)", who, unit,
                       (long long)W * B * unit * C, (long long)records_bytes);
    FG_CHECK_ARG(ldk >= C && ldk % 8 == 0 && (mode == 0 || (ldv >= C && ldv % 8 == 0)),
                       "%s: leading dimensions must be >= H*D and multiples of 8", who);
    FG_CHECK_ARG(bs_k >= (rows - 1) * ldk + C && bs_k % 8 == 0 && (mode == 0 || (bs_v >= (rows - 1) * ldv + C && bs_v % 8 == 0)),
                       "%s: element strides must cover the element's rows and be multiples of 8", who);
    FG_CHECK_ARG(FG_ALIGNED16(records) && FG_ALIGNED16(k) && FG_ALIGNED16(v) && FG_ALIGNED16(kbar) && FG_ALIGNED16(sv) && FG_ALIGNED16(mu) &&
                           (((uintptr_t)k8 | (uintptr_t)v8) & 7) == 0 && (((uintptr_t)sk) & 3) == 0,
                       "%s: records, k, v, kbar, sv, mu must be 16-byte aligned (k8, v8: 8; sk: 4)", who);
    FG_CHECK_ARG((rows + 15) / 16 < (1ll << 31), "%s: grid too large", who);
    const dim3 heads((unsigned)H, (unsigned)B);
    if (mode == 2)
        hipLaunchKernelGGL(shard8b_finalise_kernel<true>, heads, dim3(128), 0, (hipStream_t)stream, (const uint8_t*)records, W, B, C, N, kbar, sk, sv,
                           mu);
    else
        hipLaunchKernelGGL(shard8b_finalise_kernel<false>, heads, dim3(128), 0, (hipStream_t)stream, (const uint8_t*)records, W, B, C, N, kbar, sk,
                           mode == 1 ? sv : nullptr, (float*)nullptr);
    if (int e = fg_launch_status(who)) return e;
    const dim3 grid((unsigned)((rows + 15) / 16), (unsigned)H, (unsigned)B);
#define FG_SHARD8B_QUANT(M)                                                                                                                 \
    hipLaunchKernelGGL(shard8b_quant_kernel<M>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)k, ldk, bs_k, (const bf16*)(M ? v : nullptr), \
                       M ? ldv : (int64_t)0, M ? bs_v : (int64_t)0, (const float*)kbar, (const float*)sk, (const float*)(M ? sv : nullptr),    \
                       (const float*)(M == 2 ? mu : nullptr), (uint8_t*)k8, (uint8_t*)(M ? v8 : nullptr), rows, H)
    if (mode == 2)
        FG_SHARD8B_QUANT(2);
    else if (mode == 1)
        FG_SHARD8B_QUANT(1);
    else
        FG_SHARD8B_QUANT(0);
#undef FG_SHARD8B_QUANT
    return fg_launch_status(who);
}

}  // namespace

extern "C" int fg_attn_shard8b_version(void) { return 1; }

extern "C" int fg_attn_shard8_stats_b(const void* partials, int64_t partials_bytes, int64_t bs_partials, const void* v, int64_t ldv, int64_t bs_v,
                                      void* records, int64_t records_bytes, void* scratch, int64_t scratch_bytes, int64_t bs_scratch, int B,
                                      int64_t rows, int H, int D, fg_stream_t stream) {
    const char* who = "fg_attn_shard8_stats_b";
    const int64_t need = stats_checks(who, partials, partials_bytes, bs_partials, v, ldv, bs_v, records, records_bytes, 20, scratch, B, rows, H, D);
    if (need < 0) return FG_EINVAL;
    const int C = H * kD;
    const int64_t P = need / ((int64_t)16 * C), VP = v ? v_stat_parts(rows) : 0;
    if (v) {
        FG_CHECK_ARG(scratch && scratch_bytes >= VP * C * 4 && bs_scratch >= VP * C * 4 && bs_scratch % 16 == 0,
                     "fg_attn_shard8_stats_b: scratch must hold %lld bytes per element, element stride a multiple of 16 (got %lld, stride %lld)",
                     (long long)(VP * C * 4), (long long)scratch_bytes, (long long)bs_scratch);
        hipLaunchKernelGGL(shard8b_v_stats_kernel, dim3((unsigned)VP, (unsigned)((C / 8 + 63) / 64), (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                           (const bf16*)v, ldv, bs_v, (float*)scratch, bs_scratch / 4, rows, C);
        if (int e = fg_launch_status("fg_attn_shard8_stats_b (v statistics)")) return e;
    }
    hipLaunchKernelGGL(shard8b_record_kernel, dim3((unsigned)H, (unsigned)B), dim3(1024), 0, (hipStream_t)stream, (const uint8_t*)partials,
                       bs_partials, (int)P, (const uint8_t*)scratch, v ? bs_scratch : (int64_t)0, (int)VP, C, (uint8_t*)records);
    return fg_launch_status(who);
}

extern "C" int fg_attn_shard8_quant_b(const void* records, int64_t records_bytes, int W, int64_t N, const void* k, int64_t ldk, int64_t bs_k,
                                      const void* v, int64_t ldv, int64_t bs_v, void* k8, void* v8, float* sk, float* kbar, float* sv, int B,
                                      int64_t rows, int H, int D, fg_stream_t stream) {
    return quant_launch("fg_attn_shard8_quant_b", v ? 1 : 0, records, records_bytes, W, N, k, ldk, bs_k, v, ldv, bs_v, k8, v8, sk, kbar, sv, nullptr,
                        B, rows, H, D, stream);
}

extern "C" int fg_attn_shard8_vt_b(const void* v8, int64_t bs_v8, void* v8t, int B, int64_t N, int H, int D, fg_stream_t stream) {
    FG_CHECK_ARG(v8 && v8t, "fg_attn_shard8_vt_b: null pointer");
    FG_CHECK_ARG(D == kD, "fg_attn_shard8_vt_b: only head_dim 128 is supported (got %d)", D);
    FG_CHECK_ARG(B >= 1 && B <= kMaxBatch, "fg_attn_shard8_vt_b: B in 1..%d (got %d)", kMaxBatch, B);
    FG_CHECK_ARG(N > 0 && H > 0 && H <= kMaxHeads, "fg_attn_shard8_vt_b: N must be positive, H in 1..%d", kMaxHeads);
    FG_CHECK_ARG(bs_v8 >= N * H * kD && bs_v8 % 16 == 0,
                 "fg_attn_shard8_vt_b: the element stride of v8 must be >= N*H*D bytes and a multiple of 16 (got %lld)", (long long)bs_v8);
    FG_CHECK_ARG(FG_ALIGNED16(v8) && FG_ALIGNED16(v8t), "fg_attn_shard8_vt_b: v8 and v8t must be 16-byte aligned");
    const int64_t nkp = (N + kTileKeys - 1) / kTileKeys * kTileKeys, nt = nkp / kTileKeys;
    hipLaunchKernelGGL(shard8b_vt_kernel, dim3((unsigned)(nt < kMaxTileBlocks ? nt : kMaxTileBlocks), (unsigned)H, (unsigned)B), dim3(256), 0,
                       (hipStream_t)stream, (const uint8_t*)v8, bs_v8, (uint8_t*)v8t, N, nkp, H);
    return fg_launch_status("fg_attn_shard8_vt_b");
}

extern "C" int fg_attn_shard8s_stats_b(const void* partials, int64_t partials_bytes, int64_t bs_partials, const void* v, int64_t ldv, int64_t bs_v,
                                       void* records, int64_t records_bytes, void* scratch, int64_t scratch_bytes, int64_t bs_scratch, int B,
                                       int64_t rows, int H, int D, fg_stream_t stream) {
    const char* who = "fg_attn_shard8s_stats_b";
    FG_CHECK_ARG(v && scratch, "fg_attn_shard8s_stats_b: null pointer");
    const int64_t need = stats_checks(who, partials, partials_bytes, bs_partials, v, ldv, bs_v, records, records_bytes, 32, scratch, B, rows, H, D);
    if (need < 0) return FG_EINVAL;
    const int C = H * kD;
    const int64_t P = need / ((int64_t)16 * C), VP = v_stat_parts(rows);
    FG_CHECK_ARG(scratch_bytes >= VP * C * 16 && bs_scratch >= VP * C * 16 && bs_scratch % 16 == 0,
                 "fg_attn_shard8s_stats_b: scratch must hold %lld bytes per element, element stride a multiple of 16 (got %lld, stride %lld)",
                 (long long)(VP * C * 16), (long long)scratch_bytes, (long long)bs_scratch);
    hipLaunchKernelGGL(shard8sb_v_stats_kernel, dim3((unsigned)VP, (unsigned)((C / 8 + 63) / 64), (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                       (const bf16*)v, ldv, bs_v, (uint8_t*)scratch, bs_scratch, VP, rows, C);
    if (int e = fg_launch_status("fg_attn_shard8s_stats_b (v statistics)")) return e;
    hipLaunchKernelGGL(shard8sb_record_kernel, dim3((unsigned)H, (unsigned)B), dim3(1024), 0, (hipStream_t)stream, (const uint8_t*)partials,
                       bs_partials, (int)P, (const uint8_t*)scratch, bs_scratch, (int)VP, C, (uint8_t*)records);
    return fg_launch_status(who);
}

extern "C" int fg_attn_shard8s_quant_b(const void* records, int64_t records_bytes, int W, int64_t N, const void* k, int64_t ldk, int64_t bs_k,
                                       const void* v, int64_t ldv, int64_t bs_v, void* k8, void* v8, float* sk, float* kbar, float* sv, float* mu,
                                       int B, int64_t rows, int H, int D, fg_stream_t stream) {
    FG_CHECK_ARG(v && v8 && sv && mu, "fg_attn_shard8s_quant_b: null pointer");
    return quant_launch("fg_attn_shard8s_quant_b", 2, records, records_bytes, W, N, k, ldk, bs_k, v, ldv, bs_v, k8, v8, sk, kbar, sv, mu, B, rows, H, D,
                        stream);
}
