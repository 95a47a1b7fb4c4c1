// The e4m3 operands of the 8-bit self-attention on a token shard (include/fairygen_hip_shard8.h), for gfx950.
//
// The N keys are sharded by rows over W ranks; the key mean, sk and sv are statistics over all of them.  Per rank and block:
//   1. fg_attn_shard8_stats: the rank's partial key records (fg_rmsnorm_rope_kstats_bf16) and a walk over its v rows -> ONE record:
//      per channel the fp64 key sum, the key minimum and maximum, the maximum of |v|;
//   2. the W records are all-gathered by the host (W * 20 * C bytes);
//   3. fg_attn_shard8_quant: every rank reduces the W records in the same order with the expressions of attn_k_finalise_kernel
//      (attn_qk8_fused.hip) and attn_quant_vt_kernel (attn_pv8.hip), then converts its rows: k8 as attn_quant_k_kernel, v8 row-major;
//   4. the host all-gathers k8 and v8 (the e4m3 bytes: half of the bf16 ones);
//   5. fg_attn_shard8_vt: the gathered v8 (N, C) -> v8t (H, 128, Nkp) in the tile order of the attention kernel's P fragment.
// An exact fp64 sum, a minimum and a maximum do not depend on the order, so the bytes are those of the unsharded producers.
// The row walks are HBM-bound; no atomics, nothing waits on another workgroup.
#include "common.h"
#include "../../include/fairygen_hip_shard8.h"
#include "attn_qk8_quant.h"
#include "attn_pv8_parts.h"

#include <math.h>

namespace {

constexpr int kMaxHeads = 32;      // C <= 4096, the fused producers' limit
constexpr int kMaxTileBlocks = 32;

// One workgroup of 1024 per head: thread t reduces channel t & 127 over the key records (t >> 7) + 8 i and the |v| records likewise, LDS
// joins the 8 groups, the first 128 threads write the head's slice of the record.
__global__ __launch_bounds__(1024) void shard8_record_kernel(const double* __restrict__ psum, const float* __restrict__ pmin,
                                                             const float* __restrict__ pmax, int P, const float* __restrict__ vrec, int VP,
                                                             int C, double* __restrict__ rsum, float* __restrict__ rmin,
                                                             float* __restrict__ rmax, float* __restrict__ rvmax) {
    __shared__ double sum_s[8][kD];
    __shared__ float min_s[8][kD], max_s[8][kD], vmax_s[8][kD];
    const int h = blockIdx.x, tid = threadIdx.x, c = tid & (kD - 1), g = tid >> 7;
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
    rsum[h * kD + c] = s;
    rmin[h * kD + c] = lo;
    rmax[h * kD + c] = hi;
    rvmax[h * kD + c] = vm;
}

// One workgroup of 128 per head: thread c walks the W records in rank order; the expressions of attn_k_finalise_kernel and of
// attn_quant_vt_kernel.
__global__ __launch_bounds__(128) void shard8_finalise_kernel(const uint8_t* __restrict__ records, int W, int C, int64_t N,
                                                              float* __restrict__ kbar, float* __restrict__ sk, float* __restrict__ sv) {
    __shared__ float amax_s[2];
    const int h = blockIdx.x, tid = threadIdx.x, ch = h * kD + tid;
    double s = 0.0;
    float lo = INFINITY, hi = -INFINITY, vm = 0.f;
    for (int w = 0; w < W; ++w) {
        const uint8_t* r = records + (int64_t)w * 20 * C;
        s += reinterpret_cast<const double*>(r)[ch];
        lo = fminf(lo, reinterpret_cast<const float*>(r + (int64_t)8 * C)[ch]);
        hi = fmaxf(hi, reinterpret_cast<const float*>(r + (int64_t)12 * C)[ch]);
        vm = fmaxf(vm, reinterpret_cast<const float*>(r + (int64_t)16 * C)[ch]);
    }
    const float m = (float)(s / (double)N);
    kbar[ch] = m;
    if (sv) sv[ch] = fmaxf(vm / kE4M3Max, kScaleFloor);
    const float amax = wave_max(fmaxf(hi - m, m - lo));
    if ((tid & 63) == 0) amax_s[tid >> 6] = amax;
    __syncthreads();
    if (tid == 0) sk[h] = fmaxf(fmaxf(amax_s[0], amax_s[1]) / kE4M3Max, kScaleFloor);
}

// attn_quant_k_kernel with v beside it: 16 rows of one head per workgroup of 256, 16 lanes x 8 channels cover a row.
template <bool HAS_V>
__global__ __launch_bounds__(256) void shard8_quant_kernel(const bf16* __restrict__ k, int64_t ldk, const bf16* __restrict__ v, int64_t ldv,
                                                           const float* __restrict__ kbar, const float* __restrict__ sk,
                                                           const float* __restrict__ sv, uint8_t* __restrict__ k8, uint8_t* __restrict__ v8,
                                                           int64_t rows, int H) {
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
    if (HAS_V) {
        const bf16x8 vv = *reinterpret_cast<const bf16x8*>(v + row * ldv + ch);
        const f32x4 s0 = *reinterpret_cast<const f32x4*>(sv + ch), s1 = *reinterpret_cast<const f32x4*>(sv + ch + 4);
        float f[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = (float)vv[j] / (j < 4 ? s0[j & 3] : s1[j & 3]);
        u32x2 w;
        w[0] = cvt2_e4m3(f[0], f[1]) | (cvt2_e4m3(f[2], f[3]) << 16);
        w[1] = cvt2_e4m3(f[4], f[5]) | (cvt2_e4m3(f[6], f[7]) << 16);
        *reinterpret_cast<u32x2*>(v8 + o) = w;
    }
}

// Workgroup (x, h) of 256 walks the tiles x, x + gridDim.x, .. of head h.  Thread t holds the 8 channels of chunk cl = t & 15 of the 4 keys
// 4 kg .. 4 kg + 3, kg = t >> 4: 8 bytes a key; the bytes of one channel's 4 keys make the dword attn_quant_vt_kernel writes to the image.
__global__ __launch_bounds__(256) void shard8_vt_kernel(const uint8_t* __restrict__ v8, uint8_t* __restrict__ v8t, int64_t N, int64_t Nkp,
                                                        int H) {
    __shared__ __attribute__((aligned(16))) uint32_t img[kD][16];
    const int h = blockIdx.y, tid = threadIdx.x, cl = tid & 15, kg = tid >> 4;
    const int64_t C = (int64_t)H * kD;
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

bool channels_ok(int C) { return C >= kD && C % kD == 0 && C <= kMaxHeads * kD; }

}  // namespace

extern "C" int fg_attn_shard8_version(void) { return 1; }

extern "C" int64_t fg_attn_shard8_record_bytes(int C) {
    if (!channels_ok(C)) {
        fg_set_error("fg_attn_shard8_record_bytes: C must be a multiple of 128 up to %d (got %d)", kMaxHeads * kD, C);
        return -1;
    }
    return (int64_t)20 * C;
}

extern "C" int64_t fg_attn_shard8_scratch_bytes(int64_t rows, int C) {
    if (rows < 1 || !channels_ok(C)) {
        fg_set_error("fg_attn_shard8_scratch_bytes: rows must be positive, C a multiple of 128 up to %d (got rows=%lld C=%d)", kMaxHeads * kD,
                     (long long)rows, C);
        return -1;
    }
    return v_stat_parts(rows) * C * 4;
}

extern "C" int fg_attn_shard8_stats(const void* partials, int64_t partials_bytes, const void* v, int64_t ldv, void* record,
                                    int64_t record_bytes, void* scratch, int64_t scratch_bytes, int64_t rows, int H, int D,
                                    fg_stream_t stream) {
    FG_CHECK_ARG(partials && record, "fg_attn_shard8_stats: null pointer");
    FG_CHECK_ARG(D == kD, "fg_attn_shard8_stats: only head_dim 128 is supported (got %d)", D);
    FG_CHECK_ARG(rows > 0 && H > 0 && H <= kMaxHeads, "fg_attn_shard8_stats: rows must be positive, H in 1..%d", kMaxHeads);
    const int C = H * kD;
    const int64_t need = fg_attn_qk8_fused_scratch_bytes(rows, C);      // P records of 16 C bytes: the layout of the key producer
    FG_CHECK_ARG(need > 0 && partials_bytes >= need, "fg_attn_shard8_stats: partials must hold %lld bytes (got %lld)", (long long)need,
                 (long long)partials_bytes);
    FG_CHECK_ARG(record_bytes >= (int64_t)20 * C, "fg_attn_shard8_stats: the record must hold %lld bytes (got %lld)", (long long)20 * C,
                 (long long)record_bytes);
    FG_CHECK_ARG(FG_ALIGNED16(partials) && FG_ALIGNED16(record) && FG_ALIGNED16(v) && FG_ALIGNED16(scratch),
                 "fg_attn_shard8_stats: partials, v, record and scratch must be 16-byte aligned");
    const int64_t P = need / ((int64_t)16 * C), VP = v ? v_stat_parts(rows) : 0;
    if (v) {
        FG_CHECK_ARG(ldv >= C && ldv % 8 == 0, "fg_attn_shard8_stats: ldv must be >= H*D and a multiple of 8");
        FG_CHECK_ARG(scratch && scratch_bytes >= VP * C * 4, "fg_attn_shard8_stats: scratch must hold %lld bytes (got %lld)",
                     (long long)(VP * C * 4), (long long)scratch_bytes);
        hipLaunchKernelGGL(attn_v_stats_kernel, dim3((unsigned)VP, (unsigned)((C / 8 + 63) / 64)), dim3(256), 0, (hipStream_t)stream,
                           (const bf16*)v, ldv, (float*)scratch, rows, C);
        if (int e = fg_launch_status("fg_attn_shard8_stats (v statistics)")) return e;
    }
    const double* psum = (const double*)partials;
    const float* pmin = (const float*)(psum + P * C);
    const float* pmax = pmin + P * C;
    double* rsum = (double*)record;
    float* rmin = (float*)(rsum + C);
    hipLaunchKernelGGL(shard8_record_kernel, dim3((unsigned)H), dim3(1024), 0, (hipStream_t)stream, psum, pmin, pmax, (int)P,
                       (const float*)scratch, (int)VP, C, rsum, rmin, rmin + C, rmin + 2 * C);
    return fg_launch_status("fg_attn_shard8_stats");
}

extern "C" int fg_attn_shard8_quant(const void* records, int64_t records_bytes, int W, int64_t N, const void* k, int64_t ldk, const void* v,
                                    int64_t ldv, void* k8, void* v8, float* sk, float* kbar, float* sv, int64_t rows, int H, int D,
                                    fg_stream_t stream) {
    FG_CHECK_ARG(records && k && k8 && sk && kbar, "fg_attn_shard8_quant: null pointer");
    FG_CHECK_ARG(!v || (v8 && sv), "fg_attn_shard8_quant: v needs v8 and sv");
    FG_CHECK_ARG(D == kD, "fg_attn_shard8_quant: only head_dim 128 is supported (got %d)", D);
    FG_CHECK_ARG(H > 0 && H <= kMaxHeads, "fg_attn_shard8_quant: H in 1..%d", kMaxHeads);
    FG_CHECK_ARG(W >= 1 && N >= 1, "fg_attn_shard8_quant: W and N must be positive (got W=%d N=%lld)", W, (long long)N);
    FG_CHECK_ARG(rows >= 1 && rows <= N, "fg_attn_shard8_quant: 1 <= rows <= N (got rows=%lld N=%lld)", (long long)rows, (long long)N);
    const int C = H * kD;
    FG_CHECK_ARG(records_bytes >= (int64_t)W * 20 * C, "fg_attn_shard8_quant: records must hold W * 20 * C = %lld bytes (got %lld)",
                 (long long)W * 20 * C, (long long)records_bytes);
    FG_CHECK_ARG(ldk >= C && ldk % 8 == 0 && (!v || (ldv >= C && ldv % 8 == 0)),
                 "fg_attn_shard8_quant: leading dimensions must be >= H*D and multiples of 8");
    FG_CHECK_ARG(FG_ALIGNED16(records) && FG_ALIGNED16(k) && FG_ALIGNED16(v) && FG_ALIGNED16(kbar) && FG_ALIGNED16(sv) &&
                     (((uintptr_t)k8 | (uintptr_t)v8) & 7) == 0 && (((uintptr_t)sk) & 3) == 0,
                 "fg_attn_shard8_quant: records, k, v, kbar, sv must be 16-byte aligned (k8, v8: 8; sk: 4)");
    FG_CHECK_ARG((rows + 15) / 16 < (1ll << 31), "fg_attn_shard8_quant: grid too large");
    hipLaunchKernelGGL(shard8_finalise_kernel, dim3((unsigned)H), dim3(128), 0, (hipStream_t)stream, (const uint8_t*)records, W, C, N, kbar, sk,
                       v ? sv : nullptr);
    if (int e = fg_launch_status("fg_attn_shard8_quant (scales)")) return e;
    const dim3 grid((unsigned)((rows + 15) / 16), (unsigned)H);
    if (v)
        hipLaunchKernelGGL(shard8_quant_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)k, ldk, (const bf16*)v, ldv,
                           (const float*)kbar, (const float*)sk, (const float*)sv, (uint8_t*)k8, (uint8_t*)v8, rows, H);
    else
        hipLaunchKernelGGL(shard8_quant_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)k, ldk, (const bf16*)nullptr,
                           (int64_t)0, (const float*)kbar, (const float*)sk, (const float*)nullptr, (uint8_t*)k8, (uint8_t*)nullptr, rows, H);
    return fg_launch_status("fg_attn_shard8_quant");
}

extern "C" int fg_attn_shard8_vt(const void* v8, void* v8t, int64_t N, int H, int D, fg_stream_t stream) {
    FG_CHECK_ARG(v8 && v8t, "fg_attn_shard8_vt: null pointer");
    FG_CHECK_ARG(D == kD, "fg_attn_shard8_vt: only head_dim 128 is supported (got %d)", D);
    FG_CHECK_ARG(N > 0 && H > 0 && H <= kMaxHeads, "fg_attn_shard8_vt: N must be positive, H in 1..%d", kMaxHeads);
    FG_CHECK_ARG(FG_ALIGNED16(v8) && FG_ALIGNED16(v8t), "fg_attn_shard8_vt: v8 and v8t must be 16-byte aligned");
    const int64_t nkp = (N + kTileKeys - 1) / kTileKeys * kTileKeys, nt = nkp / kTileKeys;
    hipLaunchKernelGGL(shard8_vt_kernel, dim3((unsigned)(nt < kMaxTileBlocks ? nt : kMaxTileBlocks), (unsigned)H), dim3(256), 0,
                       (hipStream_t)stream, (const uint8_t*)v8, (uint8_t*)v8t, N, nkp, H);
    return fg_launch_status("fg_attn_shard8_vt");
}
