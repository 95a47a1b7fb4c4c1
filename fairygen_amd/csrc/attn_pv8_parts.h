// What the e4m3 V producer (attn_pv8.hip) and the producers of a token shard (attn_shard8.hip) share, so that both write the same bytes:
// the per-channel maximum of |v| over a row walk (up to 256 row strides leave one fp32 record each; a maximum does not depend on the
// order, so whoever reduces the records gets the exact value), and the tile order of v8t with the read-out of a tile's LDS image.
#pragma once
#include "common.h"
#include "attn_qk8_quant.h"

namespace {

constexpr int kMaxVParts = 256;
constexpr int kTileKeys = 64;

// records per channel: a function of the row count alone, 16 rows a workgroup until one workgroup per CU is reached
inline int64_t v_stat_parts(int64_t n) {
    const int64_t p = (n + 15) / 16;
    return p > kMaxVParts ? kMaxVParts : p;
}

// Workgroup (x, y) of 4 waves: lane l owns the 8 channels of 16-byte chunk 64 y + l; wave w walks the rows 4 x + w + 4 gridDim.x i.
__device__ __forceinline__ void attn_v_stats_body(const bf16* __restrict__ v, int64_t ldv, float* __restrict__ rec, int64_t N, int C) {
    __shared__ float amax_s[3][8][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunk = blockIdx.y * 64 + lane;
    const bool live = chunk * 8 < C;
    float amax[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) amax[j] = 0.f;
    if (live) {
        for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < N; row += (int64_t)gridDim.x * 4) {
            const bf16x8 x = *reinterpret_cast<const bf16x8*>(v + row * ldv + (int64_t)chunk * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) amax[j] = fmaxf(amax[j], fabsf((float)x[j]));
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) amax_s[wave - 1][j][lane] = amax[j];
    }
    __syncthreads();
    if (wave > 0 || !live) return;
    f32x4 lo, hi;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float a = fmaxf(fmaxf(amax[j], amax_s[0][j][lane]), fmaxf(amax_s[1][j][lane], amax_s[2][j][lane]));
        if (j < 4) lo[j] = a; else hi[j - 4] = a;
    }
    float* o = rec + (int64_t)blockIdx.x * C + (int64_t)chunk * 8;
    *reinterpret_cast<f32x4*>(o) = lo;
    *reinterpret_cast<f32x4*>(o + 4) = hi;
}

__global__ __launch_bounds__(256) void attn_v_stats_kernel(const bf16* __restrict__ v, int64_t ldv, float* __restrict__ rec, int64_t N, int C) {
    attn_v_stats_body(v, ldv, rec, N, C);
}

// Dword (4 keys) d of a tile's 16 holds the keys 4 kg .. 4 kg + 3 with d = kPv8Dword(kg): MFMA k index 32 hh + 16 sub + j stands for key
// 32 sub + 8 (j >> 2) + 4 hh + (j & 3), so keys 4 kg + (0..3) (sub = kg >> 3, j >> 2 = (kg >> 1) & 3, hh = kg & 1) are bytes 4 d + (0..3)
__device__ __forceinline__ int pv8_dword(int kg) { return 8 * (kg & 1) + 4 * (kg >> 3) + ((kg >> 1) & 3); }

// A workgroup of 256 writes tile t of head h from its LDS image: row ch of the image is channel ch, written by the thread of chunk
// cl = ch >> 3 at dword pv8_dword(kg) ^ cl; 16-byte reads of the image, 16-byte writes of v8t (H, 128, Nkp).
__device__ __forceinline__ void pv8_store_tile(const uint32_t (*img)[16], uint8_t* __restrict__ v8t, int h, int64_t Nkp, int64_t t, int tid) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = tid + 256 * i, ch = idx >> 2, q = idx & 3, x = ch >> 3;      // x: the chunk cl that wrote row ch
        const u32x4 rd = *reinterpret_cast<const u32x4*>(&img[ch][4 * (q ^ (x >> 2))]);
        u32x4 w;      // logical dword d of the chunk sits at d ^ (x & 3)
        w[0] = (x & 1) ? rd[1] : rd[0];
        w[1] = (x & 1) ? rd[0] : rd[1];
        w[2] = (x & 1) ? rd[3] : rd[2];
        w[3] = (x & 1) ? rd[2] : rd[3];
        if (x & 2) {
            const uint32_t a = w[0], b = w[1];
            w[0] = w[2]; w[1] = w[3]; w[2] = a; w[3] = b;
        }
        *reinterpret_cast<u32x4*>(v8t + ((int64_t)h * kD + ch) * Nkp + t * kTileKeys + q * 16) = w;
    }
}

}  // namespace
