// The e4m3 V operand of the opt-in 8-bit P V self-attention (fg_attn_fwd_pv8_bf16, include/fairygen_hip_pv8.h), for gfx950.
//
// The recipe (DESIGN §5 "e4m3 P V"), per head, v (N, 128) bf16 as the qkv GEMM left it:
//   sv[c] = max(max over the N keys of |v[j][c]| / 448, 2^-20)   one scale per head and channel,
//   v8    = e4m3(v / sv[c])   round-to-nearest-even, saturating: the division and conversion of attn_qk8_quant.h,
//   v8t   = v8 transposed, (H, 128, Nkp) bytes, Nkp = N rounded up to whole 64-key tiles, the padding written as zero, the keys of a tile
//           in the order of the attention kernel's P fragment: byte p of a tile is key kPv8Key(p) (attention.hip, the PV8 form).
// Two stream-ordered launches, no atomics, nothing waits on another workgroup:
//   1. up to 256 x ceil(H / 4) workgroups walk the rows and leave, per channel, the maximum of |v| over the rows they saw: one record
//      each in the caller's scratch (fg_attn_pv8_scratch_bytes);
//   2. a workgroup per (head, up to 32 strides of tiles) reduces the records of its 128 channels -- a maximum does not depend on the
//      order, so sv is exact -- and converts its tiles: 16-byte reads of v, the dwords of four adjacent keys of one channel into an LDS
//      image of the transposed tile, 16-byte reads of that image, 16-byte writes of v8t.
// HBM-bound: v is read twice, half a byte written per byte read.
#include "common.h"
#include "../../include/fairygen_hip_pv8.h"
#include "attn_qk8_quant.h"
#include "attn_pv8_parts.h"

namespace {

constexpr int kMaxTileBlocks = 32;

// Workgroup (x, h) of 256: the scales of head h from the `parts` records, then the tiles x, x + gridDim.x, ..  Thread t converts the 8
// channels of chunk cl = t & 15 of the 4 keys 4 kg .. 4 kg + 3, kg = t >> 4: 8 dwords, one per channel, to row 8 cl + j of the image at
// dword pv8_dword(kg) ^ cl (the XOR spreads the 16 chunks of a key group over 16 banks; it permutes the dwords of a 16-byte chunk among
// themselves and the chunks of a row among themselves, and the read below undoes both).
__global__ __launch_bounds__(256) void attn_quant_vt_kernel(const bf16* __restrict__ v, int64_t ldv, const float* __restrict__ rec, int parts,
                                                            uint8_t* __restrict__ v8t, float* __restrict__ sv, int64_t N, int64_t Nkp, int H) {
    __shared__ float red_s[kD];
    __shared__ float sv_s[kD];
    __shared__ __attribute__((aligned(16))) uint32_t img[kD][16];
    const int h = blockIdx.y, tid = threadIdx.x, C = H * kD;
    {
        const int c = tid & (kD - 1), g = tid >> 7;
        float a = 0.f;
        for (int p = g; p < parts; p += 2) a = fmaxf(a, rec[(int64_t)p * C + h * kD + c]);
        if (g == 1) red_s[c] = a;
        __syncthreads();
        if (g == 0) {
            const float s = fmaxf(fmaxf(a, red_s[c]) / kE4M3Max, kScaleFloor);
            sv_s[c] = s;
            if (blockIdx.x == 0) sv[h * kD + c] = s;
        }
        __syncthreads();
    }
    const int cl = tid & 15, kg = tid >> 4;
    float s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = sv_s[cl * 8 + j];
    const int wr = pv8_dword(kg) ^ cl;
    const int64_t nt = Nkp / kTileKeys;
    for (int64_t t = blockIdx.x; t < nt; t += gridDim.x) {
        float f[4][8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t key = t * kTileKeys + 4 * kg + i;
            bf16x8 x = {};
            if (key < N) x = *reinterpret_cast<const bf16x8*>(v + key * ldv + (int64_t)h * kD + cl * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) f[i][j] = key < N ? (float)x[j] : 0.f;      // the padding keys of the last tile: zero bytes
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            img[cl * 8 + j][wr] = cvt2_e4m3(f[0][j] / s[j], f[1][j] / s[j]) | (cvt2_e4m3(f[2][j] / s[j], f[3][j] / s[j]) << 16);
        __syncthreads();
        pv8_store_tile(img, v8t, h, Nkp, t, tid);
        __syncthreads();
    }
}

}  // namespace

extern "C" int fg_attn_pv8_version(void) { return 1; }

extern "C" int64_t fg_attn_pv8_scratch_bytes(int64_t N, int H) {
    if (N < 1 || H < 1 || H > 65535) {
        fg_set_error("fg_attn_pv8_scratch_bytes: N must be positive, H in 1..65535 (got N=%lld H=%d)", (long long)N, H);
        return -1;
    }
    return v_stat_parts(N) * H * kD * 4;
}

extern "C" int fg_attn_quant_vt_bf16(const void* v, int64_t ldv, void* v8t, float* sv, void* scratch, int64_t scratch_bytes, int64_t N, int H,
                                     int D, fg_stream_t stream) {
    FG_CHECK_ARG(v && v8t && sv && scratch, "fg_attn_quant_vt_bf16: null pointer");
    FG_CHECK_ARG(D == kD, "fg_attn_quant_vt_bf16: only head_dim 128 is supported (got %d)", D);
    FG_CHECK_ARG(N > 0 && H > 0 && H <= 65535, "fg_attn_quant_vt_bf16: N must be positive, H in 1..65535");
    const int64_t hd = (int64_t)H * D, nkp = (N + kTileKeys - 1) / kTileKeys * kTileKeys;
    FG_CHECK_ARG(ldv >= hd && ldv % 8 == 0, "fg_attn_quant_vt_bf16: ldv must be >= H*D and a multiple of 8");
    FG_CHECK_ARG(FG_ALIGNED16(v) && FG_ALIGNED16(v8t) && FG_ALIGNED16(sv) && FG_ALIGNED16(scratch),
                 "fg_attn_quant_vt_bf16: v, v8t, sv and scratch must be 16-byte aligned");
    const int64_t parts = v_stat_parts(N);
    FG_CHECK_ARG(scratch_bytes >= parts * hd * 4, "fg_attn_quant_vt_bf16: scratch must hold %lld bytes (got %lld)", (long long)(parts * hd * 4),
                 (long long)scratch_bytes);
    hipLaunchKernelGGL(attn_v_stats_kernel, dim3((unsigned)parts, (unsigned)((hd / 8 + 63) / 64)), dim3(256), 0, (hipStream_t)stream, (const bf16*)v,
                       ldv, (float*)scratch, N, (int)hd);
    if (int e = fg_launch_status("fg_attn_quant_vt_bf16 (v statistics)")) return e;
    const int64_t nt = nkp / kTileKeys;
    hipLaunchKernelGGL(attn_quant_vt_kernel, dim3((unsigned)(nt < kMaxTileBlocks ? nt : kMaxTileBlocks), (unsigned)H), dim3(256), 0,
                       (hipStream_t)stream, (const bf16*)v, ldv, (const float*)scratch, (int)parts, (uint8_t*)v8t, sv, N, nkp, H);
    return fg_launch_status("fg_attn_quant_vt_bf16");
}
