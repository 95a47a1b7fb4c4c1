// The row arithmetic of RMSNorm(+RoPE), shared by rmsnorm_rope_kernel (dit_elementwise.hip) and the e4m3 operand producers
// (attn_qk8_fused.hip): one wave owns one token row held in registers, so whatever leaves the wave — the bf16 row, or its e4m3 form —
// is made from the same bf16-rounded values by construction.
#pragma once
#include "common.h"

namespace {

constexpr int kMaxVec = 8;            // 8 lanes-vectors * 64 lanes * 8 elems = 4096 channels max
constexpr int kRowsPerBlock = 4;      // 4 waves per 256-thread workgroup

template <int NV>
struct RowT {
    float v[NV][8];
};
typedef RowT<kMaxVec> Row;

template <int NV>
__device__ __forceinline__ void load_row(const bf16* p, int C, int lane, RowT<NV>& r) {
    const int nvec = C >> 3;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int vi = lane + i * 64;
        if (vi < nvec) {
            bf16x8 t = *reinterpret_cast<const bf16x8*>(p + (int64_t)vi * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) r.v[i][j] = (float)t[j];
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) r.v[i][j] = 0.f;
        }
    }
}

__device__ __forceinline__ bf16x8 ld8(const bf16* p) { return *reinterpret_cast<const bf16x8*>(p); }
__device__ __forceinline__ void st8(bf16* p, const float* f) {
    bf16x8 t;
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = (bf16)f[j];
    *reinterpret_cast<bf16x8*>(p) = t;
}

// RMSNorm over the whole row, * weight, then RoPE on adjacent pairs, in two steps a kernel calls from its own loop over the row's
// vectors: rope_begin (the row's 1/rms and, where they can be hoisted, its rotation pairs), then rope_vec for every vector inside C,
// which hands back the vector's 8 bf16-rounded values.
// F32TAB false: fp64 cos / sin tables and an fp64 rotation, the reference's arithmetic (43 us of fp64 VALU + 16-byte table loads per
// pair on top of the 77 us the HBM-bound norm takes at N = 27 280).  F32TAB true: `ct` is ONE interleaved fp32 table (rows,
// head_dim/2, {cos, sin}) = the fp64 table rounded once, rotation as two fp32 FMAs: the bf16 result differs from the fp64 one only
// where the exact value lies within ~2e-7 relative of a bf16 rounding boundary (measured in tests/test_hip_kernels.py).
// PLAIN: head_dim a power of two — the runtime `% head_dim` (an integer division per vector) becomes a mask.
struct RopeRow {
    float rinv;
    bool hoist;
    f32x4 h0, h1;
};

// NV: the vectors a lane holds (the ones past C zero); the sum of squares over fewer vectors only leaves out terms that are +0, so it
// is the same sum.
template <bool F32TAB, bool PLAIN, int NV>
__device__ __forceinline__ RopeRow rope_begin(const RowT<NV>& r, const void* ctv, int64_t row, int C, int head_dim, float eps, int lane) {
    RopeRow c;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) q += r.v[i][j] * r.v[i][j];
    const float ms = wave_sum(q) / (float)C;
    c.rinv = 1.0f / sqrtf(ms + eps);
    const int half = head_dim >> 1;
    // fp32 table: a lane's vectors are 512 channels apart, so when head_dim divides 512 (128 here) every vector of the lane
    // sits at the same channel offset inside its head and needs the SAME four (cos, sin) pairs: loaded once per row
    c.hoist = F32TAB && ctv != nullptr && (512 % head_dim) == 0;
    c.h0 = f32x4{0.f, 0.f, 0.f, 0.f};
    c.h1 = f32x4{0.f, 0.f, 0.f, 0.f};
    if (c.hoist) {
        const int d_lane = PLAIN ? ((lane * 8) & (head_dim - 1)) : ((lane * 8) % head_dim);
        const f32x4* tp = reinterpret_cast<const f32x4*>(static_cast<const float*>(ctv) + (row * half + (d_lane >> 1)) * 2);
        c.h0 = tp[0];
        c.h1 = tp[1];
    }
    return c;
}

// o = the 8 values of vector vi (raw values rv, weights wv) after the norm and the rotation, each rounded to bf16.
template <bool F32TAB, bool PLAIN>
__device__ __forceinline__ void rope_vec(const RopeRow& c, const float* rv, const bf16x8 wv, const void* ctv, const void* stv, int64_t row,
                                         int head_dim, int vi, float* o) {
    const int half = head_dim >> 1;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = rbf(rbf(rv[j] * c.rinv) * (float)wv[j]);
    if (ctv != nullptr) {
        const int d0 = PLAIN ? ((vi * 8) & (head_dim - 1)) : ((vi * 8) % head_dim);          // channel within the head, multiple of 8
        if (F32TAB) {
            f32x4 t0 = c.h0, t1 = c.h1;                  // (c0,s0,c1,s1) (c2,s2,c3,s3)
            if (!c.hoist) {
                const f32x4* tp = reinterpret_cast<const f32x4*>(static_cast<const float*>(ctv) + (row * half + (d0 >> 1)) * 2);
                t0 = tp[0];
                t1 = tp[1];
            }
            const float cs[8] = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float a = o[2 * j], b = o[2 * j + 1], cc = cs[2 * j], sn = cs[2 * j + 1];
                o[2 * j] = rbf(__builtin_fmaf(a, cc, -(b * sn)));
                o[2 * j + 1] = rbf(__builtin_fmaf(a, sn, b * cc));
            }
        } else {
            const double* cp = static_cast<const double*>(ctv) + row * half + (d0 >> 1);
            const double* sp = static_cast<const double*>(stv) + row * half + (d0 >> 1);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double a = (double)o[2 * j], b = (double)o[2 * j + 1];
                const double cc = cp[j], sn = sp[j];
                o[2 * j] = (float)(bf16)(a * cc - b * sn);
                o[2 * j + 1] = (float)(bf16)(a * sn + b * cc);
            }
        }
    }
}

}  // namespace
