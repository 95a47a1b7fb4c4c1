// DiT token-side kernels: LayerNorm+modulate, LayerNorm affine, gate-residual (+ fused next norm),
// RMSNorm(+RoPE), activations, CFG+Euler.  All are HBM-bound: one wave owns one token row, keeps it in
// registers (C <= 4096 -> <= 8 x 16-byte vectors per lane), reduces with wave shuffles (no LDS, no
// barrier) and touches every byte exactly once with 16-byte coalesced accesses.
// Rounding points mirror the reference's bf16 tensor arithmetic op by op (see include/fairygen_hip.h).
#include "common.h"
#include "../../include/fairygen_hip_rowbatch.h"      // the batched forms of the row kernels that read a per-row table
#include "../../include/fairygen_hip_rowbatch8.h"     // ... and of the norms with the fp8 output
#include "../../include/fairygen_hip_lorabatch.h"     // ... and of the two-output norm of unfused adapters
#include "rmsnorm_rope_row.h"     // Row, load_row, ld8, st8 and the RMSNorm+RoPE row arithmetic

// Row kernels (one wave per token row held in registers): second launch-bound = minimum waves per SIMD the register
// allocation must allow (FG_ROW_MIN_WAVES; measured in tools/microbench.py elementwise).
#ifndef FG_ROW_MIN_WAVES
#define FG_ROW_MIN_WAVES 4
#endif
#define FG_ROW_BOUNDS __launch_bounds__(256, FG_ROW_MIN_WAVES)

namespace {

// mean / rstd of a row held in registers (two-pass, fp32).
__device__ __forceinline__ void row_moments(const Row& r, int C, int lane, float eps, float& mean, float& rstd) {
    const int nvec = C >> 3;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kMaxVec; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) s += r.v[i][j];
    mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < kMaxVec; ++i) {
        if (lane + i * 64 < nvec) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float d = r.v[i][j] - mean;
                q += d * d;
            }
        }
    }
    const float var = wave_sum(q) / (float)C;
    rstd = 1.0f / sqrtf(var + eps);
}

__device__ __forceinline__ int64_t mod_row(int64_t row, int64_t mod_rows, int64_t first_rows) {
    return mod_rows == 1 ? 0 : (mod_rows == 2 ? (row < first_rows ? 0 : 1) : row);
}

// norm_out = modulate(LN(row)) or LN(row)*w+b, written from registers.
template <int MODE>
__device__ __forceinline__ void norm_store(const Row& r, int C, int lane, float eps, const bf16* p0, const bf16* p1,
                                           bf16* out) {
    const int nvec = C >> 3;
    float mean, rstd;
    row_moments(r, C, lane, eps, mean, rstd);
#pragma unroll
    for (int i = 0; i < kMaxVec; ++i) {
        const int vi = lane + i * 64;
        if (vi < nvec) {
            const bf16x8 a = ld8(p0 + (int64_t)vi * 8);
            const bf16x8 b = ld8(p1 + (int64_t)vi * 8);
            float o[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float n = (r.v[i][j] - mean) * rstd;
                if (MODE == 0) {  // p0 = shift, p1 = scale
                    const float y = rbf(n);
                    const float s1 = rbf(1.0f + (float)b[j]);
                    o[j] = rbf(y * s1) + (float)a[j];
                } else {          // p0 = weight, p1 = bias
                    o[j] = n * (float)a[j] + (float)b[j];
                }
            }
            st8(out + (int64_t)vi * 8, o);
        }
    }
}

// Two fp32 -> two e4m3 bytes in the low half of a dword (v_cvt_pk_fp8_f32: RNE, OCP e4m3fn on gfx950).
__device__ __forceinline__ uint32_t cvt2_fp8(float a, float b) {
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false) & 0xffffu;
}

// The same normalised row as norm_store, but handed to the fp8 Linear that consumes it (AutoWrappedLinear.fp8_linear,
// core/vram/layers.py:331-342) without a trip through HBM: the bf16-rounded values stay in registers, the row maximum gives the
// dynamic scale, the row leaves as e4m3 bytes + one fp32 scale — exactly fg_fp8_quant_rows_bf16's arithmetic on norm_store's output.
// DUAL: the bf16 row is written as well (out16, norm_store's bytes), for a hot-loaded LoRA adapter that reads the bf16 activation next to
// the fp8 Linear (AutoWrappedLinear.forward, core/vram/layers.py:429-436).
template <int MODE, bool DUAL = false>
__device__ __forceinline__ void norm_store_fp8(Row& r, int C, int lane, float eps, const bf16* p0, const bf16* p1,
                                               uint8_t* out8, float* scale_out, float fp8_max, bf16* out16 = nullptr) {
    const int nvec = C >> 3;
    float mean, rstd;
    row_moments(r, C, lane, eps, mean, rstd);
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < kMaxVec; ++i) {
        const int vi = lane + i * 64;
        if (vi < nvec) {
            const bf16x8 a = ld8(p0 + (int64_t)vi * 8);
            const bf16x8 b = ld8(p1 + (int64_t)vi * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float n = (r.v[i][j] - mean) * rstd;
                float o;
                if (MODE == 0) {
                    const float y = rbf(n);
                    const float s1 = rbf(1.0f + (float)b[j]);
                    o = rbf(y * s1) + (float)a[j];
                } else {
                    o = n * (float)a[j] + (float)b[j];
                }
                r.v[i][j] = rbf(o);
                amax = fmaxf(amax, fabsf(r.v[i][j]));
            }
            if (DUAL) st8(out16 + (int64_t)vi * 8, r.v[i]);
        }
    }
    amax = wave_max(amax);
    const float sc = fmaxf(rbf(amax / fp8_max), 1.0f);
    const float denom = sc + 1e-8f;
    if (lane == 0) *scale_out = sc;
#pragma unroll
    for (int i = 0; i < kMaxVec; ++i) {
        const int vi = lane + i * 64;
        if (vi < nvec) {
            u32x2 w;
            w[0] = cvt2_fp8(r.v[i][0] / denom, r.v[i][1] / denom) | (cvt2_fp8(r.v[i][2] / denom, r.v[i][3] / denom) << 16);
            w[1] = cvt2_fp8(r.v[i][4] / denom, r.v[i][5] / denom) | (cvt2_fp8(r.v[i][6] / denom, r.v[i][7] / denom) << 16);
            *reinterpret_cast<u32x2*>(out8 + (int64_t)vi * 8) = w;
        }
    }
}

__global__ FG_ROW_BOUNDS void ln_modulate_fp8_kernel(const bf16* __restrict__ x, const bf16* __restrict__ shift,
                                                     const bf16* __restrict__ scale, uint8_t* __restrict__ out8,
                                                     float* __restrict__ scale_out, int64_t rows, int C, float eps, int64_t mod_rows,
                                                     int64_t first_rows, int64_t mod_ld, float fp8_max) {
#include "ln_modulate_fp8_body.inc"
}

// (bf16 row, e4m3 row, scale) of one norm in one pass.  MODE 0: p0 = shift, p1 = scale (modulation rows); 1: p0 = weight, p1 = bias.
template <int MODE>
__global__ FG_ROW_BOUNDS void ln_dual_kernel(const bf16* __restrict__ x, const bf16* __restrict__ p0, const bf16* __restrict__ p1,
                                             bf16* __restrict__ out, uint8_t* __restrict__ out8, float* __restrict__ scale_out,
                                             int64_t rows, int C, float eps, int64_t mod_rows, int64_t first_rows, int64_t mod_ld,
                                             float fp8_max) {
#include "ln_dual_body.inc"
}

// ... on a batch that shares the table (include/fairygen_hip_lorabatch.h; MODE 0 only — the affine form reads no table and runs on all
// rows as it is): as ln_modulate_fp8_b_kernel, with the bf16 row moving with x as well
template <int MODE>
__global__ FG_ROW_BOUNDS void ln_dual_b_kernel(const bf16* __restrict__ x, const bf16* __restrict__ p0, const bf16* __restrict__ p1,
                                               bf16* __restrict__ out, uint8_t* __restrict__ out8, float* __restrict__ scale_out,
                                               int64_t rows, int C, float eps, int64_t mod_rows, int64_t first_rows, int64_t mod_ld,
                                               float fp8_max) {
    const int64_t e0 = (int64_t)blockIdx.y * rows * C;
    x += e0; out += e0; out8 += e0; scale_out += (int64_t)blockIdx.y * rows;
#include "ln_dual_body.inc"
}

__global__ FG_ROW_BOUNDS void ln_modulate_kernel(const bf16* __restrict__ x, const bf16* __restrict__ shift,
                                                          const bf16* __restrict__ scale, bf16* __restrict__ out,
                                                          int64_t rows, int C, float eps, int64_t mod_rows,
                                                          int64_t first_rows, int64_t mod_ld) {
#include "ln_modulate_body.inc"
}

// The batched forms (include/fairygen_hip_rowbatch.h): x / y / the outputs are the B * rows rows of one matrix, the last grid dimension
// picks the batch element, and the element runs the body of the single-element kernel on its own pointers — the modulation / RoPE table
// is ONE element's, read by the row inside the element.  No workgroup holds rows of two elements.
__global__ FG_ROW_BOUNDS void ln_modulate_b_kernel(const bf16* __restrict__ x, const bf16* __restrict__ shift,
                                                   const bf16* __restrict__ scale, bf16* __restrict__ out,
                                                   int64_t rows, int C, float eps, int64_t mod_rows,
                                                   int64_t first_rows, int64_t mod_ld) {
    const int64_t e0 = (int64_t)blockIdx.y * rows * C;
    x += e0; out += e0;
#include "ln_modulate_body.inc"
}

// ... and with the fp8 output (include/fairygen_hip_rowbatch8.h): the e4m3 rows move with x, the row scales by the element's rows
__global__ FG_ROW_BOUNDS void ln_modulate_fp8_b_kernel(const bf16* __restrict__ x, const bf16* __restrict__ shift,
                                                       const bf16* __restrict__ scale, uint8_t* __restrict__ out8,
                                                       float* __restrict__ scale_out, int64_t rows, int C, float eps, int64_t mod_rows,
                                                       int64_t first_rows, int64_t mod_ld, float fp8_max) {
    const int64_t e0 = (int64_t)blockIdx.y * rows * C;
    x += e0; out8 += e0; scale_out += (int64_t)blockIdx.y * rows;
#include "ln_modulate_fp8_body.inc"
}

__global__ FG_ROW_BOUNDS void ln_affine_kernel(const bf16* __restrict__ x, const bf16* __restrict__ w,
                                                        const bf16* __restrict__ b, bf16* __restrict__ out,
                                                        int64_t rows, int C, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= rows) return;
    Row r;
    load_row(x + row * C, C, lane, r);
    norm_store<1>(r, C, lane, eps, w, b, out + row * C);
}

// x_out = x + gate*y ; optional fused norm of x_out.  MODE: -1 none, 0 modulate, 1 affine.
template <int MODE>
__global__ FG_ROW_BOUNDS void residual_kernel(const bf16* __restrict__ x, const bf16* __restrict__ y,
                                                       const bf16* __restrict__ gate, bf16* __restrict__ x_out,
                                                       const bf16* __restrict__ p0, const bf16* __restrict__ p1,
                                                       bf16* __restrict__ norm_out, int64_t rows, int C, float eps,
                                                       int64_t mod_rows, int64_t first_rows, int64_t mod_ld,
                                                       uint8_t* __restrict__ norm_fp8 = nullptr, float* __restrict__ norm_scale = nullptr,
                                                       float fp8_max = 0.f) {
#include "residual_body.inc"
}

// batched (bf16 norm output only: the fp8 output has residual_fp8_b_kernel below); MODE -1 has no norm_out
template <int MODE>
__global__ FG_ROW_BOUNDS void residual_b_kernel(const bf16* __restrict__ x, const bf16* __restrict__ y,
                                                const bf16* __restrict__ gate, bf16* __restrict__ x_out,
                                                const bf16* __restrict__ p0, const bf16* __restrict__ p1,
                                                bf16* __restrict__ norm_out, int64_t rows, int C, float eps,
                                                int64_t mod_rows, int64_t first_rows, int64_t mod_ld) {
    uint8_t* const norm_fp8 = nullptr;
    float* const norm_scale = nullptr;
    const float fp8_max = 0.f;
    const int64_t e0 = (int64_t)blockIdx.y * rows * C;
    x += e0; y += e0; x_out += e0;
    if (MODE >= 0) norm_out += e0;
#include "residual_body.inc"
}

// batched with the fp8 norm output only (include/fairygen_hip_rowbatch8.h; MODE 0 or 1): no bf16 norm row, so the body's fp8 branch is
// the whole kernel — the entry point refuses a null norm_fp8
template <int MODE>
__global__ FG_ROW_BOUNDS void residual_fp8_b_kernel(const bf16* __restrict__ x, const bf16* __restrict__ y,
                                                    const bf16* __restrict__ gate, bf16* __restrict__ x_out,
                                                    const bf16* __restrict__ p0, const bf16* __restrict__ p1,
                                                    uint8_t* __restrict__ norm_fp8, float* __restrict__ norm_scale, int64_t rows, int C,
                                                    float eps, int64_t mod_rows, int64_t first_rows, int64_t mod_ld, float fp8_max) {
    bf16* const norm_out = nullptr;
    const int64_t e0 = (int64_t)blockIdx.y * rows * C;
    x += e0; y += e0; x_out += e0; norm_fp8 += e0; norm_scale += (int64_t)blockIdx.y * rows;
    __builtin_assume(norm_fp8 != nullptr);
#include "residual_body.inc"
}

// RMSNorm over the whole row, * weight, then RoPE on adjacent pairs: the arithmetic and its table modes are rope_begin's and
// rope_vec's (rmsnorm_rope_row.h).  PLAIN: plain rows (group_cols == C) and head_dim a power of two — the runtime `/ group_cols` and `% head_dim`
// (an integer division each, per vector: about as many VALU instructions as the norm itself) become a constant and a mask.
template <bool F32TAB, bool PLAIN = false>
__global__ FG_ROW_BOUNDS void rmsnorm_rope_kernel(const bf16* __restrict__ x, int64_t ldx,
                                                           const bf16* __restrict__ w, const void* __restrict__ ctv,
                                                           const void* __restrict__ stv, bf16* __restrict__ out,
                                                           int64_t rows, int C, int head_dim, float eps, int group_cols,
                                                           int64_t out_group_stride, int64_t out_ld) {
#include "rmsnorm_rope_body.inc"
}

// batched, plain rows only (no grouped form): x keeps its leading dimension, out is dense
template <bool F32TAB, bool PLAIN>
__global__ FG_ROW_BOUNDS void rmsnorm_rope_b_kernel(const bf16* __restrict__ x, int64_t ldx, const bf16* __restrict__ w,
                                                    const void* __restrict__ ctv, const void* __restrict__ stv,
                                                    bf16* __restrict__ out, int64_t rows, int C, int head_dim, float eps) {
    const int group_cols = C;
    const int64_t out_group_stride = 0, out_ld = C;
    const int64_t r0 = (int64_t)blockIdx.y * rows;
    x += r0 * ldx; out += r0 * C;
#include "rmsnorm_rope_body.inc"
}

// dst[g][r][0..cols) = src[g][r][0..cols) with independent group / row strides on both sides (16-byte vectors):
// the head-group <-> token re-layouts around the Ulysses all-to-alls.
__global__ __launch_bounds__(256) void copy_groups_kernel(const bf16* __restrict__ src, int64_t sgs, int64_t sld,
                                                          bf16* __restrict__ dst, int64_t dgs, int64_t dld, int groups,
                                                          int64_t rows, int vec_per_row) {
    const int64_t total = (int64_t)groups * rows * vec_per_row;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t rg = i / vec_per_row;            // row-major over (row, group): a wave reads one source row
        const int v = (int)(i - rg * vec_per_row);
        const int64_t r = rg / groups;
        const int g = (int)(rg - r * groups);
        *reinterpret_cast<u32x4*>(dst + g * dgs + r * dld + v * 8) =
            *reinterpret_cast<const u32x4*>(src + g * sgs + r * sld + v * 8);
    }
}


template <int KIND>
__global__ __launch_bounds__(256) void act_kernel(const bf16* __restrict__ x, bf16* __restrict__ out, int64_t nvec) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
        const bf16x8 v = ld8(x + i * 8);
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = KIND == 0 ? silu_f((float)v[j]) : gelu_tanh_f((float)v[j]);
        st8(out + i * 8, o);
    }
}

// One element of the CFG combine + Euler step, with the reference's bf16 rounding points (fg_cfg_euler_bf16, fairygen_hip.h).
__device__ __forceinline__ float cfg_euler_one(float lat, float p, float ng, bool has_nega, float cfg, float dsigma) {
    const float pred = has_nega ? rbf(ng + rbf(cfg * rbf(p - ng))) : p;
    return rbf(lat + rbf(pred * dsigma));
}

__global__ __launch_bounds__(256) void cfg_euler_kernel(const bf16* __restrict__ lat, const bf16* __restrict__ posi,
                                                        const bf16* __restrict__ nega, bf16* __restrict__ out,
                                                        int64_t n, float cfg, float dsigma) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = (bf16)cfg_euler_one((float)lat[i], (float)posi[i], nega != nullptr ? (float)nega[i] : 0.0f, nega != nullptr, cfg, dsigma);
}

// fg_cfg_euler_dev_bf16: dsigma = dsigma_table[*step], both read here; elements of latent frame 0 (offset < first_n inside their
// frame_stride-long channel block) take `first` instead.  nvec 8-element vectors (0 when a pointer is not 16-byte aligned), then the
// n - 8 * nvec elements behind them one at a time.  out may alias lat: every element is read before it is written, by one thread.
__global__ __launch_bounds__(256) void cfg_euler_dev_kernel(const bf16* lat, const bf16* __restrict__ posi, const bf16* __restrict__ nega,
                                                            bf16* out, int64_t n, int64_t nvec, float cfg,
                                                            const float* __restrict__ dsigma_table, const int* __restrict__ step,
                                                            const bf16* __restrict__ first, int64_t first_n, int64_t frame_stride) {
    const float dsigma = dsigma_table[*step];
    const bool has_nega = nega != nullptr;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = tid; i < nvec; i += nthreads) {
        const bf16x8 l = ld8(lat + i * 8), p = ld8(posi + i * 8);
        const bf16x8 g = has_nega ? ld8(nega + i * 8) : p;
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = cfg_euler_one((float)l[j], (float)p[j], (float)g[j], has_nega, cfg, dsigma);
        if (first != nullptr) {
            int64_t ch = (i * 8) / frame_stride, r = i * 8 - ch * frame_stride;      // channel block and offset inside it of element 0
            if (r < first_n || r + 7 >= frame_stride) {      // else: all 8 elements lie behind frame 0 of one channel block
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if (r < first_n) o[j] = (float)first[ch * first_n + r];
                    if (++r == frame_stride) { r = 0; ++ch; }
                }
            }
        }
        st8(out + i * 8, o);
    }
    for (int64_t i = nvec * 8 + tid; i < n; i += nthreads) {
        float o = cfg_euler_one((float)lat[i], (float)posi[i], has_nega ? (float)nega[i] : 0.0f, has_nega, cfg, dsigma);
        if (first != nullptr) {
            const int64_t ch = i / frame_stride, r = i - ch * frame_stride;
            if (r < first_n) o = (float)first[ch * first_n + r];
        }
        out[i] = (bf16)o;
    }
}

inline int check_rows(const char* fn, int64_t rows, int C, int64_t mod_rows, int64_t first_rows) {
    FG_CHECK_ARG(rows >= 0 && C > 0 && (C % 8) == 0 && C <= kMaxVec * 512, "%s: need C %% 8 == 0 and C <= %d (got rows=%lld C=%d)",
                 fn, kMaxVec * 512, (long long)rows, C);
    FG_CHECK_ARG(mod_rows == 1 || mod_rows == 2 || mod_rows == rows, "%s: mod_rows must be 1, 2 or rows (got %lld)", fn,
                 (long long)mod_rows);
    FG_CHECK_ARG(first_rows >= 0 && first_rows <= rows, "%s: first_rows out of range", fn);
    return FG_OK;
}

inline dim3 row_grid(int64_t rows) { return dim3((unsigned)((rows + kRowsPerBlock - 1) / kRowsPerBlock)); }

// the batched forms: the workgroups of one element's rows, times B in the second grid dimension (at most 65535)
inline dim3 row_grid_b(int64_t rows, int B) { return dim3((unsigned)((rows + kRowsPerBlock - 1) / kRowsPerBlock), (unsigned)B); }

inline int check_batch(const char* fn, int B) {
    FG_CHECK_ARG(B >= 1 && B <= 65535, "%s: B must be in 1..65535 (got %d)", fn, B);
    return FG_OK;
}

}  // namespace

extern "C" {

int fg_ln_modulate_bf16(const void* x, const void* shift, const void* scale, void* out, int64_t rows, int C, float eps,
                        int64_t mod_rows, int64_t first_rows, int64_t mod_ld, fg_stream_t stream) {
    if (int e = check_rows("fg_ln_modulate_bf16", rows, C, mod_rows, first_rows)) return e;
    FG_CHECK_ARG(x && shift && scale && out, "fg_ln_modulate_bf16: null pointer");
    FG_CHECK_ARG(FG_ALIGNED16(x) && FG_ALIGNED16(shift) && FG_ALIGNED16(scale) && FG_ALIGNED16(out) && mod_ld % 8 == 0,
                 "fg_ln_modulate_bf16: pointers / mod_ld must be 16-byte aligned");
    if (rows == 0) return FG_OK;
    hipLaunchKernelGGL(ln_modulate_kernel, row_grid(rows), dim3(256), 0, (hipStream_t)stream, (const bf16*)x,
                       (const bf16*)shift, (const bf16*)scale, (bf16*)out, rows, C, eps, mod_rows, first_rows, mod_ld);
    return fg_launch_status("fg_ln_modulate_bf16");
}

int fg_ln_modulate_fp8_bf16(const void* x, const void* shift, const void* scale, void* out_fp8, float* out_scale, int64_t rows, int C,
                            float eps, int64_t mod_rows, int64_t first_rows, int64_t mod_ld, float fp8_max, fg_stream_t stream) {
    if (int e = check_rows("fg_ln_modulate_fp8_bf16", rows, C, mod_rows, first_rows)) return e;
    FG_CHECK_ARG(x && shift && scale && out_fp8 && out_scale, "fg_ln_modulate_fp8_bf16: null pointer");
    FG_CHECK_ARG(FG_ALIGNED16(x) && FG_ALIGNED16(shift) && FG_ALIGNED16(scale) && (((uintptr_t)out_fp8) & 7) == 0 && mod_ld % 8 == 0 &&
                     fp8_max > 0.f,
                 "fg_ln_modulate_fp8_bf16: pointers / mod_ld must be 16-byte aligned (out_fp8: 8), fp8_max positive");
    if (rows == 0) return FG_OK;
    hipLaunchKernelGGL(ln_modulate_fp8_kernel, row_grid(rows), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, (const bf16*)shift,
                       (const bf16*)scale, (uint8_t*)out_fp8, out_scale, rows, C, eps, mod_rows, first_rows, mod_ld, fp8_max);
    return fg_launch_status("fg_ln_modulate_fp8_bf16");
}

int fg_ln_modulate_dual_bf16(const void* x, const void* shift, const void* scale, void* out, void* out_fp8, float* out_scale,
                             int64_t rows, int C, float eps, int64_t mod_rows, int64_t first_rows, int64_t mod_ld, float fp8_max,
                             fg_stream_t stream) {
    if (int e = check_rows("fg_ln_modulate_dual_bf16", rows, C, mod_rows, first_rows)) return e;
    FG_CHECK_ARG(x && shift && scale && out && out_fp8 && out_scale, "fg_ln_modulate_dual_bf16: null pointer");
    FG_CHECK_ARG(FG_ALIGNED16(x) && FG_ALIGNED16(shift) && FG_ALIGNED16(scale) && FG_ALIGNED16(out) && (((uintptr_t)out_fp8) & 7) == 0 &&
                     mod_ld % 8 == 0 && fp8_max > 0.f,
                 "fg_ln_modulate_dual_bf16: pointers / mod_ld must be 16-byte aligned (out_fp8: 8), fp8_max positive");
    if (rows == 0) return FG_OK;
    hipLaunchKernelGGL(ln_dual_kernel<0>, row_grid(rows), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, (const bf16*)shift,
                       (const bf16*)scale, (bf16*)out, (uint8_t*)out_fp8, out_scale, rows, C, eps, mod_rows, first_rows, mod_ld, fp8_max);
    return fg_launch_status("fg_ln_modulate_dual_bf16");
}

int fg_ln_affine_dual_bf16(const void* x, const void* w, const void* b, void* out, void* out_fp8, float* out_scale, int64_t rows, int C,
                           float eps, float fp8_max, fg_stream_t stream) {
    if (int e = check_rows("fg_ln_affine_dual_bf16", rows, C, 1, 0)) return e;
    FG_CHECK_ARG(x && w && b && out && out_fp8 && out_scale, "fg_ln_affine_dual_bf16: null pointer");
    FG_CHECK_ARG(FG_ALIGNED16(x) && FG_ALIGNED16(w) && FG_ALIGNED16(b) && FG_ALIGNED16(out) && (((uintptr_t)out_fp8) & 7) == 0 &&
                     fp8_max > 0.f,
                 "fg_ln_affine_dual_bf16: pointers must be 16-byte aligned (out_fp8: 8), fp8_max positive");
    if (rows == 0) return FG_OK;
    hipLaunchKernelGGL(ln_dual_kernel<1>, row_grid(rows), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, (const bf16*)w,
                       (const bf16*)b, (bf16*)out, (uint8_t*)out_fp8, out_scale, rows, C, eps, (int64_t)1, (int64_t)0, (int64_t)0, fp8_max);
    return fg_launch_status("fg_ln_affine_dual_bf16");
}

int fg_residual_ln_fp8_bf16(const void* x, const void* y, const void* gate, void* x_out, const void* p0, const void* p1,
                            void* norm_fp8, float* norm_scale, int mode, int64_t rows, int C, float eps, int64_t mod_rows,
                            int64_t first_rows, int64_t mod_ld, float fp8_max, fg_stream_t stream) {
    FG_CHECK_ARG(mode == 0 || mode == 1, "fg_residual_ln_fp8_bf16: mode must be 0 (modulate) or 1 (affine)");
    const bool need_mod = gate != nullptr || mode == 0;
    if (int e = check_rows("fg_residual_ln_fp8_bf16", rows, C, need_mod ? mod_rows : 1, need_mod ? first_rows : 0)) return e;
    FG_CHECK_ARG(x && y && x_out && p0 && p1 && norm_fp8 && norm_scale, "fg_residual_ln_fp8_bf16: null pointer");
    FG_CHECK_ARG(FG_ALIGNED16(x) && FG_ALIGNED16(y) && FG_ALIGNED16(gate) && FG_ALIGNED16(x_out) && FG_ALIGNED16(p0) &&
                     FG_ALIGNED16(p1) && (((uintptr_t)norm_fp8) & 7) == 0 && mod_ld % 8 == 0 && fp8_max > 0.f,
                 "fg_residual_ln_fp8_bf16: pointers / mod_ld must be 16-byte aligned (norm_fp8: 8), fp8_max positive");
    if (rows == 0) return FG_OK;
    if (!need_mod) { mod_rows = 1; first_rows = 0; }
    if (mode == 0)
        hipLaunchKernelGGL(residual_kernel<0>, row_grid(rows), dim3(256), 0, (hipStream_t)stream, (const bf16*)x,
                           (const bf16*)y, (const bf16*)gate, (bf16*)x_out, (const bf16*)p0, (const bf16*)p1,
                           (bf16*)nullptr, rows, C, eps, mod_rows, first_rows, mod_ld, (uint8_t*)norm_fp8, norm_scale, fp8_max);
    else
        hipLaunchKernelGGL(residual_kernel<1>, row_grid(rows), dim3(256), 0, (hipStream_t)stream, (const bf16*)x,
                           (const bf16*)y, (const bf16*)gate, (bf16*)x_out, (const bf16*)p0, (const bf16*)p1,
                           (bf16*)nullptr, rows, C, eps, mod_rows, first_rows, mod_ld, (uint8_t*)norm_fp8, norm_scale, fp8_max);
    return fg_launch_status("fg_residual_ln_fp8_bf16");
}

int fg_ln_affine_bf16(const void* x, const void* w, const void* b, void* out, int64_t rows, int C, float eps,
                      fg_stream_t stream) {
    if (int e = check_rows("fg_ln_affine_bf16", rows, C, 1, 0)) return e;
    FG_CHECK_ARG(x && w && b && out, "fg_ln_affine_bf16: null pointer");
    FG_CHECK_ARG(FG_ALIGNED16(x) && FG_ALIGNED16(w) && FG_ALIGNED16(b) && FG_ALIGNED16(out),
                 "fg_ln_affine_bf16: pointers must be 16-byte aligned");
    if (rows == 0) return FG_OK;
    hipLaunchKernelGGL(ln_affine_kernel, row_grid(rows), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, (const bf16*)w,
                       (const bf16*)b, (bf16*)out, rows, C, eps);
    return fg_launch_status("fg_ln_affine_bf16");
}

int fg_gate_residual_bf16(const void* x, const void* y, const void* gate, void* out, int64_t rows, int C, int64_t mod_rows,
                          int64_t first_rows, int64_t mod_ld, fg_stream_t stream) {
    if (int e = check_rows("fg_gate_residual_bf16", rows, C, gate ? mod_rows : 1, gate ? first_rows : 0)) return e;
    FG_CHECK_ARG(x && y && out, "fg_gate_residual_bf16: null pointer");
    FG_CHECK_ARG(FG_ALIGNED16(x) && FG_ALIGNED16(y) && FG_ALIGNED16(gate) && FG_ALIGNED16(out) && mod_ld % 8 == 0,
                 "fg_gate_residual_bf16: pointers / mod_ld must be 16-byte aligned");
    if (rows == 0) return FG_OK;
    hipLaunchKernelGGL(residual_kernel<-1>, row_grid(rows), dim3(256), 0, (hipStream_t)stream, (const bf16*)x,
                       (const bf16*)y, (const bf16*)gate, (bf16*)out, (const bf16*)nullptr, (const bf16*)nullptr,
                       (bf16*)nullptr, rows, C, 0.f, gate ? mod_rows : 1, gate ? first_rows : 0, mod_ld);
    return fg_launch_status("fg_gate_residual_bf16");
}

int fg_residual_ln_bf16(const void* x, const void* y, const void* gate, void* x_out, const void* p0, const void* p1,
                        void* norm_out, int mode, int64_t rows, int C, float eps, int64_t mod_rows, int64_t first_rows,
                        int64_t mod_ld, fg_stream_t stream) {
    FG_CHECK_ARG(mode == 0 || mode == 1, "fg_residual_ln_bf16: mode must be 0 (modulate) or 1 (affine)");
    const bool need_mod = gate != nullptr || mode == 0;
    if (int e = check_rows("fg_residual_ln_bf16", rows, C, need_mod ? mod_rows : 1, need_mod ? first_rows : 0)) return e;
    FG_CHECK_ARG(x && y && x_out && p0 && p1 && norm_out, "fg_residual_ln_bf16: null pointer");
    FG_CHECK_ARG(FG_ALIGNED16(x) && FG_ALIGNED16(y) && FG_ALIGNED16(gate) && FG_ALIGNED16(x_out) && FG_ALIGNED16(p0) &&
                     FG_ALIGNED16(p1) && FG_ALIGNED16(norm_out) && mod_ld % 8 == 0,
                 "fg_residual_ln_bf16: pointers / mod_ld must be 16-byte aligned");
    if (rows == 0) return FG_OK;
    if (!need_mod) { mod_rows = 1; first_rows = 0; }
    if (mode == 0)
        hipLaunchKernelGGL(residual_kernel<0>, row_grid(rows), dim3(256), 0, (hipStream_t)stream, (const bf16*)x,
                           (const bf16*)y, (const bf16*)gate, (bf16*)x_out, (const bf16*)p0, (const bf16*)p1,
                           (bf16*)norm_out, rows, C, eps, mod_rows, first_rows, mod_ld);
    else
        hipLaunchKernelGGL(residual_kernel<1>, row_grid(rows), dim3(256), 0, (hipStream_t)stream, (const bf16*)x,
                           (const bf16*)y, (const bf16*)gate, (bf16*)x_out, (const bf16*)p0, (const bf16*)p1,
                           (bf16*)norm_out, rows, C, eps, mod_rows, first_rows, mod_ld);
    return fg_launch_status("fg_residual_ln_bf16");
}

int fg_rmsnorm_rope_bf16(const void* x, int64_t ldx, const void* weight, const void* cos_tab, const void* sin_tab,
                         int table_f32, void* out, int64_t rows, int C, int num_heads, float eps, fg_stream_t stream) {
    if (int e = check_rows("fg_rmsnorm_rope_bf16", rows, C, 1, 0)) return e;
    FG_CHECK_ARG(x && weight && out, "fg_rmsnorm_rope_bf16: null pointer");
    FG_CHECK_ARG(table_f32 ? (cos_tab != nullptr && sin_tab == nullptr) : ((cos_tab == nullptr) == (sin_tab == nullptr)),
                 "fg_rmsnorm_rope_bf16: fp64 mode takes both tables or neither, fp32 mode ONE interleaved table in cos_tab");
    FG_CHECK_ARG(num_heads > 0 && C % num_heads == 0 && (C / num_heads) % 8 == 0,
                 "fg_rmsnorm_rope_bf16: head_dim must be a multiple of 8");
    FG_CHECK_ARG(ldx >= C && ldx % 8 == 0 && FG_ALIGNED16(x) && FG_ALIGNED16(weight) && FG_ALIGNED16(out) &&
                     FG_ALIGNED16(cos_tab) && FG_ALIGNED16(sin_tab),
                 "fg_rmsnorm_rope_bf16: pointers / ldx must be 16-byte aligned");
    if (rows == 0) return FG_OK;
    const int hd = C / num_heads;
    const bool plain = (hd & (hd - 1)) == 0;          // plain rows + power-of-two head_dim: the division-free instantiation
#define FG_ROPE_LAUNCH(TAB, PL)                                                                                                  \
    hipLaunchKernelGGL((rmsnorm_rope_kernel<TAB, PL>), row_grid(rows), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, ldx,    \
                       (const bf16*)weight, cos_tab, sin_tab, (bf16*)out, rows, C, hd, eps, C, (int64_t)0, (int64_t)C)
    if (table_f32) { if (plain) FG_ROPE_LAUNCH(true, true); else FG_ROPE_LAUNCH(true, false); }
    else { if (plain) FG_ROPE_LAUNCH(false, true); else FG_ROPE_LAUNCH(false, false); }
#undef FG_ROPE_LAUNCH
    return fg_launch_status("fg_rmsnorm_rope_bf16");
}

int fg_rmsnorm_rope_grouped_bf16(const void* x, int64_t ldx, const void* weight, const void* cos_tab,
                                 const void* sin_tab, int table_f32, void* out, int64_t rows, int C, int num_heads, float eps,
                                 int group_cols, int64_t out_group_stride, int64_t out_ld, fg_stream_t stream) {
    if (int e = check_rows("fg_rmsnorm_rope_grouped_bf16", rows, C, 1, 0)) return e;
    FG_CHECK_ARG(x && weight && out, "fg_rmsnorm_rope_grouped_bf16: null pointer");
    FG_CHECK_ARG(table_f32 ? (cos_tab != nullptr && sin_tab == nullptr) : ((cos_tab == nullptr) == (sin_tab == nullptr)),
                 "fg_rmsnorm_rope_grouped_bf16: fp64 mode takes both tables or neither, fp32 mode ONE interleaved table in cos_tab");
    FG_CHECK_ARG(num_heads > 0 && C % num_heads == 0 && (C / num_heads) % 8 == 0,
                 "fg_rmsnorm_rope_grouped_bf16: head_dim must be a multiple of 8");
    FG_CHECK_ARG(group_cols > 0 && group_cols % 8 == 0 && C % group_cols == 0 && out_ld >= group_cols && out_ld % 8 == 0 &&
                     out_group_stride % 8 == 0 && out_group_stride >= 0,
                 "fg_rmsnorm_rope_grouped_bf16: group_cols must divide C; group_cols, out_ld, out_group_stride multiples of 8");
    FG_CHECK_ARG(ldx >= C && ldx % 8 == 0 && FG_ALIGNED16(x) && FG_ALIGNED16(weight) && FG_ALIGNED16(out) &&
                     FG_ALIGNED16(cos_tab) && FG_ALIGNED16(sin_tab),
                 "fg_rmsnorm_rope_grouped_bf16: pointers / ldx must be 16-byte aligned");
    if (rows == 0) return FG_OK;
    if (table_f32)
        hipLaunchKernelGGL((rmsnorm_rope_kernel<true, false>), row_grid(rows), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, ldx,
                           (const bf16*)weight, cos_tab, sin_tab, (bf16*)out, rows, C, C / num_heads, eps, group_cols,
                           out_group_stride, out_ld);
    else
        hipLaunchKernelGGL((rmsnorm_rope_kernel<false, false>), row_grid(rows), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, ldx,
                           (const bf16*)weight, cos_tab, sin_tab, (bf16*)out, rows, C, C / num_heads, eps, group_cols,
                           out_group_stride, out_ld);
    return fg_launch_status("fg_rmsnorm_rope_grouped_bf16");
}

int fg_copy_groups_bf16(const void* src, int64_t src_group_stride, int64_t src_ld, void* dst, int64_t dst_group_stride,
                        int64_t dst_ld, int groups, int64_t rows, int cols, fg_stream_t stream) {
    FG_CHECK_ARG(src && dst, "fg_copy_groups_bf16: null pointer");
    FG_CHECK_ARG(groups > 0 && rows >= 0 && cols > 0 && cols % 8 == 0, "fg_copy_groups_bf16: cols must be a positive multiple of 8");
    FG_CHECK_ARG(src_group_stride % 8 == 0 && src_ld % 8 == 0 && dst_group_stride % 8 == 0 && dst_ld % 8 == 0 &&
                     src_ld >= cols && dst_ld >= cols && FG_ALIGNED16(src) && FG_ALIGNED16(dst),
                 "fg_copy_groups_bf16: strides must be multiples of 8 elements, rows at least cols wide, pointers 16-byte aligned");
    if (rows == 0) return FG_OK;
    const int64_t total = (int64_t)groups * rows * (cols / 8);
    const unsigned grid = (unsigned)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    hipLaunchKernelGGL(copy_groups_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16*)src, src_group_stride,
                       src_ld, (bf16*)dst, dst_group_stride, dst_ld, groups, rows, cols / 8);
    return fg_launch_status("fg_copy_groups_bf16");
}

int fg_act_bf16(const void* x, void* out, int64_t n, int kind, fg_stream_t stream) {
    FG_CHECK_ARG(x && out && n >= 0 && n % 8 == 0, "fg_act_bf16: n must be a multiple of 8");
    FG_CHECK_ARG(kind == 0 || kind == 1, "fg_act_bf16: kind must be 0 (silu) or 1 (gelu_tanh)");
    FG_CHECK_ARG(FG_ALIGNED16(x) && FG_ALIGNED16(out), "fg_act_bf16: pointers must be 16-byte aligned");
    if (n == 0) return FG_OK;
    const int64_t nvec = n / 8;
    const unsigned grid = (unsigned)((nvec + 255) / 256 < 8192 ? (nvec + 255) / 256 : 8192);
    if (kind == 0)
        hipLaunchKernelGGL(act_kernel<0>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, (bf16*)out, nvec);
    else
        hipLaunchKernelGGL(act_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, (bf16*)out, nvec);
    return fg_launch_status("fg_act_bf16");
}

int fg_cfg_euler_bf16(const void* latents, const void* posi, const void* nega, void* out, int64_t n, float cfg_scale,
                      float dsigma, fg_stream_t stream) {
    FG_CHECK_ARG(latents && posi && out && n >= 0, "fg_cfg_euler_bf16: null pointer");
    if (n == 0) return FG_OK;
    const unsigned grid = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(cfg_euler_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16*)latents,
                       (const bf16*)posi, (const bf16*)nega, (bf16*)out, n, cfg_scale, dsigma);
    return fg_launch_status("fg_cfg_euler_bf16");
}

int fg_cfg_euler_dev_bf16(const void* latents, const void* posi, const void* nega, void* out, int64_t n, float cfg_scale,
                          const float* dsigma_table, const int* step, const void* first, int64_t first_n, int64_t frame_stride,
                          fg_stream_t stream) {
    FG_CHECK_ARG(latents && posi && out && dsigma_table && step && n >= 0, "fg_cfg_euler_dev_bf16: null pointer");
    FG_CHECK_ARG((((uintptr_t)dsigma_table) & 3) == 0 && (((uintptr_t)step) & 3) == 0, "fg_cfg_euler_dev_bf16: dsigma_table / step must be 4-byte aligned");
    FG_CHECK_ARG(first == nullptr || (first_n > 0 && frame_stride >= first_n && n % frame_stride == 0),
                 "fg_cfg_euler_dev_bf16: with `first`, need 0 < first_n <= frame_stride and n a multiple of frame_stride (got n=%lld first_n=%lld "
                 "frame_stride=%lld)", (long long)n, (long long)first_n, (long long)frame_stride);
    if (n == 0) return FG_OK;
    const bool vec = FG_ALIGNED16(latents) && FG_ALIGNED16(posi) && FG_ALIGNED16(out) && (nega == nullptr || FG_ALIGNED16(nega));
    const int64_t nvec = vec ? n / 8 : 0;
    const int64_t work = nvec > n - nvec * 8 ? nvec : n - nvec * 8;
    const unsigned grid = (unsigned)((work + 255) / 256 < 4096 ? (work + 255) / 256 : 4096);
    hipLaunchKernelGGL(cfg_euler_dev_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16*)latents, (const bf16*)posi,
                       (const bf16*)nega, (bf16*)out, n, nvec, cfg_scale, dsigma_table, step, (const bf16*)first, first_n, frame_stride);
    return fg_launch_status("fg_cfg_euler_dev_bf16");
}

// ---- include/fairygen_hip_rowbatch.h: the row kernels that read a per-row table, on B elements of `rows` rows each.  The checks are
// those of the single-element entry point on ONE element (rows, mod_rows, first_rows count inside the element), then B.
int fg_dit_rowbatch_version(void) { return 1; }

int fg_ln_modulate_bf16_b(const void* x, const void* shift, const void* scale, void* out, int B, int64_t rows, int C, float eps,
                          int64_t mod_rows, int64_t first_rows, int64_t mod_ld, fg_stream_t stream) {
    if (int e = check_rows("fg_ln_modulate_bf16_b", rows, C, mod_rows, first_rows)) return e;
    if (int e = check_batch("fg_ln_modulate_bf16_b", B)) return e;
    FG_CHECK_ARG(x && shift && scale && out, "fg_ln_modulate_bf16_b: null pointer");
    FG_CHECK_ARG(FG_ALIGNED16(x) && FG_ALIGNED16(shift) && FG_ALIGNED16(scale) && FG_ALIGNED16(out) && mod_ld % 8 == 0,
                 "fg_ln_modulate_bf16_b: pointers / mod_ld must be 16-byte aligned");
    if (rows == 0) return FG_OK;
    hipLaunchKernelGGL(ln_modulate_b_kernel, row_grid_b(rows, B), dim3(256), 0, (hipStream_t)stream, (const bf16*)x,
                       (const bf16*)shift, (const bf16*)scale, (bf16*)out, rows, C, eps, mod_rows, first_rows, mod_ld);
    return fg_launch_status("fg_ln_modulate_bf16_b");
}

int fg_gate_residual_bf16_b(const void* x, const void* y, const void* gate, void* out, int B, int64_t rows, int C, int64_t mod_rows,
                            int64_t first_rows, int64_t mod_ld, fg_stream_t stream) {
    if (int e = check_rows("fg_gate_residual_bf16_b", rows, C, gate ? mod_rows : 1, gate ? first_rows : 0)) return e;
    if (int e = check_batch("fg_gate_residual_bf16_b", B)) return e;
    FG_CHECK_ARG(x && y && out, "fg_gate_residual_bf16_b: null pointer");
    FG_CHECK_ARG(FG_ALIGNED16(x) && FG_ALIGNED16(y) && FG_ALIGNED16(gate) && FG_ALIGNED16(out) && mod_ld % 8 == 0,
                 "fg_gate_residual_bf16_b: pointers / mod_ld must be 16-byte aligned");
    if (rows == 0) return FG_OK;
    hipLaunchKernelGGL(residual_b_kernel<-1>, row_grid_b(rows, B), dim3(256), 0, (hipStream_t)stream, (const bf16*)x,
                       (const bf16*)y, (const bf16*)gate, (bf16*)out, (const bf16*)nullptr, (const bf16*)nullptr,
                       (bf16*)nullptr, rows, C, 0.f, gate ? mod_rows : 1, gate ? first_rows : 0, mod_ld);
    return fg_launch_status("fg_gate_residual_bf16_b");
}

int fg_residual_ln_bf16_b(const void* x, const void* y, const void* gate, void* x_out, const void* p0, const void* p1,
                          void* norm_out, int mode, int B, int64_t rows, int C, float eps, int64_t mod_rows, int64_t first_rows,
                          int64_t mod_ld, fg_stream_t stream) {
    FG_CHECK_ARG(mode == 0 || mode == 1, "fg_residual_ln_bf16_b: mode must be 0 (modulate) or 1 (affine)");
    const bool need_mod = gate != nullptr || mode == 0;
    if (int e = check_rows("fg_residual_ln_bf16_b", rows, C, need_mod ? mod_rows : 1, need_mod ? first_rows : 0)) return e;
    if (int e = check_batch("fg_residual_ln_bf16_b", B)) return e;
    FG_CHECK_ARG(x && y && x_out && p0 && p1 && norm_out, "fg_residual_ln_bf16_b: null pointer");
    FG_CHECK_ARG(FG_ALIGNED16(x) && FG_ALIGNED16(y) && FG_ALIGNED16(gate) && FG_ALIGNED16(x_out) && FG_ALIGNED16(p0) &&
                     FG_ALIGNED16(p1) && FG_ALIGNED16(norm_out) && mod_ld % 8 == 0,
                 "fg_residual_ln_bf16_b: pointers / mod_ld must be 16-byte aligned");
    if (rows == 0) return FG_OK;
    if (!need_mod) { mod_rows = 1; first_rows = 0; }
    if (mode == 0)
        hipLaunchKernelGGL(residual_b_kernel<0>, row_grid_b(rows, B), dim3(256), 0, (hipStream_t)stream, (const bf16*)x,
                           (const bf16*)y, (const bf16*)gate, (bf16*)x_out, (const bf16*)p0, (const bf16*)p1,
                           (bf16*)norm_out, rows, C, eps, mod_rows, first_rows, mod_ld);
    else
        hipLaunchKernelGGL(residual_b_kernel<1>, row_grid_b(rows, B), dim3(256), 0, (hipStream_t)stream, (const bf16*)x,
                           (const bf16*)y, (const bf16*)gate, (bf16*)x_out, (const bf16*)p0, (const bf16*)p1,
                           (bf16*)norm_out, rows, C, eps, mod_rows, first_rows, mod_ld);
    return fg_launch_status("fg_residual_ln_bf16_b");
}

int fg_rmsnorm_rope_bf16_b(const void* x, int64_t ldx, const void* weight, const void* cos_tab, const void* sin_tab,
                           int table_f32, void* out, int B, int64_t rows, int C, int num_heads, float eps, fg_stream_t stream) {
    if (int e = check_rows("fg_rmsnorm_rope_bf16_b", rows, C, 1, 0)) return e;
    if (int e = check_batch("fg_rmsnorm_rope_bf16_b", B)) return e;
    FG_CHECK_ARG(x && weight && out, "fg_rmsnorm_rope_bf16_b: null pointer");
    FG_CHECK_ARG(table_f32 ? (cos_tab != nullptr && sin_tab == nullptr) : ((cos_tab == nullptr) == (sin_tab == nullptr)),
                 "fg_rmsnorm_rope_bf16_b: fp64 mode takes both tables or neither, fp32 mode ONE interleaved table in cos_tab");
    FG_CHECK_ARG(num_heads > 0 && C % num_heads == 0 && (C / num_heads) % 8 == 0,
                 "fg_rmsnorm_rope_bf16_b: head_dim must be a multiple of 8");
    FG_CHECK_ARG(ldx >= C && ldx % 8 == 0 && FG_ALIGNED16(x) && FG_ALIGNED16(weight) && FG_ALIGNED16(out) &&
                     FG_ALIGNED16(cos_tab) && FG_ALIGNED16(sin_tab),
                 "fg_rmsnorm_rope_bf16_b: pointers / ldx must be 16-byte aligned");
    if (rows == 0) return FG_OK;
    const int hd = C / num_heads;
    const bool plain = (hd & (hd - 1)) == 0;          // as fg_rmsnorm_rope_bf16 picks its instantiation
#define FG_ROPE_B_LAUNCH(TAB, PL)                                                                                                    \
    hipLaunchKernelGGL((rmsnorm_rope_b_kernel<TAB, PL>), row_grid_b(rows, B), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, ldx, \
                       (const bf16*)weight, cos_tab, sin_tab, (bf16*)out, rows, C, hd, eps)
    if (table_f32) { if (plain) FG_ROPE_B_LAUNCH(true, true); else FG_ROPE_B_LAUNCH(true, false); }
    else { if (plain) FG_ROPE_B_LAUNCH(false, true); else FG_ROPE_B_LAUNCH(false, false); }
#undef FG_ROPE_B_LAUNCH
    return fg_launch_status("fg_rmsnorm_rope_bf16_b");
}

// ---- include/fairygen_hip_rowbatch8.h: the norms with the fp8 output on B elements of `rows` rows each; checks as above.
int fg_dit_rowbatch8_version(void) { return 1; }

int fg_ln_modulate_fp8_bf16_b(const void* x, const void* shift, const void* scale, void* out_fp8, float* out_scale, int B, int64_t rows,
                              int C, float eps, int64_t mod_rows, int64_t first_rows, int64_t mod_ld, float fp8_max, fg_stream_t stream) {
    if (int e = check_rows("fg_ln_modulate_fp8_bf16_b", rows, C, mod_rows, first_rows)) return e;
    if (int e = check_batch("fg_ln_modulate_fp8_bf16_b", B)) return e;
    FG_CHECK_ARG(x && shift && scale && out_fp8 && out_scale, "fg_ln_modulate_fp8_bf16_b: null pointer");
    FG_CHECK_ARG(FG_ALIGNED16(x) && FG_ALIGNED16(shift) && FG_ALIGNED16(scale) && (((uintptr_t)out_fp8) & 7) == 0 && mod_ld % 8 == 0 &&
                     fp8_max > 0.f,
                 "fg_ln_modulate_fp8_bf16_b: pointers / mod_ld must be 16-byte aligned (out_fp8: 8), fp8_max positive");
    if (rows == 0) return FG_OK;
    hipLaunchKernelGGL(ln_modulate_fp8_b_kernel, row_grid_b(rows, B), dim3(256), 0, (hipStream_t)stream, (const bf16*)x,
                       (const bf16*)shift, (const bf16*)scale, (uint8_t*)out_fp8, out_scale, rows, C, eps, mod_rows, first_rows, mod_ld,
                       fp8_max);
    return fg_launch_status("fg_ln_modulate_fp8_bf16_b");
}

int fg_residual_ln_fp8_bf16_b(const void* x, const void* y, const void* gate, void* x_out, const void* p0, const void* p1,
                              void* norm_fp8, float* norm_scale, int mode, int B, int64_t rows, int C, float eps, int64_t mod_rows,
                              int64_t first_rows, int64_t mod_ld, float fp8_max, fg_stream_t stream) {
    FG_CHECK_ARG(mode == 0 || mode == 1, "fg_residual_ln_fp8_bf16_b: mode must be 0 (modulate) or 1 (affine)");
    const bool need_mod = gate != nullptr || mode == 0;
    if (int e = check_rows("fg_residual_ln_fp8_bf16_b", rows, C, need_mod ? mod_rows : 1, need_mod ? first_rows : 0)) return e;
    if (int e = check_batch("fg_residual_ln_fp8_bf16_b", B)) return e;
    FG_CHECK_ARG(x && y && x_out && p0 && p1 && norm_fp8 && norm_scale, "fg_residual_ln_fp8_bf16_b: null pointer");
    FG_CHECK_ARG(FG_ALIGNED16(x) && FG_ALIGNED16(y) && FG_ALIGNED16(gate) && FG_ALIGNED16(x_out) && FG_ALIGNED16(p0) &&
                     FG_ALIGNED16(p1) && (((uintptr_t)norm_fp8) & 7) == 0 && mod_ld % 8 == 0 && fp8_max > 0.f,
                 "fg_residual_ln_fp8_bf16_b: pointers / mod_ld must be 16-byte aligned (norm_fp8: 8), fp8_max positive");
    if (rows == 0) return FG_OK;
    if (!need_mod) { mod_rows = 1; first_rows = 0; }
    if (mode == 0)
        hipLaunchKernelGGL(residual_fp8_b_kernel<0>, row_grid_b(rows, B), dim3(256), 0, (hipStream_t)stream, (const bf16*)x,
                           (const bf16*)y, (const bf16*)gate, (bf16*)x_out, (const bf16*)p0, (const bf16*)p1, (uint8_t*)norm_fp8,
                           norm_scale, rows, C, eps, mod_rows, first_rows, mod_ld, fp8_max);
    else
        hipLaunchKernelGGL(residual_fp8_b_kernel<1>, row_grid_b(rows, B), dim3(256), 0, (hipStream_t)stream, (const bf16*)x,
                           (const bf16*)y, (const bf16*)gate, (bf16*)x_out, (const bf16*)p0, (const bf16*)p1, (uint8_t*)norm_fp8,
                           norm_scale, rows, C, eps, mod_rows, first_rows, mod_ld, fp8_max);
    return fg_launch_status("fg_residual_ln_fp8_bf16_b");
}

// ---- include/fairygen_hip_lorabatch.h: the two-output modulate norm on B elements of `rows` rows each (its version query is next to
// fg_lora_apply_bf16_b, lora.hip); checks as above.
int fg_ln_modulate_dual_bf16_b(const void* x, const void* shift, const void* scale, void* out, void* out_fp8, float* out_scale, int B,
                               int64_t rows, int C, float eps, int64_t mod_rows, int64_t first_rows, int64_t mod_ld, float fp8_max,
                               fg_stream_t stream) {
    if (int e = check_rows("fg_ln_modulate_dual_bf16_b", rows, C, mod_rows, first_rows)) return e;
    if (int e = check_batch("fg_ln_modulate_dual_bf16_b", B)) return e;
    FG_CHECK_ARG(x && shift && scale && out && out_fp8 && out_scale, "fg_ln_modulate_dual_bf16_b: null pointer");
    FG_CHECK_ARG(FG_ALIGNED16(x) && FG_ALIGNED16(shift) && FG_ALIGNED16(scale) && FG_ALIGNED16(out) && (((uintptr_t)out_fp8) & 7) == 0 &&
                     mod_ld % 8 == 0 && fp8_max > 0.f,
                 "fg_ln_modulate_dual_bf16_b: pointers / mod_ld must be 16-byte aligned (out_fp8: 8), fp8_max positive");
    if (rows == 0) return FG_OK;
    hipLaunchKernelGGL(ln_dual_b_kernel<0>, row_grid_b(rows, B), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, (const bf16*)shift,
                       (const bf16*)scale, (bf16*)out, (uint8_t*)out_fp8, out_scale, rows, C, eps, mod_rows, first_rows, mod_ld, fp8_max);
    return fg_launch_status("fg_ln_modulate_dual_bf16_b");
}

}  // extern "C"
