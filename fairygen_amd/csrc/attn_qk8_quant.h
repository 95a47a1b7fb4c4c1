// The e4m3 conversion of the 8-bit Q K^T operands, shared by the stand-alone quantise pass (attn_qk8.hip) and the producers fused into
// the RMSNorm+RoPE pass (attn_qk8_fused.hip): one division and one conversion, so both write the same bytes.
#pragma once
#include "common.h"

namespace {

constexpr int kD = 128;
constexpr float kE4M3Max = 448.0f;
constexpr float kScaleFloor = 0x1p-20f;

__device__ __forceinline__ uint32_t cvt2_e4m3(float a, float b) {      // v_cvt_pk_fp8_f32: RNE, OCP e4m3fn on gfx950
    a = fminf(fmaxf(a, -kE4M3Max), kE4M3Max);
    b = fminf(fmaxf(b, -kE4M3Max), kE4M3Max);
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false) & 0xffffu;
}

// 8 values / s -> 8 e4m3 bytes
__device__ __forceinline__ u32x2 quant8_e4m3(const float* f, float s) {
    u32x2 w;
    w[0] = cvt2_e4m3(f[0] / s, f[1] / s) | (cvt2_e4m3(f[2] / s, f[3] / s) << 16);
    w[1] = cvt2_e4m3(f[4] / s, f[5] / s) | (cvt2_e4m3(f[6] / s, f[7] / s) << 16);
    return w;
}

}  // namespace
