// Cross-attention with both matrix products on the e4m3 MFMA and one head's K8 and V8^T resident in LDS (fg_attn_fwd_cross8_bf16,
// include/fairygen_hip_cross8.h), for gfx950.
//
// The operands and the arithmetic are those of fg_attn_fwd_pv8_bf16 (attention.hip, the QK8 + PV8 form of the 8-wave template; DESIGN §5
// "e4m3 P V"): q8 / sq, k8 / sk with the key mean removed, v8t in the tile order of attn_pv8_parts.h with zero padding, sv; S^T = K8 Q8^T
// and O^T += V8^T P8^T on v_mfma_f32_32x32x64_f8f6f4, P8 = e4m3(c p) with c = 2^5 under a deferred rescale of T = 3 bits, 64-key tiles in
// ascending order, the ragged last tile masked (P8 = 0), out = acc sv / l.  A wave owns 32 query rows of a 256-row block exactly as there
// (the deferred rescale is decided per wave), and every expression a row goes through is written as it is there, so the output is bit for
// bit that of fg_attn_fwd_pv8_bf16 launched without a workspace (tests/test_attention_cross8.py holds it to that, with torch.equal).
//
// What differs is where K and V come from.  At e4m3 a key is 128 B of K8 and 128 B of V8^T per head, so the Nkv <= 640 keys of a text
// context fit the 160 KiB of LDS a workgroup may declare.  H x G workgroups of 8 waves, G = min(ceil(Nq / 256), max(1, CUs / H)):
//   * workgroup (h, g) copies head h's K8 tiles and V8^T tiles into LDS once (the tile images and swizzles of the 8-wave template: K8 rows
//     of 128 B with the 16-byte chunk XORed by row & 7, V8^T channel rows of 64 B with the chunk XORed by (row >> 2) & 3, both conflict-free
//     for the 16-lane groups of ds_read_b128); key rows >= Nkv are written as zeros;
//   * ONE barrier; then it walks the query blocks g, g + G, g + 2 G, .. of 256 rows (the last may be ragged), each wave on its own: no
//     ring, no per-tile load, no further barrier, nothing waits on another workgroup and there are no atomics;
//   * per tile and wave the step of the template: the 4 MFMAs of S^T(t+1) under the exponentials of tile t, then the 4 of O^T(t).
// LDS: 256 * Nkp bytes (Nkp = Nkv rounded up to whole tiles) and nothing else: P stays in registers.
//
// The smoothed-V forms (fg_attn_fwd_cross8s_bf16 / _b, include/fairygen_hip_cross8s.h; DESIGN §5 "e4m3 cross-attention with smoothed V")
// compile the same body with SMV: v8t / sv are those of fg_attn_quant_vt_smooth_bf16 (v minus its key mean), and the epilogue adds the mean
// mu (H, 128) back in fp32 before the one rounding to bf16, as attn_fwd_pv8s_kernel does, whose bits they give.  mu is read from global
// memory there: at 640 keys the tiles fill the LDS.
#include "common.h"
#include "../../include/fairygen_hip_cross8.h"
#include "../../include/fairygen_hip_batch8.h"
#include "../../include/fairygen_hip_cross8s.h"
#include "attn_qk8_quant.h"
#include "attn_pv8_parts.h"
#include <math.h>
#include <type_traits>

namespace {

constexpr int kBM = 256;                              // query rows per block: 8 waves x 32 rows
constexpr int kTile8Bytes = kTileKeys * kD;           // 8 KiB: an e4m3 K tile, or an e4m3 V^T tile
constexpr int kLdsBudget = 160 * 1024;                // what one workgroup may declare on gfx950
constexpr int kMaxKv = kLdsBudget / (2 * kTile8Bytes) * kTileKeys;      // 640 keys: K8 + V8^T of a head, nothing besides
static_assert(kMaxKv >= 512 && kMaxKv % kTileKeys == 0, "the text context of the DiT (512 keys) must fit");
// P8 = e4m3(c p) with p <= 2^T, c = 2^5 and T = 3 (include/fairygen_hip_pv8.h)
constexpr float kPv8DeferLog2 = 3.0f;
constexpr float kPv8Log2C = 5.0f;

typedef __attribute__((ext_vector_type(8))) int i32x8;

// the tile images of attention.hip's e4m3 forms
__device__ __forceinline__ int k8_lds_off(int row, int chunk) { return row * 128 + ((chunk ^ (row & 7)) << 4); }
__device__ __forceinline__ int v8_lds_off(int row, int chunk) { return row * 64 + ((chunk ^ ((row >> 2) & 3)) << 4); }

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float max3(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float add_f32(float a, float b) {
    float r;
    asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// max / sum across the lane pair (l, l^32) that shares a query row
__device__ __forceinline__ float pair_max(float x) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float pair_sum(float x) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}
// all 32 exponentials of a tile under the 16 QK gaps, two a gap
__host__ __device__ constexpr int exps_before(int g) { return 2 * g < 32 ? 2 * g : 32; }

struct Cross8Params {
    const uint8_t* q8; const uint8_t* k8; const float* sq; const float* sk; const uint8_t* v8t; const float* sv;
    bf16* out;
    int64_t Nq, Nkv, Nkp;
    int H, G, nqb;
    float scale_log2e;
};

// Workgroup h * G + g: head h, query blocks g, g + G, ..  Lane (r, hh) of wave w owns query row 256 qb + 32 w + r of its block, as in
// attn_fwd_kernel<true, true>; the operand maps of the two MFMAs are described there.
// (the body is one text for this form and the smoothed-V form; FG_CROSS8_NO_SMV names what only the other form reads)
#define FG_CROSS8_NO_SMV            \
    constexpr bool SMV = false;     \
    const float* const mu = nullptr
__global__ __launch_bounds__(512, 2) void attn_cross8_kernel(const Cross8Params P) {
    FG_CROSS8_NO_SMV;
#include "attn_cross8_body.inc"
}

// fg_attn_fwd_cross8s_bf16: attn_cross8_kernel with the key mean of V added in the epilogue; mu is an argument of its own, so that
// Cross8Params and the kernels that take it stay what they are.
__global__ __launch_bounds__(512, 2) void attn_cross8s_kernel(const Cross8Params P, const float* __restrict__ mu) {
    constexpr bool SMV = true;
#include "attn_cross8_body.inc"
}

// The batched form (fg_attn_fwd_cross8_bf16_b, include/fairygen_hip_batch8.h): workgroup (h * G + g, b) is workgroup h * G + g of the
// single-element kernel on element b's operands — one head's K8 and V8^T of ONE element in LDS.  Strides: bytes for the e4m3 operands,
// floats for the scales, bf16 elements for out.
struct Cross8ParamsB {
    Cross8Params p;
    int64_t bs_q8, bs_k8, bs_sq, bs_sk, bs_v8t, bs_sv, bs_out;
};

__global__ __launch_bounds__(512, 2) void attn_cross8_b_kernel(const Cross8ParamsB PB) {
    const int64_t b = blockIdx.y;
    Cross8Params Pe = PB.p;
    Pe.q8 += b * PB.bs_q8; Pe.k8 += b * PB.bs_k8; Pe.sq += b * PB.bs_sq; Pe.sk += b * PB.bs_sk;
    Pe.v8t += b * PB.bs_v8t; Pe.sv += b * PB.bs_sv; Pe.out += b * PB.bs_out;
    const Cross8Params P = Pe;
    FG_CROSS8_NO_SMV;
#include "attn_cross8_body.inc"
}
#undef FG_CROSS8_NO_SMV

// fg_attn_fwd_cross8s_bf16_b: bs_mu counts floats
__global__ __launch_bounds__(512, 2) void attn_cross8s_b_kernel(const Cross8ParamsB PB, const float* __restrict__ mu, int64_t bs_mu) {
    constexpr bool SMV = true;
    const int64_t b = blockIdx.y;
    Cross8Params Pe = PB.p;
    Pe.q8 += b * PB.bs_q8; Pe.k8 += b * PB.bs_k8; Pe.sq += b * PB.bs_sq; Pe.sk += b * PB.bs_sk;
    Pe.v8t += b * PB.bs_v8t; Pe.sv += b * PB.bs_sv; Pe.out += b * PB.bs_out;
    mu += b * bs_mu;
    const Cross8Params P = Pe;
#include "attn_cross8_body.inc"
}

int device_cus() {
    static thread_local int cached_dev = -1, cached_cus = 256;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (dev != cached_dev) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) cached_cus = n;
        cached_dev = dev;
    }
    return cached_cus;
}

}  // namespace

extern "C" int fg_attn_cross8_version(void) { return 1; }

extern "C" int64_t fg_attn_cross8_max_kv(void) { return kMaxKv; }

extern "C" int fg_attn_fwd_cross8_bf16(const void* q8, const void* k8, const float* sq, const float* sk, const void* v8t, const float* sv,
                                       void* out, int64_t Nq, int64_t Nkv, int H, int D, float scale, fg_stream_t stream) {
    FG_CHECK_ARG(q8 && k8 && sq && sk && v8t && sv && out, "fg_attn_fwd_cross8_bf16: null pointer");
    FG_CHECK_ARG(D == kD, "fg_attn_fwd_cross8_bf16: only head_dim 128 is supported (got %d)", D);
    FG_CHECK_ARG(H > 0 && Nq > 0, "fg_attn_fwd_cross8_bf16: H, Nq must be positive");
    FG_CHECK_ARG(Nkv >= 1 && Nkv <= kMaxKv, "fg_attn_fwd_cross8_bf16: Nkv must be in 1..%d, the keys whose K8 and V8^T fit the LDS (got %lld)",
                 kMaxKv, (long long)Nkv);
    FG_CHECK_ARG(scale > 0.f, "fg_attn_fwd_cross8_bf16: scale must be positive");
    const int64_t hd = (int64_t)H * D, nkp = (Nkv + kTileKeys - 1) / kTileKeys * kTileKeys, nqb = (Nq + kBM - 1) / kBM;
    FG_CHECK_ARG(FG_ALIGNED16(q8) && FG_ALIGNED16(k8) && FG_ALIGNED16(v8t) && FG_ALIGNED16(sv) && FG_ALIGNED16(out) &&
                     (((uintptr_t)sq | (uintptr_t)sk) & 3) == 0,
                 "fg_attn_fwd_cross8_bf16: pointers must be 16-byte aligned (sq, sk: 4)");
    FG_CHECK_ARG(Nq * hd * 2 < (1ll << 32), "fg_attn_fwd_cross8_bf16: O must span < 4 GiB");
    const int cus = device_cus();
    const int64_t per_head = cus / H > 1 ? cus / H : 1;
    const int64_t G = nqb < per_head ? nqb : per_head;      // a function of Nq, H and the device only
    FG_CHECK_ARG((int64_t)H * G < (1ll << 30), "fg_attn_fwd_cross8_bf16: grid too large");
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(attn_cross8_kernel),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget);
    FG_CHECK_ARG(attr == hipSuccess, "fg_attn_fwd_cross8_bf16: cannot reserve 160 KiB of LDS: %s", hipGetErrorString(attr));
    Cross8Params P{};
    P.q8 = (const uint8_t*)q8; P.k8 = (const uint8_t*)k8; P.sq = sq; P.sk = sk; P.v8t = (const uint8_t*)v8t; P.sv = sv;
    P.out = (bf16*)out;
    P.Nq = Nq; P.Nkv = Nkv; P.Nkp = nkp;
    P.H = H; P.G = (int)G; P.nqb = (int)nqb;
    P.scale_log2e = scale * 1.4426950408889634f;
    hipLaunchKernelGGL(attn_cross8_kernel, dim3((unsigned)(H * G)), dim3(512), (size_t)(2 * kD * nkp), (hipStream_t)stream, P);
    return fg_launch_status("fg_attn_fwd_cross8_bf16");
}

extern "C" int fg_attn_fwd_cross8_bf16_b(const void* q8, int64_t bs_q8, const void* k8, int64_t bs_k8, const float* sq, int64_t bs_sq,
                                         const float* sk, int64_t bs_sk, const void* v8t, int64_t bs_v8t, const float* sv, int64_t bs_sv,
                                         void* out, int64_t bs_out, int B, int64_t Nq, int64_t Nkv, int H, int D, float scale,
                                         fg_stream_t stream) {
    FG_CHECK_ARG(q8 && k8 && sq && sk && v8t && sv && out, "fg_attn_fwd_cross8_bf16_b: null pointer");
    FG_CHECK_ARG(D == kD, "fg_attn_fwd_cross8_bf16_b: only head_dim 128 is supported (got %d)", D);
    FG_CHECK_ARG(B >= 1 && B <= 65535, "fg_attn_fwd_cross8_bf16_b: B must be in 1..65535 (got %d)", B);
    FG_CHECK_ARG(H > 0 && Nq > 0, "fg_attn_fwd_cross8_bf16_b: H, Nq must be positive");
    FG_CHECK_ARG(Nkv >= 1 && Nkv <= kMaxKv, "fg_attn_fwd_cross8_bf16_b: Nkv must be in 1..%d, the keys whose K8 and V8^T fit the LDS (got %lld)",
                 kMaxKv, (long long)Nkv);
    FG_CHECK_ARG(scale > 0.f, "fg_attn_fwd_cross8_bf16_b: scale must be positive");
    const int64_t hd = (int64_t)H * D, nkp = (Nkv + kTileKeys - 1) / kTileKeys * kTileKeys, nqb = (Nq + kBM - 1) / kBM;
    FG_CHECK_ARG(FG_ALIGNED16(q8) && FG_ALIGNED16(k8) && FG_ALIGNED16(v8t) && FG_ALIGNED16(sv) && FG_ALIGNED16(out) &&
                     (((uintptr_t)sq | (uintptr_t)sk) & 3) == 0,
                 "fg_attn_fwd_cross8_bf16_b: pointers must be 16-byte aligned (sq, sk: 4)");
    FG_CHECK_ARG(bs_q8 >= Nq * hd && bs_k8 >= Nkv * hd && bs_sq >= Nq * H && bs_sk >= H && bs_v8t >= hd * nkp && bs_sv >= hd && bs_out >= Nq * hd,
                 "fg_attn_fwd_cross8_bf16_b: a batch stride is smaller than one element of its operand");
    FG_CHECK_ARG(bs_q8 % 16 == 0 && bs_k8 % 16 == 0 && bs_v8t % 16 == 0 && bs_sv % 4 == 0 && bs_out % 8 == 0,
                 "fg_attn_fwd_cross8_bf16_b: batch strides must keep the 16-byte alignment of q8, k8, v8t, sv and out");
    FG_CHECK_ARG(Nq * hd * 2 < (1ll << 32), "fg_attn_fwd_cross8_bf16_b: O of one batch element must span < 4 GiB");
    const int cus = device_cus();
    const int64_t per_head = cus / ((int64_t)B * H) > 1 ? cus / ((int64_t)B * H) : 1;
    const int64_t G = nqb < per_head ? nqb : per_head;      // a function of Nq, B, H and the device only
    FG_CHECK_ARG((int64_t)H * G < (1ll << 30), "fg_attn_fwd_cross8_bf16_b: grid too large");
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(attn_cross8_b_kernel),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget);
    FG_CHECK_ARG(attr == hipSuccess, "fg_attn_fwd_cross8_bf16_b: cannot reserve 160 KiB of LDS: %s", hipGetErrorString(attr));
    Cross8ParamsB PB{};
    Cross8Params& P = PB.p;
    P.q8 = (const uint8_t*)q8; P.k8 = (const uint8_t*)k8; P.sq = sq; P.sk = sk; P.v8t = (const uint8_t*)v8t; P.sv = sv;
    P.out = (bf16*)out;
    P.Nq = Nq; P.Nkv = Nkv; P.Nkp = nkp;
    P.H = H; P.G = (int)G; P.nqb = (int)nqb;
    P.scale_log2e = scale * 1.4426950408889634f;
    PB.bs_q8 = bs_q8; PB.bs_k8 = bs_k8; PB.bs_sq = bs_sq; PB.bs_sk = bs_sk; PB.bs_v8t = bs_v8t; PB.bs_sv = bs_sv; PB.bs_out = bs_out;
    hipLaunchKernelGGL(attn_cross8_b_kernel, dim3((unsigned)(H * G), (unsigned)B), dim3(512), (size_t)(2 * kD * nkp), (hipStream_t)stream, PB);
    return fg_launch_status("fg_attn_fwd_cross8_bf16_b");
}

// ---- the smoothed-V forms (include/fairygen_hip_cross8s.h): the two entry points above on the v8t, sv and mu of the smoothing V producer
// (include/fairygen_hip_smoothv.h); the same checks, the same grid, the key mean added where an output row is rounded.
extern "C" int fg_attn_cross8s_version(void) { return 1; }

extern "C" int fg_attn_fwd_cross8s_bf16(const void* q8, const void* k8, const float* sq, const float* sk, const void* v8t, const float* sv,
                                        const float* mu, void* out, int64_t Nq, int64_t Nkv, int H, int D, float scale, fg_stream_t stream) {
    FG_CHECK_ARG(q8 && k8 && sq && sk && v8t && sv && out, "fg_attn_fwd_cross8s_bf16: null pointer");
    FG_CHECK_ARG(mu && FG_ALIGNED16(mu), "fg_attn_fwd_cross8s_bf16: mu must be a 16-byte aligned pointer to H*128 floats");
    FG_CHECK_ARG(D == kD, "fg_attn_fwd_cross8s_bf16: only head_dim 128 is supported (got %d)", D);
    FG_CHECK_ARG(H > 0 && Nq > 0, "fg_attn_fwd_cross8s_bf16: H, Nq must be positive");
    FG_CHECK_ARG(Nkv >= 1 && Nkv <= kMaxKv, "fg_attn_fwd_cross8s_bf16: Nkv must be in 1..%d, the keys whose K8 and V8^T fit the LDS (got %lld)",
                 kMaxKv, (long long)Nkv);
    FG_CHECK_ARG(scale > 0.f, "fg_attn_fwd_cross8s_bf16: scale must be positive");
    const int64_t hd = (int64_t)H * D, nkp = (Nkv + kTileKeys - 1) / kTileKeys * kTileKeys, nqb = (Nq + kBM - 1) / kBM;
    FG_CHECK_ARG(FG_ALIGNED16(q8) && FG_ALIGNED16(k8) && FG_ALIGNED16(v8t) && FG_ALIGNED16(sv) && FG_ALIGNED16(out) &&
                     (((uintptr_t)sq | (uintptr_t)sk) & 3) == 0,
                 "fg_attn_fwd_cross8s_bf16: pointers must be 16-byte aligned (sq, sk: 4)");
    FG_CHECK_ARG(Nq * hd * 2 < (1ll << 32), "fg_attn_fwd_cross8s_bf16: O must span < 4 GiB");
    const int cus = device_cus();
    const int64_t per_head = cus / H > 1 ? cus / H : 1;
    const int64_t G = nqb < per_head ? nqb : per_head;      // a function of Nq, H and the device only
    FG_CHECK_ARG((int64_t)H * G < (1ll << 30), "fg_attn_fwd_cross8s_bf16: grid too large");
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(attn_cross8s_kernel),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget);
    FG_CHECK_ARG(attr == hipSuccess, "fg_attn_fwd_cross8s_bf16: cannot reserve 160 KiB of LDS: %s", hipGetErrorString(attr));
    Cross8Params P{};
    P.q8 = (const uint8_t*)q8; P.k8 = (const uint8_t*)k8; P.sq = sq; P.sk = sk; P.v8t = (const uint8_t*)v8t; P.sv = sv;
    P.out = (bf16*)out;
    P.Nq = Nq; P.Nkv = Nkv; P.Nkp = nkp;
    P.H = H; P.G = (int)G; P.nqb = (int)nqb;
    P.scale_log2e = scale * 1.4426950408889634f;
    hipLaunchKernelGGL(attn_cross8s_kernel, dim3((unsigned)(H * G)), dim3(512), (size_t)(2 * kD * nkp), (hipStream_t)stream, P, mu);
    return fg_launch_status("fg_attn_fwd_cross8s_bf16");
}

extern "C" int fg_attn_fwd_cross8s_bf16_b(const void* q8, int64_t bs_q8, const void* k8, int64_t bs_k8, const float* sq, int64_t bs_sq,
                                          const float* sk, int64_t bs_sk, const void* v8t, int64_t bs_v8t, const float* sv, int64_t bs_sv,
                                          const float* mu, int64_t bs_mu, void* out, int64_t bs_out, int B, int64_t Nq, int64_t Nkv, int H,
                                          int D, float scale, fg_stream_t stream) {
    FG_CHECK_ARG(q8 && k8 && sq && sk && v8t && sv && out, "fg_attn_fwd_cross8s_bf16_b: null pointer");
    FG_CHECK_ARG(mu && FG_ALIGNED16(mu), "fg_attn_fwd_cross8s_bf16_b: mu must be a 16-byte aligned pointer to H*128 floats per element");
    FG_CHECK_ARG(D == kD, "fg_attn_fwd_cross8s_bf16_b: only head_dim 128 is supported (got %d)", D);
    FG_CHECK_ARG(B >= 1 && B <= 65535, "fg_attn_fwd_cross8s_bf16_b: B must be in 1..65535 (got %d)", B);
    FG_CHECK_ARG(H > 0 && Nq > 0, "fg_attn_fwd_cross8s_bf16_b: H, Nq must be positive");
    FG_CHECK_ARG(Nkv >= 1 && Nkv <= kMaxKv, "fg_attn_fwd_cross8s_bf16_b: Nkv must be in 1..%d, the keys whose K8 and V8^T fit the LDS (got %lld)",
                 kMaxKv, (long long)Nkv);
    FG_CHECK_ARG(scale > 0.f, "fg_attn_fwd_cross8s_bf16_b: scale must be positive");
    const int64_t hd = (int64_t)H * D, nkp = (Nkv + kTileKeys - 1) / kTileKeys * kTileKeys, nqb = (Nq + kBM - 1) / kBM;
    FG_CHECK_ARG(FG_ALIGNED16(q8) && FG_ALIGNED16(k8) && FG_ALIGNED16(v8t) && FG_ALIGNED16(sv) && FG_ALIGNED16(out) &&
                     (((uintptr_t)sq | (uintptr_t)sk) & 3) == 0,
                 "fg_attn_fwd_cross8s_bf16_b: pointers must be 16-byte aligned (sq, sk: 4)");
    FG_CHECK_ARG(bs_q8 >= Nq * hd && bs_k8 >= Nkv * hd && bs_sq >= Nq * H && bs_sk >= H && bs_v8t >= hd * nkp && bs_sv >= hd && bs_mu >= hd &&
                     bs_out >= Nq * hd,
                 "fg_attn_fwd_cross8s_bf16_b: a batch stride is smaller than one element of its operand");
    FG_CHECK_ARG(bs_q8 % 16 == 0 && bs_k8 % 16 == 0 && bs_v8t % 16 == 0 && bs_sv % 4 == 0 && bs_mu % 4 == 0 && bs_out % 8 == 0,
                 "fg_attn_fwd_cross8s_bf16_b: batch strides must keep the 16-byte alignment of q8, k8, v8t, sv, mu and out");
    FG_CHECK_ARG(Nq * hd * 2 < (1ll << 32), "fg_attn_fwd_cross8s_bf16_b: O of one batch element must span < 4 GiB");
    const int cus = device_cus();
    const int64_t per_head = cus / ((int64_t)B * H) > 1 ? cus / ((int64_t)B * H) : 1;
    const int64_t G = nqb < per_head ? nqb : per_head;      // a function of Nq, B, H and the device only
    FG_CHECK_ARG((int64_t)H * G < (1ll << 30), "fg_attn_fwd_cross8s_bf16_b: grid too large");
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(attn_cross8s_b_kernel),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget);
    FG_CHECK_ARG(attr == hipSuccess, "fg_attn_fwd_cross8s_bf16_b: cannot reserve 160 KiB of LDS: %s", hipGetErrorString(attr));
    Cross8ParamsB PB{};
    Cross8Params& P = PB.p;
    P.q8 = (const uint8_t*)q8; P.k8 = (const uint8_t*)k8; P.sq = sq; P.sk = sk; P.v8t = (const uint8_t*)v8t; P.sv = sv;
    P.out = (bf16*)out;
    P.Nq = Nq; P.Nkv = Nkv; P.Nkp = nkp;
    P.H = H; P.G = (int)G; P.nqb = (int)nqb;
    P.scale_log2e = scale * 1.4426950408889634f;
    PB.bs_q8 = bs_q8; PB.bs_k8 = bs_k8; PB.bs_sq = bs_sq; PB.bs_sk = bs_sk; PB.bs_v8t = bs_v8t; PB.bs_sv = bs_sv; PB.bs_out = bs_out;
    hipLaunchKernelGGL(attn_cross8s_b_kernel, dim3((unsigned)(H * G), (unsigned)B), dim3(512), (size_t)(2 * kD * nkp), (hipStream_t)stream, PB,
                       mu, bs_mu);
    return fg_launch_status("fg_attn_fwd_cross8s_bf16_b");
}
