// Hot-loaded (unfused) LoRA adapters on one plain-HIP MFMA kernel: out = epi(out, bf16(bf16(x A^T) B^T)) per column group.
//
// Replaces the two library GEMMs, the full-size temporary and the separate add of AutoWrappedLinear.lora_forward
// (core/vram/layers.py:417-436: `out = out + x @ A^T @ B^T` per adapter) for the adapters of one Linear stacked along the rank, and
// leaves the Linear itself on fg_gemm_epilogue_bf16 with its fused store.  Bandwidth-bound by design: x is streamed once (once per
// pass, see fg_lora_apply_bf16), `out` is read once and written once with 16-byte accesses; A and B are small and come from L2.
//
// A workgroup (4 waves) owns 64 rows.
//   phase 1  t^T = A x^T: the four waves split K in interleaved 64-element chunks (a wave reads one 128-byte line per row and chunk);
//            both MFMA operands are rows of a row-major matrix, so every lane loads 16 contiguous bytes straight from global memory
//            (the k order inside a chunk is permuted the same way for both operands: lane half h, step s holds k = 32h + 8s + j).
//            The four partial sums are added in fp32 in a fixed order (wave 0 + 1 + 2 + 3) through LDS; t is rounded to bf16 once and
//            stays in LDS, row-major (64, G*R), rows padded by 16 bytes.
//   phase 2  l^T = B t^T per 64-column block of `out` (blocks dealt round-robin to the waves): the A operand is 32 rows of B from
//            global memory, the B operand rows of t from LDS.  In the transposed product a lane holds 4 consecutive columns of ONE
//            output row per register quad; one v_permlane32_swap per dword pairs the quads of the two lane halves into 8 consecutive
//            columns, so the read-modify-write of `out` is dwordx4 per lane.
#include "common.h"
#include "../../include/fairygen_hip_lorabatch.h"     // the adapter kernel on batches that share their gate table

namespace {

constexpr int kRows = 64;            // rows of x / out per workgroup
constexpr int kTPad = 8;             // bf16 elements of padding per row of t in LDS (16 bytes: ds_read_b128 of 32 rows spreads over the banks)
constexpr int kMaxGroups = 4;

struct LoraParams {
    const bf16* x; const bf16* a; const bf16* b; bf16* out; const bf16* gate;
    int64_t ldx, ldc, gate_ld;       // elements; gate_ld = 0 for a 1-row gate table
    int M, K, Ng, G, mode, first_rows;
};

__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    const bf16x2 v = {(bf16)lo, (bf16)hi};
    return __builtin_bit_cast(uint32_t, v);
}

// RT: 32-row tiles of the per-group rank R (R = 32 RT); GC: groups whose t is computed in one pass over x (G % GC == 0).
template <int RT, int GC>
__global__ __launch_bounds__(256, RT * GC <= 3 ? 2 : 1) void lora_apply_kernel(const LoraParams P) {
#include "lora_apply_body.inc"
}

template <int RT, int GC>
int launch_lora(const LoraParams& P, hipStream_t stream) {
    const int lds = 2 * RT * GC * 16 * 64 * 4 + kRows * (P.G * 32 * RT + kTPad) * 2;
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(lora_apply_kernel<RT, GC>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                       2 * RT * GC * 16 * 64 * 4 + kRows * (kMaxGroups * 32 * RT + kTPad) * 2);
    FG_CHECK_ARG(attr == hipSuccess, "fg_lora_apply_bf16: cannot reserve LDS: %s", hipGetErrorString(attr));
    hipLaunchKernelGGL((lora_apply_kernel<RT, GC>), dim3((unsigned)((P.M + kRows - 1) / kRows)), dim3(256), lds, stream, P);
    return fg_launch_status("fg_lora_apply_bf16");
}

// The batched form (include/fairygen_hip_lorabatch.h): x / out are the B * M rows of one matrix each, the second grid dimension picks the
// element, and the element runs the body above on its own pointers — M, first_rows and the gate's row rule are ONE element's, A, B and
// the gate table are shared.  No workgroup holds rows of two elements.  The element offset is 64-bit; everything behind it is the
// single-element kernel's addressing.
template <int RT, int GC>
__global__ __launch_bounds__(256, RT * GC <= 3 ? 2 : 1) void lora_apply_b_kernel(const LoraParams PB) {
    LoraParams P = PB;
    P.x += (int64_t)blockIdx.y * PB.M * PB.ldx;
    P.out += (int64_t)blockIdx.y * PB.M * PB.ldc;
#include "lora_apply_body.inc"
}

template <int RT, int GC>
int launch_lora_b(const LoraParams& P, int B, hipStream_t stream) {
    const int lds = 2 * RT * GC * 16 * 64 * 4 + kRows * (P.G * 32 * RT + kTPad) * 2;
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(lora_apply_b_kernel<RT, GC>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                       2 * RT * GC * 16 * 64 * 4 + kRows * (kMaxGroups * 32 * RT + kTPad) * 2);
    FG_CHECK_ARG(attr == hipSuccess, "fg_lora_apply_bf16_b: cannot reserve LDS: %s", hipGetErrorString(attr));
    hipLaunchKernelGGL((lora_apply_b_kernel<RT, GC>), dim3((unsigned)((P.M + kRows - 1) / kRows), (unsigned)B), dim3(256), lds, stream, P);
    return fg_launch_status("fg_lora_apply_bf16_b");
}

// ---------------------------------------------------------------- fg_lora_fuse_bf16: w' = bf16(w + bf16(alpha * bf16(B A)))
// One adapter folded into one Linear's weight at the rounding points of GeneralLoRALoader.fuse_lora_to_base_model.  It is phase 2 above
// with other operands: d^T = A^T-rows x B-rows per 64 x 64 tile of w, one tile per wave, nothing shared between waves (no LDS, no barrier).
// Both MFMA operands are rows of a row-major (., R) matrix (the host hands A over transposed), so every lane loads 16 contiguous bytes;
// after the half-wave swap a lane owns 8 consecutive columns of one row of w: one dwordx4 read, one dwordx4 write and, with the e4m3 copy,
// one dwordx2 write per lane and quad pair.  A lane reads its elements of w_src before it writes them and no other lane touches them,
// so w_dst may be w_src itself.
struct FuseParams {
    const bf16* src; bf16* dst; uint8_t* dst8; const bf16* at; const bf16* b;
    int64_t ld_src, ld_dst, ld_dst8;
    int N, K;
    float alpha;
};

// Two fp32 -> two e4m3 bytes in the low half of a dword, as torch's cast to float8_e4m3fn makes them for EVERY input: v_cvt_pk_fp8_f32
// (RNE, OCP e4m3fn on gfx950) inside the finite range; above it the cast does not saturate — |v| <= 464 still rounds to 448, anything
// larger and NaN become the NaN byte with v's sign — and that is spelled out here so the result does not hang on the overflow mode.
__device__ __forceinline__ uint32_t pack_fp8x2(float a, float b) {
    const bool fa = __builtin_fabsf(a) <= 464.0f, fb = __builtin_fabsf(b) <= 464.0f;      // false for NaN
    const uint32_t v = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(fa ? fminf(fmaxf(a, -448.0f), 448.0f) : 0.0f, fb ? fminf(fmaxf(b, -448.0f), 448.0f) : 0.0f, 0, false) & 0xffffu;
    const uint32_t na = (__builtin_bit_cast(uint32_t, a) >> 24 & 0x80u) | 0x7fu, nb = (__builtin_bit_cast(uint32_t, b) >> 24 & 0x80u) | 0x7fu;
    return (fa ? v & 0xffu : na) | (fb ? v & 0xff00u : nb << 8);
}

template <int RT>
__global__ __launch_bounds__(256) void lora_fuse_kernel(const FuseParams P) {
    constexpr int R = 32 * RT;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 31, lh = lane >> 5;
    const int kb = blockIdx.y * 4 + wave;      // this wave's 64-column block of w
    if (kb >= P.K / 64) return;
    const int64_t n0 = (int64_t)blockIdx.x * 64;
    const int64_t col0 = (int64_t)kb * 64 + 8 * lh;      // this lane's first column after the half-wave swap
    u32x4 ov[2][2][2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int q = 0; q < 2; ++q) ov[mt][nt][q] = *reinterpret_cast<const u32x4*>(P.src + (n0 + 32 * mt + lr) * P.ld_src + col0 + 32 * nt + 16 * q);
    f32x16 acc[2][2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[mt][nt][i] = 0.f;
    const bf16* arow = P.at + ((int64_t)kb * 64 + lr) * R + 8 * lh;
    const bf16* brow = P.b + (n0 + lr) * R + 8 * lh;
#pragma unroll
    for (int s = 0; s < 2 * RT; ++s) {
        bf16x8 af[2], bfr[2];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) af[nt] = *reinterpret_cast<const bf16x8*>(arow + nt * 32 * R + 16 * s);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) bfr[mt] = *reinterpret_cast<const bf16x8*>(brow + mt * 32 * R + 16 * s);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[nt], bfr[mt], acc[mt][nt], 0, 0, 0);
    }
    const float alpha = P.alpha;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                // quads 2q and 2q + 1 (columns 16q + 4lh + 0..3 and 16q + 8 + 4lh + 0..3 of row lr), rounded to bf16, then paired across the halves
                uint32_t a0 = pack_bf16x2(acc[mt][nt][8 * q], acc[mt][nt][8 * q + 1]), a1 = pack_bf16x2(acc[mt][nt][8 * q + 2], acc[mt][nt][8 * q + 3]);
                uint32_t b0 = pack_bf16x2(acc[mt][nt][8 * q + 4], acc[mt][nt][8 * q + 5]), b1 = pack_bf16x2(acc[mt][nt][8 * q + 6], acc[mt][nt][8 * q + 7]);
                const auto r0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
                const auto r1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
                const u32x4 dw = {r0[0], r1[0], r0[1], r1[1]};
                const bf16x8 d8 = __builtin_bit_cast(bf16x8, dw), old = __builtin_bit_cast(bf16x8, ov[mt][nt][q]);
                bf16x8 o8;
#pragma unroll
                for (int j = 0; j < 8; ++j) o8[j] = (bf16)((float)old[j] + rbf(alpha * (float)d8[j]));      // alpha == 1: the product is d itself
                const int64_t row = n0 + 32 * mt + lr, col = col0 + 32 * nt + 16 * q;
                *reinterpret_cast<bf16x8*>(P.dst + row * P.ld_dst + col) = o8;
                if (P.dst8) {
                    const u32x2 e8 = {pack_fp8x2((float)o8[0], (float)o8[1]) | pack_fp8x2((float)o8[2], (float)o8[3]) << 16,
                                      pack_fp8x2((float)o8[4], (float)o8[5]) | pack_fp8x2((float)o8[6], (float)o8[7]) << 16};
                    *reinterpret_cast<u32x2*>(P.dst8 + row * P.ld_dst8 + col) = e8;
                }
            }
}

template <int RT>
int launch_fuse(const FuseParams& P, hipStream_t stream) {
    hipLaunchKernelGGL((lora_fuse_kernel<RT>), dim3((unsigned)(P.N / 64), (unsigned)((P.K / 64 + 3) / 4)), dim3(256), 0, stream, P);
    return fg_launch_status("fg_lora_fuse_bf16");
}


}  // namespace

// The checks of fg_lora_apply_bf16 on one element of M rows, and its parameters; shared with the batched entry point.
static int lora_params(const char* what, LoraParams& P, const void* x, int64_t ldx, const void* a, const void* b, void* out, int64_t ldc,
                       int64_t M, int64_t K, int64_t Ng, int64_t R, int64_t G, int mode, const void* gate, int64_t gate_rows,
                       int64_t gate_ld, int64_t first_rows) {
    FG_CHECK_ARG(x && a && b && out, "%s: null pointer", what);
    FG_CHECK_ARG(mode == 0 || mode == 1 || mode == 2 || mode == 4, "%s: mode must be 0 (write), 1 (out + l), 2 (out + gate*l) or 4 (gelu_tanh(out + l))", what);
    FG_CHECK_ARG(M > 0 && K > 0 && Ng > 0 && G >= 1 && G <= kMaxGroups && K % 64 == 0 && Ng % 64 == 0,
                 "%s: need K %% 64 == 0, Ng %% 64 == 0 and 1 to %d groups (K=%lld Ng=%lld G=%lld)", what, kMaxGroups, (long long)K, (long long)Ng, (long long)G);
    FG_CHECK_ARG(R >= 32 && R <= 128 && R % 32 == 0, "%s: the per-group rank must be padded to 32, 64, 96 or 128 (R=%lld)", what, (long long)R);
    FG_CHECK_ARG(mode != 2 || (gate && (gate_rows == 1 || gate_rows == 2) && gate_ld >= G * Ng && FG_ALIGNED16(gate) && gate_ld % 8 == 0),
                 "%s: mode 2 needs a gate table of 1 or 2 rows, 16-byte aligned rows", what);
    FG_CHECK_ARG(ldx >= K && ldc >= G * Ng && ldx % 8 == 0 && ldc % 8 == 0 && FG_ALIGNED16(x) && FG_ALIGNED16(a) && FG_ALIGNED16(b) && FG_ALIGNED16(out),
                 "%s: leading dimensions must cover the rows, rows and pointers 16-byte aligned", what);
    FG_CHECK_ARG(kRows * ldx * 2 < (1ll << 31) && kRows * ldc * 2 < (1ll << 31) && G * R * K * 2 < (1ll << 31) && G * Ng * R * 2 < (1ll << 31) && M < (1ll << 31),
                 "%s: tile spans must fit 31 bits", what);
    P.x = (const bf16*)x; P.a = (const bf16*)a; P.b = (const bf16*)b; P.out = (bf16*)out; P.gate = (const bf16*)gate;
    P.ldx = ldx; P.ldc = ldc; P.gate_ld = gate_rows == 2 ? gate_ld : 0;
    P.M = (int)M; P.K = (int)K; P.Ng = (int)Ng; P.G = (int)G; P.mode = mode;
    P.first_rows = gate_rows == 2 ? (int)(first_rows < 0 ? 0 : first_rows > M ? M : first_rows) : 0;
    return FG_OK;
}

extern "C" int fg_lora_apply_bf16(const void* x, int64_t ldx, const void* a, const void* b, void* out, int64_t ldc, int64_t M, int64_t K,
                                  int64_t Ng, int64_t R, int64_t G, int mode, const void* gate, int64_t gate_rows, int64_t gate_ld,
                                  int64_t first_rows, fg_stream_t stream) {
    LoraParams P;
    if (int e = lora_params("fg_lora_apply_bf16", P, x, ldx, a, b, out, ldc, M, K, Ng, R, G, mode, gate, gate_rows, gate_ld, first_rows)) return e;
    hipStream_t s = (hipStream_t)stream;
    // q | k | v at rank 32 (the common adapter) share one pass over x; every other pack takes one pass per group
    if (R == 32 && G == 3) return launch_lora<1, 3>(P, s);
    switch (R / 32) {
        case 1: return launch_lora<1, 1>(P, s);
        case 2: return launch_lora<2, 1>(P, s);
        case 3: return launch_lora<3, 1>(P, s);
        default: return launch_lora<4, 1>(P, s);
    }
}

// ---- include/fairygen_hip_lorabatch.h: fg_lora_apply_bf16 on B elements of M rows each that share A, B and the gate table.  The checks
// are the single-element entry point's on ONE element (M, first_rows count inside it), then B and the rows of the whole matrix.  The
// batch needs no span check of its own: the kernel reaches an element's first row with a 64-bit offset and addresses rows in 64 bits.
extern "C" int fg_dit_lorabatch_version(void) { return 1; }

extern "C" int fg_lora_apply_bf16_b(const void* x, int64_t ldx, const void* a, const void* b, void* out, int64_t ldc, int B, int64_t M,
                                    int64_t K, int64_t Ng, int64_t R, int64_t G, int mode, const void* gate, int64_t gate_rows,
                                    int64_t gate_ld, int64_t first_rows, fg_stream_t stream) {
    const char* what = "fg_lora_apply_bf16_b";
    LoraParams P;
    if (int e = lora_params(what, P, x, ldx, a, b, out, ldc, M, K, Ng, R, G, mode, gate, gate_rows, gate_ld, first_rows)) return e;
    FG_CHECK_ARG(B >= 1 && B <= 65535, "%s: B must be in 1..65535 (got %d)", what, B);
    FG_CHECK_ARG((int64_t)B * M < (1ll << 31), "%s: B * M must fit 31 bits (B=%d M=%lld)", what, B, (long long)M);
    hipStream_t s = (hipStream_t)stream;
    if (R == 32 && G == 3) return launch_lora_b<1, 3>(P, B, s);      // the instantiation fg_lora_apply_bf16 picks, per element
    switch (R / 32) {
        case 1: return launch_lora_b<1, 1>(P, B, s);
        case 2: return launch_lora_b<2, 1>(P, B, s);
        case 3: return launch_lora_b<3, 1>(P, B, s);
        default: return launch_lora_b<4, 1>(P, B, s);
    }
}

extern "C" int fg_lora_fuse_bf16(const void* w_src, int64_t ld_src, void* w_dst, int64_t ld_dst, void* w_dst_fp8, int64_t ld_fp8, const void* a_t,
                                 const void* b, int64_t N, int64_t K, int64_t R, float alpha, fg_stream_t stream) {
    const char* what = "fg_lora_fuse_bf16";
    FG_CHECK_ARG(w_src && w_dst && a_t && b, "%s: null pointer", what);
    FG_CHECK_ARG(N > 0 && K > 0 && N % 64 == 0 && K % 64 == 0, "%s: need N %% 64 == 0 and K %% 64 == 0 (N=%lld K=%lld)", what, (long long)N, (long long)K);
    FG_CHECK_ARG(R >= 32 && R <= 128 && R % 32 == 0, "%s: the rank must be padded to 32, 64, 96 or 128 (R=%lld)", what, (long long)R);
    FG_CHECK_ARG(ld_src >= K && ld_dst >= K && ld_src % 8 == 0 && ld_dst % 8 == 0 && FG_ALIGNED16(w_src) && FG_ALIGNED16(w_dst) && FG_ALIGNED16(a_t) &&
                     FG_ALIGNED16(b),
                 "%s: leading dimensions must cover the rows, rows and pointers 16-byte aligned", what);
    FG_CHECK_ARG(!w_dst_fp8 || (ld_fp8 >= K && ld_fp8 % 16 == 0 && FG_ALIGNED16(w_dst_fp8)), "%s: the e4m3 copy needs 16-byte aligned rows that cover K", what);
    {   // in place is fine, any other overlap is a read of elements another wave may already have rewritten
        const char *s0 = (const char*)w_src, *s1 = s0 + ((N - 1) * ld_src + K) * 2, *d0 = (const char*)w_dst, *d1 = d0 + ((N - 1) * ld_dst + K) * 2;
        FG_CHECK_ARG((s0 == d0 && ld_src == ld_dst) || s1 <= d0 || d1 <= s0, "%s: w_dst must be w_src itself (same leading dimension) or not overlap it", what);
    }
    if (w_dst_fp8) {
        const char *e0 = (const char*)w_dst_fp8, *e1 = e0 + (N - 1) * ld_fp8 + K, *s0 = (const char*)w_src, *s1 = s0 + ((N - 1) * ld_src + K) * 2,
                   *d0 = (const char*)w_dst, *d1 = d0 + ((N - 1) * ld_dst + K) * 2;
        FG_CHECK_ARG((e1 <= s0 || s1 <= e0) && (e1 <= d0 || d1 <= e0), "%s: the e4m3 copy must not overlap w_src or w_dst", what);
    }
    FG_CHECK_ARG(N < (1ll << 31) && K / 256 < 65535, "%s: N and K / 256 must fit the grid", what);
    FuseParams P;
    P.src = (const bf16*)w_src; P.dst = (bf16*)w_dst; P.dst8 = (uint8_t*)w_dst_fp8; P.at = (const bf16*)a_t; P.b = (const bf16*)b;
    P.ld_src = ld_src; P.ld_dst = ld_dst; P.ld_dst8 = ld_fp8; P.N = (int)N; P.K = (int)K; P.alpha = alpha;
    hipStream_t s = (hipStream_t)stream;
    switch (R / 32) {
        case 1: return launch_fuse<1>(P, s);
        case 2: return launch_fuse<2>(P, s);
        case 3: return launch_fuse<3>(P, s);
        default: return launch_fuse<4>(P, s);
    }
}
