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
//
// The smoothing form (fg_attn_quant_vt_smooth_bf16, include/fairygen_hip_smoothv.h; DESIGN §5 "e4m3 P V with smoothed V") takes the key
// mean of every channel out of v before it is quantised:
//   mu[c] = fl32(fp64 sum over the N keys of v[j][c] / N),  d = fl32(v - mu[c]),  sv[c] = max(max |d| / 448, 2^-20),  v8 = e4m3(d / sv[c]).
// The same two launches: pass 1 leaves per channel and row stride the fp64 sum, the minimum and the maximum of v (16 bytes a record:
// fg_attn_smoothv_scratch_bytes); pass 2 adds the sums in a fixed order (below), and since fl32(v - mu) is monotone in v the largest |d|
// is max(fl32(vmax - mu), fl32(mu - vmin)): no third pass over v.  The attention kernel adds mu back to its output rows.
#include "common.h"
#include "../../include/fairygen_hip_pv8.h"
#include "../../include/fairygen_hip_batch8.h"
#include "../../include/fairygen_hip_smoothv.h"
#include "attn_qk8_quant.h"
#include "attn_pv8_parts.h"
#include "attn_smoothv_parts.h"

namespace {

constexpr int kMaxTileBlocks = 32;

// Workgroup (x, h) of 256: the scales of head h from the `parts` records, then the tiles x, x + gridDim.x, ..  Thread t converts the 8
// channels of chunk cl = t & 15 of the 4 keys 4 kg .. 4 kg + 3, kg = t >> 4: 8 dwords, one per channel, to row 8 cl + j of the image at
// dword pv8_dword(kg) ^ cl (the XOR spreads the 16 chunks of a key group over 16 banks; it permutes the dwords of a 16-byte chunk among
// themselves and the chunks of a row among themselves, and the read below undoes both).
// (the body is one text for this form and the smoothing form; FG_QUANT_VT_PLAIN names what only the other form reads)
#define FG_QUANT_VT_PLAIN                                                                                                       \
    constexpr bool SMV = false;                                                                                                 \
    const double* const rsum = nullptr;                                                                                         \
    const float *const rlo = nullptr, *const rhi = nullptr;                                                                     \
    float* const mu = nullptr
__global__ __launch_bounds__(256) void attn_quant_vt_kernel(const bf16* __restrict__ v, int64_t ldv, const float* __restrict__ rec, int parts,
                                                            uint8_t* __restrict__ v8t, float* __restrict__ sv, int64_t N, int64_t Nkp, int H) {
    FG_QUANT_VT_PLAIN;
#include "attn_quant_vt_body.inc"
}

// The batched forms (include/fairygen_hip_batch8.h): grid dimension z picks the batch element, which runs the single-element body on its
// own pointers; bs.rec counts floats.
struct QuantVtStrides {
    int64_t v, v8t, sv, rec;
};

__global__ __launch_bounds__(256) void attn_v_stats_b_kernel(const bf16* __restrict__ v, int64_t ldv, float* __restrict__ rec, int64_t N, int C,
                                                             const QuantVtStrides bs) {
    const int64_t b = blockIdx.z;
    attn_v_stats_body(v + b * bs.v, ldv, rec + b * bs.rec, N, C);
}

__global__ __launch_bounds__(256) void attn_quant_vt_b_kernel(const bf16* __restrict__ v, int64_t ldv, const float* __restrict__ rec, int parts,
                                                              uint8_t* __restrict__ v8t, float* __restrict__ sv, int64_t N, int64_t Nkp, int H,
                                                              const QuantVtStrides bs) {
    const int64_t b = blockIdx.z;
    v += b * bs.v; rec += b * bs.rec; v8t += b * bs.v8t; sv += b * bs.sv;
    FG_QUANT_VT_PLAIN;
#include "attn_quant_vt_body.inc"
}
#undef FG_QUANT_VT_PLAIN

// ---- the smoothing form.  The records of a launch: rsum [parts][C] fp64, then rlo and rhi [parts][C] fp32 each, in the caller's scratch.
// Pass 1 is attn_v_stats_smooth_body (attn_smoothv_parts.h, shared with the producers of a token shard).
// The records of ONE element inside its scratch of `parts` strides of C channels
struct SmoothRecords {
    double* rsum;
    float* rlo;
    float* rhi;
};
__host__ __device__ __forceinline__ SmoothRecords smooth_records(void* scratch, int64_t parts, int64_t C) {
    double* const rsum = (double*)scratch;
    float* const rlo = (float*)(rsum + parts * C);
    return SmoothRecords{rsum, rlo, rlo + parts * C};
}

struct QuantVtSmoothStrides {
    int64_t v, v8t, sv, mu, scratch;      // scratch in bytes, the others in elements
};

// grid dimension z picks the batch element (1 for the single-element entry point: every stride is then unused)
__global__ __launch_bounds__(256) void attn_v_stats_smooth_kernel(const bf16* __restrict__ v, int64_t ldv, char* __restrict__ scratch, int parts,
                                                                  int64_t N, int C, const QuantVtSmoothStrides bs) {
    const int64_t b = blockIdx.z;
    const SmoothRecords r = smooth_records(scratch + b * bs.scratch, parts, C);
    attn_v_stats_smooth_body(v + b * bs.v, ldv, r.rsum, r.rlo, r.rhi, N, C);
}

// Pass 2: attn_quant_vt_kernel's workgroups and tiles.  Thread (c, g) of the 2 x 128 adds the sums of the strides g, g + 2, .. of its
// channel in that order and the total is half 0 + half 1: with `parts` a function of N alone (v_stat_parts) mu does not depend on a
// launch grid.
__global__ __launch_bounds__(256) void attn_quant_vt_smooth_kernel(const bf16* __restrict__ v, int64_t ldv, const char* __restrict__ scratch,
                                                                   int parts, uint8_t* __restrict__ v8t, float* __restrict__ sv,
                                                                   float* __restrict__ mu, int64_t N, int64_t Nkp, int H,
                                                                   const QuantVtSmoothStrides bs) {
    constexpr bool SMV = true;
    const int64_t b = blockIdx.z;
    const SmoothRecords r = smooth_records(const_cast<char*>(scratch) + b * bs.scratch, parts, (int64_t)H * kD);
    const double* const rsum = r.rsum;
    const float *const rlo = r.rlo, *const rhi = r.rhi, *const rec = nullptr;
    v += b * bs.v; v8t += b * bs.v8t; sv += b * bs.sv; mu += b * bs.mu;
#include "attn_quant_vt_body.inc"
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

extern "C" int fg_attn_quant_vt_bf16_b(const void* v, int64_t ldv, int64_t bs_v, void* v8t, int64_t bs_v8t, float* sv, int64_t bs_sv,
                                       void* scratch, int64_t scratch_bytes, int64_t bs_scratch, int B, int64_t N, int H, int D,
                                       fg_stream_t stream) {
    FG_CHECK_ARG(v && v8t && sv && scratch, "fg_attn_quant_vt_bf16_b: null pointer");
    FG_CHECK_ARG(D == kD, "fg_attn_quant_vt_bf16_b: only head_dim 128 is supported (got %d)", D);
    FG_CHECK_ARG(B >= 1 && B <= 65535, "fg_attn_quant_vt_bf16_b: B must be in 1..65535 (got %d)", B);
    FG_CHECK_ARG(N > 0 && H > 0 && H <= 65535, "fg_attn_quant_vt_bf16_b: N must be positive, H in 1..65535");
    const int64_t hd = (int64_t)H * D, nkp = (N + kTileKeys - 1) / kTileKeys * kTileKeys;
    FG_CHECK_ARG(ldv >= hd && ldv % 8 == 0, "fg_attn_quant_vt_bf16_b: ldv must be >= H*D and a multiple of 8");
    FG_CHECK_ARG(FG_ALIGNED16(v) && FG_ALIGNED16(v8t) && FG_ALIGNED16(sv) && FG_ALIGNED16(scratch),
                 "fg_attn_quant_vt_bf16_b: v, v8t, sv and scratch must be 16-byte aligned");
    const int64_t parts = v_stat_parts(N);
    FG_CHECK_ARG(scratch_bytes >= parts * hd * 4, "fg_attn_quant_vt_bf16_b: scratch must hold %lld bytes per element (got %lld)",
                 (long long)(parts * hd * 4), (long long)scratch_bytes);
    FG_CHECK_ARG(bs_v >= (N - 1) * ldv + hd && bs_v8t >= hd * nkp && bs_sv >= hd && bs_scratch >= parts * hd * 4,
                 "fg_attn_quant_vt_bf16_b: a batch stride is smaller than one element of its operand");
    FG_CHECK_ARG(bs_v % 8 == 0 && bs_v8t % 16 == 0 && bs_sv % 4 == 0 && bs_scratch % 16 == 0,
                 "fg_attn_quant_vt_bf16_b: batch strides must keep the alignment (v: 8 elements; v8t: 16 bytes; sv: 4 floats; scratch: 16 bytes)");
    const QuantVtStrides bs{bs_v, bs_v8t, bs_sv, bs_scratch / 4};
    hipLaunchKernelGGL(attn_v_stats_b_kernel, dim3((unsigned)parts, (unsigned)((hd / 8 + 63) / 64), (unsigned)B), dim3(256), 0,
                       (hipStream_t)stream, (const bf16*)v, ldv, (float*)scratch, N, (int)hd, bs);
    if (int e = fg_launch_status("fg_attn_quant_vt_bf16_b (v statistics)")) return e;
    const int64_t nt = nkp / kTileKeys;
    hipLaunchKernelGGL(attn_quant_vt_b_kernel, dim3((unsigned)(nt < kMaxTileBlocks ? nt : kMaxTileBlocks), (unsigned)H, (unsigned)B), dim3(256), 0,
                       (hipStream_t)stream, (const bf16*)v, ldv, (const float*)scratch, (int)parts, (uint8_t*)v8t, sv, N, nkp, H, bs);
    return fg_launch_status("fg_attn_quant_vt_bf16_b");
}

// ---- the smoothing form (include/fairygen_hip_smoothv.h)
extern "C" int fg_attn_smoothv_version(void) { return 1; }

extern "C" int64_t fg_attn_smoothv_scratch_bytes(int64_t N, int H) {
    if (N < 1 || H < 1 || H > 65535) {
        fg_set_error("fg_attn_smoothv_scratch_bytes: N must be positive, H in 1..65535 (got N=%lld H=%d)", (long long)N, H);
        return -1;
    }
    return v_stat_parts(N) * H * kD * 16;
}

namespace {

int launch_quant_vt_smooth(const char* who, const void* v, int64_t ldv, void* v8t, float* sv, float* mu, void* scratch, int B, int64_t N, int H,
                           const QuantVtSmoothStrides& bs, fg_stream_t stream) {
    const int64_t hd = (int64_t)H * kD, nt = (N + kTileKeys - 1) / kTileKeys, parts = v_stat_parts(N);
    hipLaunchKernelGGL(attn_v_stats_smooth_kernel, dim3((unsigned)parts, (unsigned)((hd / 8 + 63) / 64), (unsigned)B), dim3(256), 0,
                       (hipStream_t)stream, (const bf16*)v, ldv, (char*)scratch, (int)parts, N, (int)hd, bs);
    if (int e = fg_launch_status(who)) return e;
    hipLaunchKernelGGL(attn_quant_vt_smooth_kernel, dim3((unsigned)(nt < kMaxTileBlocks ? nt : kMaxTileBlocks), (unsigned)H, (unsigned)B), dim3(256),
                       0, (hipStream_t)stream, (const bf16*)v, ldv, (const char*)scratch, (int)parts, (uint8_t*)v8t, sv, mu, N, nt * kTileKeys, H, bs);
    return fg_launch_status(who);
}

}  // namespace

extern "C" int fg_attn_quant_vt_smooth_bf16(const void* v, int64_t ldv, void* v8t, float* sv, float* mu, void* scratch, int64_t scratch_bytes,
                                            int64_t N, int H, int D, fg_stream_t stream) {
    FG_CHECK_ARG(v && v8t && sv && scratch, "fg_attn_quant_vt_smooth_bf16: null pointer");
    FG_CHECK_ARG(mu && FG_ALIGNED16(mu), "fg_attn_quant_vt_smooth_bf16: mu must be a 16-byte aligned pointer to H*128 floats");
    FG_CHECK_ARG(D == kD, "fg_attn_quant_vt_smooth_bf16: only head_dim 128 is supported (got %d)", D);
    FG_CHECK_ARG(N > 0 && H > 0 && H <= 65535, "fg_attn_quant_vt_smooth_bf16: N must be positive, H in 1..65535");
    const int64_t hd = (int64_t)H * D;
    FG_CHECK_ARG(ldv >= hd && ldv % 8 == 0, "fg_attn_quant_vt_smooth_bf16: ldv must be >= H*D and a multiple of 8");
    FG_CHECK_ARG(FG_ALIGNED16(v) && FG_ALIGNED16(v8t) && FG_ALIGNED16(sv) && FG_ALIGNED16(scratch),
                 "fg_attn_quant_vt_smooth_bf16: v, v8t, sv and scratch must be 16-byte aligned");
    const int64_t need = v_stat_parts(N) * hd * 16;
    FG_CHECK_ARG(scratch_bytes >= need, "fg_attn_quant_vt_smooth_bf16: scratch must hold %lld bytes (got %lld)", (long long)need,
                 (long long)scratch_bytes);
    return launch_quant_vt_smooth("fg_attn_quant_vt_smooth_bf16", v, ldv, v8t, sv, mu, scratch, 1, N, H, QuantVtSmoothStrides{}, stream);
}

extern "C" int fg_attn_quant_vt_smooth_bf16_b(const void* v, int64_t ldv, int64_t bs_v, void* v8t, int64_t bs_v8t, float* sv, int64_t bs_sv,
                                              float* mu, int64_t bs_mu, void* scratch, int64_t scratch_bytes, int64_t bs_scratch, int B,
                                              int64_t N, int H, int D, fg_stream_t stream) {
    FG_CHECK_ARG(v && v8t && sv && scratch, "fg_attn_quant_vt_smooth_bf16_b: null pointer");
    FG_CHECK_ARG(mu && FG_ALIGNED16(mu), "fg_attn_quant_vt_smooth_bf16_b: mu must be a 16-byte aligned pointer to H*128 floats per element");
    FG_CHECK_ARG(D == kD, "fg_attn_quant_vt_smooth_bf16_b: only head_dim 128 is supported (got %d)", D);
    FG_CHECK_ARG(B >= 1 && B <= 65535, "fg_attn_quant_vt_smooth_bf16_b: B must be in 1..65535 (got %d)", B);
    FG_CHECK_ARG(N > 0 && H > 0 && H <= 65535, "fg_attn_quant_vt_smooth_bf16_b: N must be positive, H in 1..65535");
    const int64_t hd = (int64_t)H * D, nkp = (N + kTileKeys - 1) / kTileKeys * kTileKeys;
    FG_CHECK_ARG(ldv >= hd && ldv % 8 == 0, "fg_attn_quant_vt_smooth_bf16_b: ldv must be >= H*D and a multiple of 8");
    FG_CHECK_ARG(FG_ALIGNED16(v) && FG_ALIGNED16(v8t) && FG_ALIGNED16(sv) && FG_ALIGNED16(scratch),
                 "fg_attn_quant_vt_smooth_bf16_b: v, v8t, sv and scratch must be 16-byte aligned");
    const int64_t need = v_stat_parts(N) * hd * 16;
    FG_CHECK_ARG(scratch_bytes >= need, "fg_attn_quant_vt_smooth_bf16_b: scratch must hold %lld bytes per element (got %lld)", (long long)need,
                 (long long)scratch_bytes);
    FG_CHECK_ARG(bs_v >= (N - 1) * ldv + hd && bs_v8t >= hd * nkp && bs_sv >= hd && bs_mu >= hd && bs_scratch >= need,
                 "fg_attn_quant_vt_smooth_bf16_b: a batch stride is smaller than one element of its operand");
    FG_CHECK_ARG(bs_v % 8 == 0 && bs_v8t % 16 == 0 && bs_sv % 4 == 0 && bs_mu % 4 == 0 && bs_scratch % 16 == 0,
                 "fg_attn_quant_vt_smooth_bf16_b: batch strides must keep the alignment (v: 8 elements; v8t: 16 bytes; sv, mu: 4 floats; "
                 "scratch: 16 bytes)");
    return launch_quant_vt_smooth("fg_attn_quant_vt_smooth_bf16_b", v, ldv, v8t, sv, mu, scratch, B, N, H,
                                  QuantVtSmoothStrides{bs_v, bs_v8t, bs_sv, bs_mu, bs_scratch}, stream);
}
