// The body of attn_combine_kernel (attention.hip), included by that kernel and by its batched form attn_combine_b_kernel and the smoothed-V forms
// of the two: all see `const AttnParams P`, the constant SMV and (read only with SMV) the pointer mu.
    // one workgroup per 8 rows of a split q-block: 32 lanes x float4 cover d = 128
    const int rows_per_blk = 8, groups = kBM / rows_per_blk;
    const int blk = blockIdx.x / groups, rowgrp = blockIdx.x % groups;      // blk = (bh, rq)
    const int rq = blk % P.R, bh = blk / P.R;
    const int b = bh / P.H, h = bh % P.H;
    const int qb = P.nfull + rq;
    const int lane32 = threadIdx.x & 31, row = rowgrp * rows_per_blk + (threadIdx.x >> 5);
    const int64_t piece0 = ((int64_t)bh * P.R + rq) * P.S;
    const int64_t qrow = (int64_t)qb * kBM + row;
    if (qrow >= P.Nq) return;
    float mmax = -INFINITY;
    for (int sp = 0; sp < P.S; ++sp) mmax = fmaxf(mmax, P.ml_part[((piece0 + sp) * kBM + row) * 2]);
    float denom = 0.f;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int sp = 0; sp < P.S; ++sp) {
        const float* ml = P.ml_part + ((piece0 + sp) * kBM + row) * 2;
        const float w = fast_exp2((ml[0] - mmax) * P.scale_log2e);
        denom += w * ml[1];
        const f32x4 ov = *reinterpret_cast<const f32x4*>(P.o_part + ((piece0 + sp) * kBM + row) * kD + lane32 * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += w * ov[j];
    }
    const float inv = 1.0f / denom;
    bf16x4 w4;
    if constexpr (SMV) {      // as the direct store of attn_fwd_body.inc: product, sum, one rounding
        const f32x4 m4 = *reinterpret_cast<const f32x4*>(mu + (int64_t)h * kD + lane32 * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) w4[j] = (bf16)__fadd_rn(__fmul_rn(acc[j], inv), m4[j]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) w4[j] = (bf16)(acc[j] * inv);
    }
    *reinterpret_cast<bf16x4*>(P.out + ((int64_t)b * P.Nq + qrow) * ((int64_t)P.H * kD) + (int64_t)h * kD + lane32 * 4) = w4;
