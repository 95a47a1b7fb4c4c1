// The body of gemm_reduce_kernel and gemm_reduce_pg_kernel (dit_gemm.hip): P (GemmPParams) and per are the including kernel's, and
// FG_GEMM_REDUCE_ROW1 its rule for "this row reads gate row 1" (in scope: row, m0).
    const int chunk = blockIdx.x & 15, wave = (blockIdx.x >> 4) & 3;
    int q = blockIdx.x >> 6, xcd = 0;      // q-th k-split tile of the launch -> (xcd, t)
    for (; xcd < (int)P.s.nxcd; ++xcd) {
        const TailPlan tp(P.total, xcd, (int)P.s.nxcd, per, (int)P.s.nk, true, 1);
        const int n = tp.split > 1 ? tp.rem : 0;
        if (q < n) break;
        q -= n;
    }
    if (xcd == (int)P.s.nxcd) return;
    const TailPlan tp(P.total, xcd, (int)P.s.nxcd, per, (int)P.s.nk, true, 1);
    const int logical = tp.start + tp.full * per + q, GM = P.group_m;
    const int group = logical / (GM * (int)P.s.tiles_n), in_group = logical % (GM * (int)P.s.tiles_n);
    const int gm = ((int)P.s.tiles_m - group * GM) < GM ? ((int)P.s.tiles_m - group * GM) : GM;
    const int mt = group * GM + in_group % gm, nt = in_group / gm;
    const int64_t m0 = (int64_t)mt * 256, n0 = (int64_t)nt * 256;
    const f32x4* ws = reinterpret_cast<const f32x4*>((const char*)P.s.workspace + (int64_t)(xcd * per + q * tp.split) * kPieceBytes);
    {
        const int item = chunk * 256 + threadIdx.x;
        const int st = item >> 6, lane = item & 63, blk = st >> 2, g = st & 3, ni = blk >> 2, mi = blk & 3;
        const int64_t row = m0 + 128 * (wave & 1) + 32 * mi + (lane & 31);
        if (row >= (int64_t)P.s.M) return;
        const int64_t col = n0 + 128 * (wave >> 1) + 32 * ni + 8 * g + 4 * (lane >> 5);
        const f32x4* src = ws + (wave * 64 + st) * 64 + lane;
        f32x4 acc = src[0];
        int p = 1;
        for (; p + 4 <= tp.split; p += 4) {      // four loads in flight, added in k order
            const f32x4 v0 = src[(int64_t)p * (kPieceBytes / 16)], v1 = src[(int64_t)(p + 1) * (kPieceBytes / 16)];
            const f32x4 v2 = src[(int64_t)(p + 2) * (kPieceBytes / 16)], v3 = src[(int64_t)(p + 3) * (kPieceBytes / 16)];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = ((acc[j] + v0[j]) + v1[j]) + v2[j] + v3[j];
        }
        for (; p < tp.split; ++p) {
            const f32x4 v = src[(int64_t)p * (kPieceBytes / 16)];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += v[j];
        }
        if (P.s.scale != nullptr) {      // e4m3 form: (acc * scale_a) is one fp32 operation of torch._scaled_mm, the bias add the next
            const float sa = P.s.scale[row];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] *= sa;
        }
        bf16* cp = P.s.c + row * (int64_t)(P.s.ldc_bytes / 2) + col;
        const bf16x4 bv = *reinterpret_cast<const bf16x4*>(P.s.bias + col);
        bf16x4 xv = {(bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f}, gv = xv, out;
        if (P.s.flags == 2 || P.s.flags == 3) xv = *reinterpret_cast<const bf16x4*>(cp);
        if (P.s.flags == 2) gv = *reinterpret_cast<const bf16x4*>(P.s.gate + (FG_GEMM_REDUCE_ROW1 ? P.s.gate_ld_bytes / 2 : 0) + col);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float y = rbf(acc[j] + (float)bv[j]);
            out[j] = (bf16)(P.s.flags == 2 ? (float)xv[j] + rbf((float)gv[j] * y) : P.s.flags == 3 ? (float)xv[j] + y : P.s.flags == 4 ? gelu_tanh_epilogue(y) : y);
        }
        *reinterpret_cast<bf16x4*>(cp) = out;
    }
