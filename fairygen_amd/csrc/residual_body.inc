// The body of residual_kernel<MODE> and residual_b_kernel<MODE> (dit_elementwise.hip): x, y, x_out, norm_out (norm_fp8, norm_scale) the
// rows of ONE element, the table indexed by the row inside it.  Names it reads: x, y, gate, x_out, p0, p1, norm_out, rows, C, eps, mod_rows,
// first_rows, mod_ld, norm_fp8, norm_scale, fp8_max and the template parameter MODE.
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nvec = C >> 3;
    const int64_t m = mod_row(row, mod_rows, first_rows);
    Row r;
#pragma unroll
    for (int i = 0; i < kMaxVec; ++i) {
        const int vi = lane + i * 64;
        if (vi < nvec) {
            const bf16x8 xv = ld8(x + row * C + (int64_t)vi * 8);
            const bf16x8 yv = ld8(y + row * C + (int64_t)vi * 8);
            if (gate != nullptr) {
                const bf16x8 gv = ld8(gate + m * mod_ld + (int64_t)vi * 8);
#pragma unroll
                for (int j = 0; j < 8; ++j) r.v[i][j] = rbf((float)xv[j] + rbf((float)gv[j] * (float)yv[j]));
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) r.v[i][j] = rbf((float)xv[j] + (float)yv[j]);
            }
            st8(x_out + row * C + (int64_t)vi * 8, r.v[i]);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) r.v[i][j] = 0.f;
        }
    }
    if (norm_fp8 != nullptr) {      // the norm feeds an fp8 Linear only: e4m3 row + scale instead of the bf16 row
        if (MODE == 0) norm_store_fp8<0>(r, C, lane, eps, p0 + m * mod_ld, p1 + m * mod_ld, norm_fp8 + row * C, norm_scale + row, fp8_max);
        if (MODE == 1) norm_store_fp8<1>(r, C, lane, eps, p0, p1, norm_fp8 + row * C, norm_scale + row, fp8_max);
        return;
    }
    if (MODE == 0) norm_store<0>(r, C, lane, eps, p0 + m * mod_ld, p1 + m * mod_ld, norm_out + row * C);
    if (MODE == 1) norm_store<1>(r, C, lane, eps, p0, p1, norm_out + row * C);
