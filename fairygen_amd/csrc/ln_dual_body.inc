    // The body of ln_dual_kernel<MODE> and of its batched form (dit_elementwise.hip): one element's pointers and rows.
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= rows) return;
    Row r;
    load_row(x + row * C, C, lane, r);
    const int64_t m = MODE == 0 ? mod_row(row, mod_rows, first_rows) : 0;
    norm_store_fp8<MODE, true>(r, C, lane, eps, p0 + m * mod_ld, p1 + m * mod_ld, out8 + row * C, scale_out + row, fp8_max, out + row * C);
