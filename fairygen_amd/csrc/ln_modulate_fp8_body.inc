// The body of ln_modulate_fp8_kernel and ln_modulate_fp8_b_kernel (dit_elementwise.hip): x, out8, scale_out the rows of ONE element, the
// table indexed by the row inside it.  Names it reads: x, shift, scale, out8, scale_out, rows, C, eps, mod_rows, first_rows, mod_ld, fp8_max.
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= rows) return;
    Row r;
    load_row(x + row * C, C, lane, r);
    const int64_t m = mod_row(row, mod_rows, first_rows);
    norm_store_fp8<0>(r, C, lane, eps, shift + m * mod_ld, scale + m * mod_ld, out8 + row * C, scale_out + row, fp8_max);
