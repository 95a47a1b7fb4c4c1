// The body of rmsnorm_rope_kernel<F32TAB, PLAIN> and rmsnorm_rope_b_kernel<F32TAB, PLAIN> (dit_elementwise.hip): x, out the rows of ONE
// element, the RoPE table indexed by the row inside it.  Names it reads: x, ldx, w, ctv, stv, out, rows, C, head_dim, eps, group_cols,
// out_group_stride, out_ld and the template parameters.
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= rows) return;
    Row r;
    load_row(x + row * ldx, C, lane, r);
    const int nvec = C >> 3;
    const RopeRow rr = rope_begin<F32TAB, PLAIN>(r, ctv, row, C, head_dim, eps, lane);
#pragma unroll
    for (int i = 0; i < kMaxVec; ++i) {
        const int vi = lane + i * 64;
        if (vi < nvec) {
            float o[8];
            rope_vec<F32TAB, PLAIN>(rr, r.v[i], ld8(w + (int64_t)vi * 8), ctv, stv, row, head_dim, vi, o);
            // column block g = col / group_cols goes to its own (rows, out_ld) plane (group_cols == C: plain rows)
            const int col = vi * 8, g = PLAIN ? 0 : col / group_cols;
            st8(out + g * out_group_stride + row * out_ld + (col - g * group_cols), o);
        }
    }
