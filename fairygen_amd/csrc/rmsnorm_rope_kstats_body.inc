// The body of rmsnorm_rope_kstats_kernel (attn_qk8_fused.hip), included by that kernel and by its batched form (they see x, ldx, w, ctv, stv, out, psum, pmin, pmax, rows, C and eps): both compile the same text.
    __shared__ double sum_s[NV * 512];       // [vector slot][element][lane]: conflict-free
    __shared__ float min_s[NV * 512], max_s[NV * 512];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nvec = C >> 3;
    double sum[NV][8];
    float mn[NV][8], mx[NV][8];
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            sum[i][j] = 0.0;
            mn[i][j] = INFINITY;
            mx[i][j] = -INFINITY;
        }
    for (int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + wave; row < rows; row += (int64_t)gridDim.x * kRowsPerBlock) {
        RowT<NV> r;
        load_row(x + row * ldx, C, lane, r);
        const RopeRow rr = rope_begin<F32TAB, true>(r, ctv, row, C, kD, eps, lane);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int vi = lane + i * 64;
            if (vi < nvec) {
                float o[8];
                rope_vec<F32TAB, true>(rr, r.v[i], ld8(w + (int64_t)vi * 8), ctv, stv, row, kD, vi, o);
                st8(out + row * C + (int64_t)vi * 8, o);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    sum[i][j] += (double)o[j];
                    mn[i][j] = fminf(mn[i][j], o[j]);
                    mx[i][j] = fmaxf(mx[i][j], o[j]);
                }
            }
        }
    }
    for (int wv = 1; wv < kRowsPerBlock; ++wv) {
        if (wave == wv) {
#pragma unroll
            for (int i = 0; i < NV; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    sum_s[(i * 8 + j) * 64 + lane] = sum[i][j];
                    min_s[(i * 8 + j) * 64 + lane] = mn[i][j];
                    max_s[(i * 8 + j) * 64 + lane] = mx[i][j];
                }
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int i = 0; i < NV; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    sum[i][j] += sum_s[(i * 8 + j) * 64 + lane];
                    mn[i][j] = fminf(mn[i][j], min_s[(i * 8 + j) * 64 + lane]);
                    mx[i][j] = fmaxf(mx[i][j], max_s[(i * 8 + j) * 64 + lane]);
                }
        }
        __syncthreads();
    }
    if (wave != 0) return;
    const int64_t base = (int64_t)blockIdx.x * C;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int vi = lane + i * 64;
        if (vi < nvec) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                psum[base + vi * 8 + j] = sum[i][j];
                pmin[base + vi * 8 + j] = mn[i][j];
                pmax[base + vi * 8 + j] = mx[i][j];
            }
        }
    }
