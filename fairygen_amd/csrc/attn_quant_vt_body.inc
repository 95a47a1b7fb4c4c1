// The body of attn_quant_vt_kernel (attn_pv8.hip), included by that kernel, by its batched form and by the smoothing form (they see v, ldv, parts, v8t, sv, N, Nkp and H; the constant SMV; the plain forms read rec, the smoothing form rsum, rlo, rhi and writes mu): all compile the same text.
    __shared__ float red_s[kD];
    __shared__ float sv_s[kD];
    __shared__ __attribute__((aligned(16))) uint32_t img[kD][16];
    const int h = blockIdx.y, tid = threadIdx.x, C = H * kD;
    float m[8] = {};
    if constexpr (SMV) {      // the key mean from the fp64 sums, the scale from the minimum and maximum of v around it
        __shared__ double sum_s[kD];
        __shared__ float lo_s[kD];
        __shared__ float mu_s[kD];
        const int c = tid & (kD - 1), g = tid >> 7;
        double a = 0.0;
        float lo = INFINITY, hi = -INFINITY;
        for (int p = g; p < parts; p += 2) {
            const int64_t at = (int64_t)p * C + h * kD + c;
            a += rsum[at];
            lo = fminf(lo, rlo[at]);
            hi = fmaxf(hi, rhi[at]);
        }
        if (g == 1) {
            sum_s[c] = a;
            lo_s[c] = lo;
            red_s[c] = hi;
        }
        __syncthreads();
        if (g == 0) {
            const float m = (float)((a + sum_s[c]) / (double)N);
            const float dmax = fmaxf(fmaxf(hi, red_s[c]) - m, m - fminf(lo, lo_s[c]));      // fl32(v - m) is monotone in v
            const float s = fmaxf(dmax / kE4M3Max, kScaleFloor);
            sv_s[c] = s;
            mu_s[c] = m;
            if (blockIdx.x == 0) {
                sv[h * kD + c] = s;
                mu[h * kD + c] = m;
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) m[j] = mu_s[(tid & 15) * 8 + j];      // the 8 channels of this thread's chunk (cl below)
    } else {
        const int c = tid & (kD - 1), g = tid >> 7;
        float a = 0.f;
        for (int p = g; p < parts; p += 2) a = fmaxf(a, rec[(int64_t)p * C + h * kD + c]);
        if (g == 1) red_s[c] = a;
        __syncthreads();
        if (g == 0) {
            const float s = fmaxf(fmaxf(a, red_s[c]) / kE4M3Max, kScaleFloor);
            sv_s[c] = s;
            if (blockIdx.x == 0) sv[h * kD + c] = s;
        }
        __syncthreads();
    }
    const int cl = tid & 15, kg = tid >> 4;
    float s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = sv_s[cl * 8 + j];
    const int wr = pv8_dword(kg) ^ cl;
    const int64_t nt = Nkp / kTileKeys;
    for (int64_t t = blockIdx.x; t < nt; t += gridDim.x) {
        float f[4][8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t key = t * kTileKeys + 4 * kg + i;
            bf16x8 x = {};
            if (key < N) x = *reinterpret_cast<const bf16x8*>(v + key * ldv + (int64_t)h * kD + cl * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) {      // the padding keys of the last tile: zero bytes
                if constexpr (SMV) f[i][j] = key < N ? (float)x[j] - m[j] : 0.f;
                else f[i][j] = key < N ? (float)x[j] : 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            img[cl * 8 + j][wr] = cvt2_e4m3(f[0][j] / s[j], f[1][j] / s[j]) | (cvt2_e4m3(f[2][j] / s[j], f[3][j] / s[j]) << 16);
        __syncthreads();
        pv8_store_tile(img, v8t, h, Nkp, t, tid);
        __syncthreads();
    }
