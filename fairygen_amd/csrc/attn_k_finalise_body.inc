// The body of attn_k_finalise_kernel (attn_qk8_fused.hip), included by that kernel and by its batched form (they see psum, pmin, pmax, P, C, kbar, sk and N): both compile the same text.
    __shared__ double sum_s[8][kD];
    __shared__ float min_s[8][kD], max_s[8][kD];
    __shared__ float amax_s[2];
    const int h = blockIdx.x, tid = threadIdx.x, c = tid & (kD - 1), g = tid >> 7;
    double s = 0.0;
    float lo = INFINITY, hi = -INFINITY;
    for (int p = g; p < P; p += 8) {
        const int64_t o = (int64_t)p * C + h * kD + c;
        s += psum[o];
        lo = fminf(lo, pmin[o]);
        hi = fmaxf(hi, pmax[o]);
    }
    sum_s[g][c] = s;
    min_s[g][c] = lo;
    max_s[g][c] = hi;
    __syncthreads();
    if (tid < kD) {
#pragma unroll
        for (int i = 1; i < 8; ++i) {
            s += sum_s[i][c];
            lo = fminf(lo, min_s[i][c]);
            hi = fmaxf(hi, max_s[i][c]);
        }
        const float m = (float)(s / (double)N);
        kbar[h * kD + c] = m;
        const float amax = wave_max(fmaxf(hi - m, m - lo));
        if ((tid & 63) == 0) amax_s[tid >> 6] = amax;
    }
    __syncthreads();
    if (tid == 0) sk[h] = fmaxf(fmaxf(amax_s[0], amax_s[1]) / kE4M3Max, kScaleFloor);
