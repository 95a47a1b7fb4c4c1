// The body of attn_k_stats_kernel (attn_qk8.hip), included by that kernel and by its batched form (they see k, ldk, kbar, sk and N): both compile the same text.
    __shared__ double red[16][kD];
    __shared__ float mean_s[kD];
    __shared__ float amax_s[16];
    const int h = blockIdx.x, tid = threadIdx.x, c = tid & 15, rl = tid >> 4, wave = tid >> 6, lane = tid & 63;
    const bf16* kp = k + (int64_t)h * kD + c * 8;
    double acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.0;
    for (int64_t row = rl; row < N; row += 64) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(kp + row * ldk);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += (double)(float)v[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        acc[j] += __shfl_xor(acc[j], 16, 64);
        acc[j] += __shfl_xor(acc[j], 32, 64);
    }
    if (lane < 16) {
#pragma unroll
        for (int j = 0; j < 8; ++j) red[wave][c * 8 + j] = acc[j];
    }
    __syncthreads();
    if (tid < kD) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < 16; ++w) s += red[w][tid];
        const float m = (float)(s / (double)N);
        mean_s[tid] = m;
        kbar[h * kD + tid] = m;
    }
    __syncthreads();
    float m[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = mean_s[c * 8 + j];
    float amax = 0.f;
    for (int64_t row = rl; row < N; row += 64) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(kp + row * ldk);
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf((float)v[j] - m[j]));
    }
    amax = wave_max(amax);
    if (lane == 0) amax_s[wave] = amax;
    __syncthreads();
    if (tid == 0) {
        float a = amax_s[0];
#pragma unroll
        for (int w = 1; w < 16; ++w) a = fmaxf(a, amax_s[w]);
        sk[h] = fmaxf(a / kE4M3Max, kScaleFloor);
    }
