// The body of rmsnorm_rope_q8_kernel (attn_qk8_fused.hip), included by that kernel and by its batched form (they see x, ldx, w, ctv, stv, q8, sq, rows, C and eps): both compile the same text.
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nvec = C >> 3, H = C >> 7;
    Row r;
    load_row(x + row * ldx, C, lane, r);
    const RopeRow rr = rope_begin<F32TAB, true>(r, ctv, row, C, kD, eps, lane);
#pragma unroll
    for (int i = 0; i < kMaxVec; ++i) {
        const int vi = lane + i * 64;
        if (vi < nvec) {         // nvec is a multiple of 16: the 16 lanes of a head are in or out together
            float o[8];
            rope_vec<F32TAB, true>(rr, r.v[i], ld8(w + (int64_t)vi * 8), ctv, stv, row, kD, vi, o);
            float amax = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(o[j]));
#pragma unroll
            for (int s = 8; s > 0; s >>= 1) amax = fmaxf(amax, __shfl_xor(amax, s, 64));
            const float s_q = fmaxf(amax / kE4M3Max, kScaleFloor);
            *reinterpret_cast<u32x2*>(q8 + row * C + (int64_t)vi * 8) = quant8_e4m3(o, s_q);
            if ((lane & 15) == 0) sq[row * H + (vi >> 4)] = s_q;
        }
    }
