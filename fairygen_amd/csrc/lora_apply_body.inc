    // The body of lora_apply_kernel<RT, GC> and of its batched form (lora.hip): `P` is the LoraParams of ONE element.
    constexpr int R = 32 * RT, NT = RT * GC;      // NT rank tiles per pass
    extern __shared__ __attribute__((aligned(16))) char smem_lora[];
    constexpr int kRedBytes = 2 * NT * 16 * 64 * 4;                            // one wave's partial sums: 2 * NT tiles x 16 registers x 64 lanes of fp32
    float* red = reinterpret_cast<float*>(smem_lora);
    bf16* tl = reinterpret_cast<bf16*>(smem_lora + kRedBytes);                 // t: (64, ldt) bf16
    const int ldt = P.G * R + kTPad;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 31, lh = lane >> 5;
    const int64_t m0 = (int64_t)blockIdx.x * kRows;

    // ---------------------------------------------------------------- phase 1: t = bf16(x A^T), rows m0 .. m0 + 63
    const bf16* xrow[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        int64_t row = m0 + 32 * mt + lr;
        row = row < P.M ? row : (int64_t)P.M - 1;      // rows past M: a valid address, the results are never stored
        xrow[mt] = P.x + row * P.ldx + 32 * lh;
    }
    const int chunks = P.K / 64;
    for (int pass = 0; pass < P.G / GC; ++pass) {
        const bf16* arow = P.a + ((int64_t)pass * NT * 32 + lr) * P.K + 32 * lh;
        f32x16 acc[2][NT];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int rt = 0; rt < NT; ++rt)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[mt][rt][i] = 0.f;
        // a wave's chunks are c = wave, wave + 4, ...; an iteration takes half a chunk (MFMA steps 2i' and 2i' + 1: 32 bytes per lane and row),
        // which keeps the double-buffered fragments small enough for two waves per SIMD
        bf16x8 xf[2][2], af[NT][2];
        auto load = [&](int it) {
            const int off = (wave + 4 * (it >> 1)) * 64 + 16 * (it & 1);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) xf[mt][s] = *reinterpret_cast<const bf16x8*>(xrow[mt] + off + 8 * s);
#pragma unroll
                for (int rt = 0; rt < NT; ++rt) af[rt][s] = *reinterpret_cast<const bf16x8*>(arow + (int64_t)rt * 32 * P.K + off + 8 * s);
            }
        };
        const int iters = wave < chunks ? 2 * ((chunks - wave + 3) / 4) : 0;
        if (iters > 0) load(0);
        for (int it = 0; it < iters; ++it) {
            bf16x8 xc[2][2], ac[NT][2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) xc[mt][s] = xf[mt][s];
#pragma unroll
                for (int rt = 0; rt < NT; ++rt) ac[rt][s] = af[rt][s];
            }
            if (it + 1 < iters) load(it + 1);      // the next half chunk's loads fly under this one's MFMAs
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int rt = 0; rt < NT; ++rt)
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
                        acc[mt][rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ac[rt][s], xc[mt][s], acc[mt][rt], 0, 0, 0);
        }
        // wave 0 += wave 1, 2, 3 (fp32, fixed order); the partials keep their register layout, so the buffer is indexed [register][lane]
        for (int w = 1; w < 4; ++w) {
            if (wave == w) {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int rt = 0; rt < NT; ++rt)
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const f32x4 v = {acc[mt][rt][4 * q], acc[mt][rt][4 * q + 1], acc[mt][rt][4 * q + 2], acc[mt][rt][4 * q + 3]};
                            reinterpret_cast<f32x4*>(red)[(((mt * NT + rt) * 4 + q) * 64) + lane] = v;
                        }
            }
            __syncthreads();
            if (wave == 0) {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int rt = 0; rt < NT; ++rt)
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const f32x4 v = reinterpret_cast<const f32x4*>(red)[(((mt * NT + rt) * 4 + q) * 64) + lane];
#pragma unroll
                            for (int i = 0; i < 4; ++i) acc[mt][rt][4 * q + i] += v[i];
                        }
            }
            __syncthreads();
        }
        // register 4q + i of lane (lr, lh) is t^T[rank 8q + 4lh + i][row lr] of its tile: 4 consecutive ranks of one row -> 8 bytes of t
        if (wave == 0) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int rt = 0; rt < NT; ++rt)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const u32x2 v = {pack_bf16x2(acc[mt][rt][4 * q], acc[mt][rt][4 * q + 1]), pack_bf16x2(acc[mt][rt][4 * q + 2], acc[mt][rt][4 * q + 3])};
                        *reinterpret_cast<u32x2*>(tl + (32 * mt + lr) * ldt + (pass * NT + rt) * 32 + 8 * q + 4 * lh) = v;
                    }
        }
    }
    __syncthreads();

    // ---------------------------------------------------------------- phase 2: out = epi(out, bf16(t B^T)) in 64-column blocks
    const int nblk = P.Ng / 64, mode = P.mode;
    int64_t orow[2];
    bool live[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int64_t row = m0 + 32 * mt + lr;
        live[mt] = row < P.M;
        orow[mt] = (live[mt] ? row : (int64_t)P.M - 1);
    }
    for (int u = wave; u < P.G * nblk; u += 4) {
        const int g = u / nblk, nb = u - g * nblk;
        const int64_t col0 = (int64_t)g * P.Ng + nb * 64 + 8 * lh;      // this lane's first column after the half-wave swap
        // the old values at the columns this lane will own after the swap: quad pair q of tile nt = columns 32nt + 16q + 8lh + 0..7
        u32x4 ov[2][2][2];
        if (mode != 0) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                    for (int q = 0; q < 2; ++q) ov[mt][nt][q] = *reinterpret_cast<const u32x4*>(P.out + orow[mt] * P.ldc + col0 + 32 * nt + 16 * q);
        }
        f32x16 acc[2][2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[mt][nt][i] = 0.f;
        const bf16* brow = P.b + ((int64_t)g * P.Ng + nb * 64 + lr) * R + 8 * lh;
        const bf16* trow = tl + lr * ldt + g * R + 8 * lh;
#pragma unroll
        for (int s = 0; s < 2 * RT; ++s) {
            bf16x8 bfr[2], tf[2];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) bfr[nt] = *reinterpret_cast<const bf16x8*>(brow + (int64_t)nt * 32 * R + 16 * s);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) tf[mt] = *reinterpret_cast<const bf16x8*>(trow + mt * 32 * ldt + 16 * s);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bfr[nt], tf[mt], acc[mt][nt], 0, 0, 0);
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    // quads 2q and 2q + 1 (columns 16q + 4lh + 0..3 and 16q + 8 + 4lh + 0..3 of row lr), rounded to bf16, then paired across the halves
                    uint32_t a0 = pack_bf16x2(acc[mt][nt][8 * q], acc[mt][nt][8 * q + 1]), a1 = pack_bf16x2(acc[mt][nt][8 * q + 2], acc[mt][nt][8 * q + 3]);
                    uint32_t b0 = pack_bf16x2(acc[mt][nt][8 * q + 4], acc[mt][nt][8 * q + 5]), b1 = pack_bf16x2(acc[mt][nt][8 * q + 6], acc[mt][nt][8 * q + 7]);
                    const auto r0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
                    const auto r1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
                    const u32x4 lw = {r0[0], r1[0], r0[1], r1[1]};
                    const bf16x8 l8 = __builtin_bit_cast(bf16x8, lw);
                    bf16x8 o8 = l8;
                    if (mode != 0) {
                        const bf16x8 old = __builtin_bit_cast(bf16x8, ov[mt][nt][q]);
                        if (mode == 2) {
                            // the gate table is a few KiB and stays in L2: read here rather than held across the MFMAs
                            const bf16x8 g8 = *reinterpret_cast<const bf16x8*>(P.gate + (orow[mt] >= P.first_rows ? P.gate_ld : 0) + col0 + 32 * nt + 16 * q);
#pragma unroll
                            for (int j = 0; j < 8; ++j) o8[j] = (bf16)((float)old[j] + rbf((float)g8[j] * (float)l8[j]));
                        } else if (mode == 4) {
#pragma unroll
                            for (int j = 0; j < 8; ++j) o8[j] = (bf16)gelu_tanh_epilogue(rbf((float)old[j] + (float)l8[j]));
                        } else {
#pragma unroll
                            for (int j = 0; j < 8; ++j) o8[j] = (bf16)((float)old[j] + (float)l8[j]);
                        }
                    }
                    if (live[mt]) *reinterpret_cast<bf16x8*>(P.out + orow[mt] * P.ldc + col0 + 32 * nt + 16 * q) = o8;
                }
    }
