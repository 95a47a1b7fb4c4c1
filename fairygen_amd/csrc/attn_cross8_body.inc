// The body of attn_cross8_kernel (attn_cross8.hip, which describes it), included by that kernel and by its batched form
// attn_cross8_b_kernel, and by the smoothed-V forms of the two: all see `const Cross8Params P`, the constant SMV and (read only with SMV)
// the pointer mu, and compile the same text.
    extern __shared__ __attribute__((aligned(16))) char smem[];      // K8 tiles 0 .. nt - 1, then V8^T tiles 0 .. nt - 1
    const int64_t Nq = P.Nq, Nkv = P.Nkv;
    const int H = P.H;
    const int nt = (int)(P.Nkp / kTileKeys);
    char* const k_lds = smem;
    char* const v_lds = smem + nt * kTile8Bytes;
    const int h = blockIdx.x / P.G, g0 = blockIdx.x % P.G;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int64_t hd8 = (int64_t)H * kD;      // row pitch of q8 / k8 in bytes

    // ---- the head's K8 and V8^T into LDS, once.  Per tile a thread moves one 16-byte chunk of each: K8 row t >> 3, chunk t & 7 (a key row
    // >= Nkv is not read and becomes zeros); V8^T channel row t >> 2, chunk t & 3 (the padding of the last tile is the producer's zeros).
    {
        const uint8_t* kg = P.k8 + (int64_t)h * kD + (int64_t)(tid >> 3) * hd8 + (tid & 7) * 16;
        const uint8_t* vg = P.v8t + ((int64_t)h * kD + (tid >> 2)) * P.Nkp + (tid & 3) * 16;
        const int ko = k8_lds_off(tid >> 3, tid & 7), vo = v8_lds_off(tid >> 2, tid & 3);
        for (int t0 = 0; t0 < nt; t0 += 4) {      // 4 tiles in flight
            u32x4 kr[4], vr[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = t0 + i;
                kr[i] = u32x4{0u, 0u, 0u, 0u};
                vr[i] = u32x4{0u, 0u, 0u, 0u};
                if (t < nt) {
                    if ((int64_t)t * kTileKeys + (tid >> 3) < Nkv) kr[i] = *reinterpret_cast<const u32x4*>(kg + (int64_t)t * kTileKeys * hd8);
                    vr[i] = *reinterpret_cast<const u32x4*>(vg + (int64_t)t * kTileKeys);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = t0 + i;
                if (t < nt) {
                    *reinterpret_cast<u32x4*>(k_lds + t * kTile8Bytes + ko) = kr[i];
                    *reinterpret_cast<u32x4*>(v_lds + t * kTile8Bytes + vo) = vr[i];
                }
            }
        }
    }
    __syncthreads();      // the only barrier

    // ---- loop-invariant per-lane LDS read addresses (tile t: + t * kTile8Bytes)
    // K8: MFMA m = 2 sub + ks reads chunks 4 ks + 2 hh and + 1 of row 32 sub + r (+ 4096 B for sub 1)
    int k8_rd[2][2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int c = 0; c < 2; ++c) k8_rd[ks][c] = k8_lds_off(r, 4 * ks + 2 * hh + c);
    union Q8F { u32x4 h2[2]; i32x8 f; };
    auto read_k8 = [&](const char* kb, int m) {
        Q8F a;
        a.h2[0] = *reinterpret_cast<const u32x4*>(kb + k8_rd[m & 1][0] + (m >> 1) * 4096);
        a.h2[1] = *reinterpret_cast<const u32x4*>(kb + k8_rd[m & 1][1] + (m >> 1) * 4096);
        return a.f;
    };
    // V8^T: the fragment of channel block db is chunks 2 hh and 2 hh + 1 of row 32 db + r (+ 2048 B per db; the swizzle is r's)
    const int v8_rd[2] = {v8_lds_off(r, 2 * hh), v8_lds_off(r, 2 * hh + 1)};
    auto read_v8 = [&](const char* vb, int db) {
        Q8F a;
        a.h2[0] = *reinterpret_cast<const u32x4*>(vb + v8_rd[0] + db * 2048);
        a.h2[1] = *reinterpret_cast<const u32x4*>(vb + v8_rd[1] + db * 2048);
        return a.f;
    };
    auto mfma8 = [](i32x8 a, i32x8 bq, f32x16 c) { return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, bq, c, 0, 0, 0, 0, 0, 0); };
    const float sk_h = P.sk[h];
    const float* const svp = P.sv + (int64_t)h * kD + 4 * hh;

    for (int qb = g0; qb < P.nqb; qb += P.G) {
        // ---- Q8^T fragments (B operand of S^T = K8 Q8^T): lane (r, hh) holds bytes 64 ks + 32 hh + 0..31 of its row
        int64_t my_q = (int64_t)qb * kBM + wave * 32 + r;
        const bool q_valid = my_q < Nq;
        if (!q_valid) my_q = Nq - 1;
        Q8F qf8[2];
        {
            const uint8_t* q8row = P.q8 + my_q * hd8 + (int64_t)h * kD;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                qf8[ks].h2[0] = *reinterpret_cast<const u32x4*>(q8row + 64 * ks + 32 * hh);
                qf8[ks].h2[1] = *reinterpret_cast<const u32x4*>(q8row + 64 * ks + 32 * hh + 16);
            }
        }
        // scale * log2(e) in the units of this lane's scores
        const float row_unit = P.sq[my_q * H + h] * sk_h;
        const float scale_log2e = P.scale_log2e * row_unit;

        f32x16 o[4];
        float m_run = -INFINITY, l_run = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 16; ++j) o[i][j] = 0.f;

        // s[sub][reg] = score(key = 64 t + 32 sub + (reg & 3) + 8 (reg >> 2) + 4 hh, query row r)
        auto mask_tile = [&](f32x16 (&s)[2], int t) {
            const int64_t kbase = (int64_t)t * kTileKeys + 4 * hh;
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (kbase + 32 * sub + (j & 3) + 8 * (j >> 2) >= Nkv) s[sub][j] = -INFINITY;
        };
        auto tile_max = [&](const f32x16 (&s)[2]) {
            float mt = max3(s[0][0], s[1][0], s[0][1]);
#pragma unroll
            for (int j = 1; j < 15; ++j) mt = max3(mt, s[1][j], s[0][j + 1]);
            return pair_max(fmaxf(mt, s[1][15]));
        };
        // Deferred rescale: keep the stale max while no row of the wave outgrew it by more than 2^T.
        auto absorb_max = [&](float mt) {
            const bool grow = (mt - m_run) * scale_log2e > kPv8DeferLog2;
            if (__builtin_amdgcn_ballot_w64(grow) != 0) {
                const float m_new = fmaxf(m_run, mt);
                const float alpha = fast_exp2((m_run - m_new) * scale_log2e);
                m_run = m_new;
                l_run *= alpha;
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 16; ++j) o[i][j] *= alpha;
            }
        };

        // One step for tile t as 32 MFMA gaps (every 4th holds one 32x32x64 MFMA: 4 of S^T(t+1), then 4 of O^T += V8(t)^T P8(t)^T), the
        // other work dealt out between them in program order and pinned by sched_barrier: two exponentials of tile t per QK gap, a dword
        // of P8 in the even gaps 2..16, the K8 / V8^T fragment reads 3 gaps ahead of their MFMA, and (kMode 0) the row max of tile t+1
        // under the PV gaps.  kMode 0: tile t+1 exists and is full; 1: it exists, maybe ragged (mask and max after the gaps); 2: t is the
        // last tile (no S^T MFMAs).
        auto step = [&](f32x16 (&sc)[2], f32x16 (&sn)[2], int t, auto mode_tag) {
            constexpr int kMode = decltype(mode_tag)::value;
            const char* kb = k_lds + (t + 1) * kTile8Bytes;
            const char* vb = v_lds + t * kTile8Bytes;
            const float mb = m_run * scale_log2e - kPv8Log2C;
            float ps0 = 0.f, ps1 = 0.f, mt = 0.f;
            float pe[32];
            i32x8 ka8[4], va8[4];
            union PF8 { uint32_t w[8]; i32x8 f; } pf8;
            auto do_exp = [&](int e) {
                const float p = fast_exp2(sc[e >> 4][e & 15] * scale_log2e - mb);
                pe[e] = p;
            };
            // Row-sum add as opaque asm, one gap AFTER the exponential (a transcendental needs a wait state before a VALU reader of its
            // result, and the compiler's hazard pass does not look inside inline asm).
            auto do_add = [&](int e) { if (e & 1) ps1 = add_f32(ps1, pe[e]); else ps0 = add_f32(ps0, pe[e]); };
            // dword w of the B operand = exponentials 4 w .. 4 w + 3 (c p <= 2^8: no clamp)
            auto do_pack8 = [&](int w) {
                const int lo = __builtin_amdgcn_cvt_pk_fp8_f32(pe[4 * w], pe[4 * w + 1], 0, false);
                pf8.w[w] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(pe[4 * w + 2], pe[4 * w + 3], lo, true);
            };
            if constexpr (kMode < 2) ka8[0] = read_k8(kb, 0);
            __builtin_amdgcn_sched_barrier(0);
            static_for<0, 32>([&](auto gc) {
                constexpr int g = decltype(gc)::value;
                constexpr int e0 = exps_before(g), e1 = exps_before(g + 1);
                constexpr int ep = g == 0 ? 0 : exps_before(g - 1);
                if constexpr ((g & 1) == 0 && g >= 2 && g <= 16) do_pack8(g / 2 - 1);
                if constexpr (g < 16) {
                    if constexpr (kMode < 2) {
                        constexpr int sub = g >> 3;
                        if constexpr ((g & 7) == 0) {
#pragma unroll
                            for (int j = 0; j < 16; ++j) sn[sub][j] = 0.f;
                        }
                        if constexpr ((g & 3) == 0) sn[sub] = mfma8(ka8[g >> 2], qf8[(g >> 2) & 1].f, sn[sub]);
                        if constexpr ((g & 3) == 1 && g < 12) ka8[(g >> 2) + 1] = read_k8(kb, (g >> 2) + 1);
                    }
                } else {
                    if constexpr ((g & 3) == 0) o[(g - 16) >> 2] = mfma8(va8[(g - 16) >> 2], pf8.f, o[(g - 16) >> 2]);
                }
                if constexpr ((g & 3) == 1 && g >= 13 && g < 29) va8[(g - 13) >> 2] = read_v8(vb, (g - 13) >> 2);
                if constexpr (e1 > e0) do_exp(e0);
                if constexpr (e1 > e0 + 1) do_exp(e0 + 1);
                if constexpr (e0 > ep) do_add(ep);
                if constexpr (e0 > ep + 1) do_add(ep + 1);
                if constexpr (kMode == 0 && g >= 17) {      // 15 max3 steps in gaps 17..31 (scores of tile t+1 complete after gap 15)
                    constexpr int i = g - 17;
                    if constexpr (i == 0) mt = max3(sn[0][0], sn[1][0], sn[0][1]);
                    else mt = max3(mt, sn[1][i], sn[0][i + 1]);
                }
                __builtin_amdgcn_sched_barrier(0);
            });
            l_run += ps0 + ps1;
            if constexpr (kMode == 0) {
                absorb_max(pair_max(fmaxf(mt, sn[1][15])));
            } else if constexpr (kMode == 1) {
                if ((int64_t)(t + 2) * kTileKeys > Nkv) mask_tile(sn, t + 1);      // ragged last tile (wave-uniform)
                absorb_max(tile_max(sn));
            }
        };

        // ---- prologue: the scores of tile 0 and their max
        f32x16 sA[2], sB[2];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
            for (int j = 0; j < 16; ++j) sA[sub][j] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) sA[sub] = mfma8(read_k8(k_lds, 2 * sub + ks), qf8[ks].f, sA[sub]);
        }
        if ((int64_t)kTileKeys > Nkv) mask_tile(sA, 0);
        m_run = tile_max(sA);

        // fast steps: the next tile exists and is full
        const int t_fast = min(nt - 1, (int)(Nkv / kTileKeys) - 1);
        int t = 0;
        for (; t + 1 < t_fast; t += 2) {
            step(sA, sB, t, std::integral_constant<int, 0>{});
            step(sB, sA, t + 1, std::integral_constant<int, 0>{});
        }
        for (; t + 1 < nt; ++t) {      // <= 2 steps: odd fast step, ragged-next step
            step(sA, sB, t, std::integral_constant<int, 1>{});
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) sA[sub] = sB[sub];
        }
        step(sA, sB, t, std::integral_constant<int, 2>{});

        // ---- epilogue: lane holds O[query r][d = 32 db + 8 g + 4 hh + 0..3]
        const float l_tot = pair_sum(l_run);
#pragma unroll
        for (int db = 0; db < 4; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 s4 = *reinterpret_cast<const f32x4*>(svp + 32 * db + 8 * g);
#pragma unroll
                for (int j = 0; j < 4; ++j) o[db][4 * g + j] *= s4[j];
            }
        const float inv = 1.0f / l_tot;
        if (q_valid) {
            bf16* orow = P.out + my_q * hd8 + (int64_t)h * kD;
#pragma unroll
            for (int db = 0; db < 4; ++db)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    bf16x4 w4;
                    if constexpr (SMV) {      // + the key mean of the channel: a product, then a sum, then the one rounding to bf16
                        const f32x4 m4 = *reinterpret_cast<const f32x4*>(mu + (int64_t)h * kD + 32 * db + 8 * g + 4 * hh);
#pragma unroll
                        for (int j = 0; j < 4; ++j) w4[j] = (bf16)__fadd_rn(__fmul_rn(o[db][4 * g + j], inv), m4[j]);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) w4[j] = (bf16)(o[db][4 * g + j] * inv);
                    }
                    *reinterpret_cast<bf16x4*>(orow + 32 * db + 8 * g + 4 * hh) = w4;
                }
        }
    }
