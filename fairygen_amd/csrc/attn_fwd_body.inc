// The body of attn_fwd_kernel<QK8, PV8> (attention.hip, which describes it), included by that kernel and by its batched form
// attn_fwd_b_kernel, and by the smoothed-V forms of the two: all see `const AttnParams P`, the constants QK8, PV8 and SMV and (read only
// with SMV) the pointer mu, and compile the same text.
    const bf16* __restrict__ q = P.q; const bf16* __restrict__ k = P.k; const bf16* __restrict__ v = P.v;
    bf16* __restrict__ out = P.out;
    const int64_t ldq = P.ldq, ldk = P.ldk, ldv = P.ldv, Nq = P.Nq, Nkv = P.Nkv;
    const int H = P.H;
    static_assert(!PV8 || QK8, "the e4m3 P V form extends the e4m3 QK^T form");
    static_assert(!SMV || PV8, "the smoothed-V form is a form of the e4m3 P V form");
    constexpr float kDefer = PV8 ? kPv8DeferLog2 : kDeferLog2;
    constexpr int kVBuf = PV8 ? kTile8Bytes : kTileBytes;      // bytes of one V buffer in LDS
    constexpr int THREADS = kBM / 32 * 64;         // 8 waves, 32 query rows each
    constexpr int NST = (kBN * 16) / THREADS;      // 16-byte chunks per thread per bf16 tile (2; the e4m3 tiles: 1)
    constexpr int ST_ROWS = THREADS / 16;          // rows covered per staging pass
    __shared__ __attribute__((aligned(16))) char smem[2 * kTileBytes + 2 * kVBuf];  // K0 K1 V0 V1 (e4m3 P V form: 48 KiB, else 64)
    char* const k_lds = smem;
    char* const v_lds = smem + 2 * kTileBytes;

    const int nt = (int)((Nkv + kBN - 1) / kBN);
    int qb, bh, t_begin = 0, t_end = nt, piece = -1;
    if ((int)blockIdx.x < P.total_direct) {
        // XCD-aware remap: blocks b and b+8 share an XCD; give each XCD a contiguous logical range (of heads).
        const int bid = blockIdx.x, xcd = bid & 7, slot = bid >> 3;
        const int qd = P.total_direct >> 3, rm = P.total_direct & 7;
        const int logical = (xcd < rm ? xcd * (qd + 1) : rm * (qd + 1) + (xcd - rm) * qd) + slot;
        qb = logical % P.nfull;
        bh = logical / P.nfull;      // b*H + h
    } else {
        piece = (int)blockIdx.x - P.total_direct;
        const int sp = piece % P.S, rq = (piece / P.S) % P.R;
        bh = piece / (P.S * P.R);
        qb = P.nfull + rq;
        t_begin = (int)((int64_t)sp * nt / P.S);
        t_end = (int)((int64_t)(sp + 1) * nt / P.S);
    }
    const int b = bh / H, h = bh % H;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;

    const bf16* qp = q + (int64_t)b * Nq * ldq + (int64_t)h * kD;
    const bf16* kp = k + (int64_t)b * Nkv * ldk + (int64_t)h * kD;
    const bf16* vp = v + (int64_t)b * Nkv * ldv + (int64_t)h * kD;
    bf16* op = out + (int64_t)b * Nq * ((int64_t)H * kD) + (int64_t)h * kD;
    const int64_t hd8 = (int64_t)H * kD;      // row pitch of q8 / k8 in bytes

    // ---- Q^T fragments (B operand of S^T = K Q^T): lane (r,hh) holds Q[row r][16*ks + 8*hh + 0..7].
    // (this block and the epilogue stay one-trip loops, as when a wave could own several q-blocks: written straight out, hipcc allocates
    //  the registers of all three forms differently, and what was measured is this code -- tools/isa_diff.py against the parent's)
    int64_t my_q;
    bool q_valid;
    bf16x8 qf[8];
    union Q8F { u32x4 h2[2]; i32x8 f; } qf8[2];
#pragma unroll
    for (int once = 0; once < 1; ++once) {
        my_q = (int64_t)qb * kBM + wave * 32 + r;
        q_valid = my_q < Nq;
        if (!q_valid) my_q = Nq - 1;
        if constexpr (QK8) {
            const uint8_t* q8row = P.q8 + ((int64_t)b * Nq + my_q) * hd8 + (int64_t)h * kD;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                qf8[ks].h2[0] = *reinterpret_cast<const u32x4*>(q8row + 64 * ks + 32 * hh);
                qf8[ks].h2[1] = *reinterpret_cast<const u32x4*>(q8row + 64 * ks + 32 * hh + 16);
            }
        } else {
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qp + my_q * ldq + ks * 16 + hh * 8);
        }
    }
    // scale * log2(e) in the units of this lane's scores; row_unit: those units (the split-KV partials carry their max in q.k units)
    float row_unit = 1.0f;
    if constexpr (QK8) row_unit = P.sq[((int64_t)b * Nq + my_q) * H + h] * P.sk[b * H + h];
    const float scale_log2e = QK8 ? P.scale_log2e * row_unit : P.scale_log2e;

    // ---- tile staging: thread t moves rows (t>>4) + ST_ROWS*i, 16-byte chunk (t&15), of K and V.
    // (e4m3 K: 64 rows x 8 chunks, one per thread: row t>>3, chunk t&7)
    const int st_row = tid >> 4, st_chunk = tid & 15;
    // (e4m3 V^T: 128 channel rows x 4 chunks, one per thread: row t>>2, chunk t&3)
    constexpr int NSTK = QK8 ? 1 : NST, NSTV = PV8 ? 1 : NST;
    int st_k[NSTK], st_v[NSTV];
#pragma unroll
    for (int i = 0; i < NST; ++i) {
        if (i < NSTK) st_k[i] = QK8 ? k8_lds_off(tid >> 3, tid & 7) : k_lds_off(st_row + ST_ROWS * i, st_chunk);
        if (i < NSTV) st_v[i] = PV8 ? v8_lds_off(tid >> 2, tid & 3) : v_lds_off(st_row + ST_ROWS * i, st_chunk);
    }
    // Buffer descriptors (wave-uniform) bound the loads to the head's rows: rows >= Nkv (ragged last tile, prefetch
    // past the end) come back as zeros from the hardware range check -- no clamps, 32-bit offsets.  The tile base stays in
    // the VGPR offset (soffset 0).  (e4m3 V^T: the descriptor spans the head's 128 channel rows, so a prefetch past the last tile is in
    // range for the rows 0..126 and returns bytes of the next row, not zeros; they reach an LDS buffer that no step reads.)
    const uint32_t k_bytes = QK8 ? (uint32_t)((Nkv - 1) * hd8 + kD) : (uint32_t)((Nkv - 1) * ldk * 2 + kD * 2);
    const uint32_t v_bytes = PV8 ? (uint32_t)(kD * P.Nkp) : (uint32_t)((Nkv - 1) * ldv * 2 + kD * 2);
    const void* v_base = PV8 ? (const void*)(P.v8t + (int64_t)h * kD * P.Nkp) : (const void*)vp;
    const void* k_base = QK8 ? (const void*)(P.k8 + (int64_t)b * Nkv * hd8 + (int64_t)h * kD) : (const void*)kp;
    const __amdgpu_buffer_rsrc_t k_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(k_base), 0, k_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t v_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(v_base), 0, v_bytes, 0x00020000);
    const uint32_t k_tile_stride = QK8 ? (uint32_t)(kBN * hd8) : (uint32_t)(kBN * ldk * 2);
    const uint32_t v_tile_stride = PV8 ? (uint32_t)kBN : (uint32_t)(kBN * ldv * 2);
    uint32_t k_off[NSTK], v_off[NSTV];
#pragma unroll
    for (int i = 0; i < NST; ++i) {
        if (i < NSTK) k_off[i] = QK8 ? (uint32_t)((tid >> 3) * hd8 + (tid & 7) * 16) : (uint32_t)((st_row + ST_ROWS * i) * ldk * 2 + st_chunk * 16);
        if (i < NSTV) v_off[i] = PV8 ? (uint32_t)((tid >> 2) * P.Nkp + (tid & 3) * 16) : (uint32_t)((st_row + ST_ROWS * i) * ldv * 2 + st_chunk * 16);
    }
    u32x4 kreg[NSTK], vreg[NSTV];
    auto load_k = [&](int t) {
        const uint32_t base = (uint32_t)t * k_tile_stride;
#pragma unroll
        for (int i = 0; i < NSTK; ++i) kreg[i] = __builtin_amdgcn_raw_buffer_load_b128(k_rsrc, k_off[i] + base, 0, 0);
    };
    auto load_v = [&](int t) {
        const uint32_t base = (uint32_t)t * v_tile_stride;
#pragma unroll
        for (int i = 0; i < NSTV; ++i) vreg[i] = __builtin_amdgcn_raw_buffer_load_b128(v_rsrc, v_off[i] + base, 0, 0);
    };
    auto write_k = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NSTK; ++i) *reinterpret_cast<u32x4*>(k_lds + buf * kTileBytes + st_k[i]) = kreg[i];
    };
    auto write_v = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NSTV; ++i) *reinterpret_cast<u32x4*>(v_lds + buf * kVBuf + st_v[i]) = vreg[i];
    };

    // ---- loop-invariant per-lane LDS read addresses
    int k_rd[8];      // K fragment of k-step ks, sub-tile 0 (sub-tile 1: + 32 rows = + 8192 B)
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) k_rd[ks] = k_lds_off(r, 2 * ks + hh);
    // e4m3: MFMA m = 2 sub + ks reads chunks 4 ks + 2 hh and + 1 of row 32 sub + r (+ 4096 B for sub 1)
    int k8_rd[2][2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int c = 0; c < 2; ++c) k8_rd[ks][c] = k8_lds_off(r, 4 * ks + 2 * hh + c);
    auto read_k8 = [&](const char* kb, int m) {
        Q8F a;
        a.h2[0] = *reinterpret_cast<const u32x4*>(kb + k8_rd[m & 1][0] + (m >> 1) * 4096);
        a.h2[1] = *reinterpret_cast<const u32x4*>(kb + k8_rd[m & 1][1] + (m >> 1) * 4096);
        return a.f;
    };
    // e4m3 V^T: the fragment of channel block db is chunks 2 hh and 2 hh + 1 of row 32 db + r (+ 2048 B per db; the swizzle is r's)
    const int v8_rd[2] = {v8_lds_off(r, 2 * hh), v8_lds_off(r, 2 * hh + 1)};
    auto read_v8 = [&](const char* vb, int db) {
        Q8F a;
        a.h2[0] = *reinterpret_cast<const u32x4*>(vb + v8_rd[0] + db * 2048);
        a.h2[1] = *reinterpret_cast<const u32x4*>(vb + v8_rd[1] + db * 2048);
        return a.f;
    };
    auto mfma8 = [](i32x8 a, i32x8 bq, f32x16 c) { return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, bq, c, 0, 0, 0, 0, 0, 0); };
    // transposed V reads: group g = lane>>4 (g>>1 == hh), i = lane&15, q_ = i>>2, p_ = i&3; block rows 16kk + 8u + 4hh + q_,
    // chunk 4db + 2(g&1) + (p_>>1): offset = base_u + 4096*kk + 512*db  (u = 0/1: second read is 8 rows further)
    const int tr_g1 = (lane >> 4) & 1, tr_q = (lane & 15) >> 2, tr_p = lane & 3;
    const int v_rd0 = v_lds_off(4 * hh + tr_q, 2 * tr_g1 + (tr_p >> 1)) + 8 * (tr_p & 1);
    const int v_rd1 = v_lds_off(8 + 4 * hh + tr_q, 2 * tr_g1 + (tr_p >> 1)) + 8 * (tr_p & 1);

    f32x16 o[4];
    float m_run = -INFINITY, l_run = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) o[i][j] = 0.f;

    // s[sub][reg] = score(key = 64t + 32sub + (reg&3) + 8(reg>>2) + 4hh, query row r)
    auto qk_tile = [&](f32x16 (&s)[2], int buf) {
        const char* kb = k_lds + buf * kTileBytes;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
            for (int j = 0; j < 16; ++j) s[sub][j] = 0.f;
            if constexpr (QK8) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) s[sub] = mfma8(read_k8(kb, 2 * sub + ks), qf8[ks].f, s[sub]);
            } else {
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) {
                    const bf16x8 a = *reinterpret_cast<const bf16x8*>(kb + k_rd[ks] + sub * 8192);
                    s[sub] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qf[ks], s[sub], 0, 0, 0);
                }
            }
        }
    };
    auto mask_tile = [&](f32x16 (&s)[2], int t) {
        const int64_t kbase = (int64_t)t * kBN + 4 * hh;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (kbase + 32 * sub + (j & 3) + 8 * (j >> 2) >= Nkv) s[sub][j] = -INFINITY;
    };

    // Row max of a finished score tile (raw units), combined across the lane pair.
    auto tile_max = [&](const f32x16 (&s)[2]) {
        float mt = max3(s[0][0], s[1][0], s[0][1]);
#pragma unroll
        for (int j = 1; j < 15; ++j) mt = max3(mt, s[1][j], s[0][j + 1]);
        return pair_max(fmaxf(mt, s[1][15]));
    };
    // Deferred rescale: keep the stale max while no row of the wave outgrew it by more than 2^kDefer.
    auto absorb_max = [&](float mt) {
        const bool grow = (mt - m_run) * scale_log2e > kDefer;
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

    // One pipeline step for tile t, written as 32 MFMA "gaps" (16 of S^T(t+1) = K(t+1) Q^T, then 16 of O^T += V(t)^T P(t)^T)
    // with the other work of the step dealt out between them in program order and pinned there by sched_barrier:
    //   * exp2 / bf16 pack of tile t (its max is already folded into m_run: done at the end of the previous step):
    //     21 of the 32 exponentials under the QK gaps, 11 under the first 11 PV gaps, chunk kk complete before PV k-step kk;
    //   * K fragment reads kKDist gaps ahead of their MFMA, V^T fragment reads kVDist gaps ahead;
    //   * the row max of tile t+1 (scores complete after gap 15) under PV gaps 18..31; rescale check after the last gap;
    //   * the LDS writes of K(t+2) / V(t+1) (global loads issued at the top of the step) in the last 4 gaps.
    // kTail: the next tile is ragged or absent (last steps of a range): mask it, or skip its max, outside the gap stream.
    // cur_tag: the K/V ring parity as a compile-time constant (0 / 1: every LDS address is a loop-invariant per-lane base plus
    // an immediate) or -1 (runtime parity, tail steps).
    auto step = [&](f32x16 (&sc)[2], f32x16 (&sn)[2], int t, auto tail_tag, auto cur_tag) {
        constexpr bool kTail = decltype(tail_tag)::value;
        constexpr int kCur = decltype(cur_tag)::value;
        const int cur = kCur >= 0 ? kCur : ((t - t_begin) & 1);
        const char* kb = k_lds + (cur ^ 1) * kTileBytes;
        const char* vb = v_lds + cur * kVBuf;
        load_k(t + 2);
        load_v(t + 1);
        const float mb = PV8 ? m_run * scale_log2e - kPv8Log2C : m_run * scale_log2e;
        float ps0 = 0.f, ps1 = 0.f, mt = 0.f;
        float pe[32];
        union PF { uint32_t w[4]; bf16x8 f; } pf[4];
        bf16x8 ka[16];
        i32x8 ka8[4], va8[4];
        union PF8 { uint32_t w[8]; i32x8 f; } pf8;
        union VF { s16x4 h2[2]; bf16x8 f; } va[16];
        auto read_k = [&](int g) { ka[g] = *reinterpret_cast<const bf16x8*>(kb + k_rd[g & 7] + (g >> 3) * 8192); };
        auto read_v = [&](int p) {
            va[p].h2[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vb + v_rd0 + 4096 * (p >> 2) + 512 * (p & 3)));
            va[p].h2[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vb + v_rd1 + 4096 * (p >> 2) + 512 * (p & 3)));
        };
        // exponential e (0..31) = element (sub = e >> 4, j = e & 15); pair unit u = e >> 1 -> word (u & 3) of pf[u >> 2]
        auto do_exp = [&](int e) {
            const float p = fast_exp2(sc[e >> 4][e & 15] * scale_log2e - mb);
            pe[e] = p;
        };
        // Row-sum add as opaque asm (no SLP packing / sinking to the end of the step).  Issued one gap AFTER the exponential:
        // gfx950 needs a wait state between a transcendental and a VALU reader of its result, and the compiler's hazard
        // pass does not look inside inline asm.
        auto do_add = [&](int e) { if (e & 1) ps1 = add_f32(ps1, pe[e]); else ps0 = add_f32(ps0, pe[e]); };
        auto do_pack = [&](int u) { pf[u >> 2].w[u & 3] = cvt_pk_bf16(pe[2 * u], pe[2 * u + 1]); };
        // e4m3 P V form: dword w of the B operand = exponentials 4 w .. 4 w + 3 (c p <= 2^8: no clamp), v_cvt_pk_fp8_f32 into each half
        auto do_pack8 = [&](int w) {
            const int lo = __builtin_amdgcn_cvt_pk_fp8_f32(pe[4 * w], pe[4 * w + 1], 0, false);
            pf8.w[w] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(pe[4 * w + 2], pe[4 * w + 3], lo, true);
        };

        if constexpr (QK8) ka8[0] = read_k8(kb, 0);
        else static_for<0, kKDist>([&](auto i) { read_k(decltype(i)::value); });
        __builtin_amdgcn_sched_barrier(0);
        static_for<0, 32>([&](auto gc) {
            constexpr int g = decltype(gc)::value;
            // exponentials issued before gap g: exps_before(g); this gap issues [e0, e1)
            constexpr int e0 = PV8 ? exps_before_pv8(g) : exps_before(g), e1 = PV8 ? exps_before_pv8(g + 1) : exps_before(g + 1);
            constexpr int ep = g == 0 ? 0 : (PV8 ? exps_before_pv8(g - 1) : exps_before(g - 1));
            // e4m3 P V form: dword g / 2 - 1 of P8 in the even gaps 2..16, ahead of the gap's MFMA (the one of gap 16 reads all 8)
            if constexpr (PV8 && (g & 1) == 0 && g >= 2 && g <= 16) do_pack8(g / 2 - 1);
            if constexpr (g < 16) {
                constexpr int sub = g >> 3, ks = g & 7;
                if constexpr (ks == 0) {
#pragma unroll
                    for (int j = 0; j < 16; ++j) sn[sub][j] = 0.f;
                }
                if constexpr (QK8) {      // one 32x32x64 MFMA (4x the length of a bf16 one) every 4th gap; its K fragment read 3 gaps ahead
                    if constexpr ((g & 3) == 0) sn[sub] = mfma8(ka8[g >> 2], qf8[(g >> 2) & 1].f, sn[sub]);
                    if constexpr ((g & 3) == 1 && g < 12) ka8[(g >> 2) + 1] = read_k8(kb, (g >> 2) + 1);
                } else {
                    sn[sub] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka[g], qf[ks], sn[sub], 0, 0, 0);
                    if constexpr (g + kKDist < 16) read_k(g + kKDist);
                }
            } else if constexpr (PV8) {      // one 32x32x64 MFMA per channel block every 4th gap; its V^T fragment read 3 gaps ahead
                if constexpr ((g & 3) == 0) o[(g - 16) >> 2] = mfma8(va8[(g - 16) >> 2], pf8.f, o[(g - 16) >> 2]);
            } else {
                constexpr int p = g - 16;
                o[p & 3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va[p].f, pf[p >> 2].f, o[p & 3], 0, 0, 0);
            }
            if constexpr (PV8) {
                if constexpr ((g & 3) == 1 && g >= 13 && g < 29) va8[(g - 13) >> 2] = read_v8(vb, (g - 13) >> 2);
            } else {
                if constexpr (g + kVDist >= 16 && g + kVDist < 32) read_v(g + kVDist - 16);
                // pack unit u in the first gap that starts with both of its exponentials issued (after this gap's MFMA: the
                // packed word is first used by a later gap's MFMA)
                constexpr int u0 = ep / 2, u1 = e0 / 2;
                if constexpr (u1 > u0) do_pack(u0);
                if constexpr (u1 > u0 + 1) do_pack(u0 + 1);
            }
            if constexpr (e1 > e0) do_exp(e0);
            if constexpr (e1 > e0 + 1) do_exp(e0 + 1);
            if constexpr (e0 > ep) do_add(ep);
            if constexpr (e0 > ep + 1) do_add(ep + 1);
            if constexpr (!kTail && g >= 17) {      // 15 max3 steps in gaps 17..31 (scores of tile t+1 complete after gap 15)
                constexpr int i = g - 17;
                if constexpr (i == 0) mt = max3(sn[0][0], sn[1][0], sn[0][1]);
                else mt = max3(mt, sn[1][i], sn[0][i + 1]);
            }
            if constexpr (g == 28) write_k(cur);
            if constexpr (g == 30) write_v(cur ^ 1);
            __builtin_amdgcn_sched_barrier(0);
        });
        l_run += ps0 + ps1;
        if (!kTail) {
            absorb_max(pair_max(fmaxf(mt, sn[1][15])));
        } else if (t + 1 < t_end) {
            if ((int64_t)(t + 2) * kBN > Nkv) mask_tile(sn, t + 1);      // ragged last tile (wave-uniform)
            absorb_max(tile_max(sn));
        }
        __syncthreads();
    };

    // ---- prologue: K(0), V(0), K(1) resident; scores(0) computed and their max taken
    f32x16 sA[2], sB[2];
    load_k(t_begin);
    load_v(t_begin);
    write_k(0);
    write_v(0);
    load_k(t_begin + 1);
    write_k(1);
    __syncthreads();
    qk_tile(sA, 0);
    if ((int64_t)(t_begin + 1) * kBN > Nkv) mask_tile(sA, t_begin);
    m_run = tile_max(sA);
    __syncthreads();      // every wave is done with the first K tile before step 0 overwrites it

    // fast steps: the next tile exists in this range and is full
    const int t_fast = min(t_end - 1, (int)(Nkv / kBN) - 1);
    int t = t_begin;
    for (; t + 1 < t_fast; t += 2) {
        step(sA, sB, t, std::false_type{}, std::integral_constant<int, 0>{});
        step(sB, sA, t + 1, std::false_type{}, std::integral_constant<int, 1>{});
    }
    for (; t < t_end; ++t) {      // <= 3 steps: odd fast step, ragged-next step, last step
        step(sA, sB, t, std::true_type{}, std::integral_constant<int, -1>{});
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) sA[sub] = sB[sub];
    }

    // ---- epilogue: lane holds O[query r][d = 32db + 8g + 4hh + 0..3]
#pragma unroll
    for (int once = 0; once < 1; ++once) {      // (a one-trip loop: see the Q^T fragments)
        const float l_tot = pair_sum(l_run);
        if constexpr (PV8) {      // the channel scales of V8: acc * sv[channel], here for the direct store and for the partials alike
            const float* svp = P.sv + (int64_t)h * kD + 4 * hh;
#pragma unroll
            for (int db = 0; db < 4; ++db)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 s4 = *reinterpret_cast<const f32x4*>(svp + 32 * db + 8 * g);
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[db][4 * g + j] *= s4[j];
                }
        }
        if (piece < 0) {      // direct: normalise and store bf16
            const float inv = 1.0f / l_tot;
            if (q_valid) {
                bf16* orow = op + my_q * ((int64_t)H * kD);
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
        } else {              // piece: un-normalised partial + (max, sum) to the workspace
            const int row = wave * 32 + r;
            float* orow = P.o_part + ((int64_t)piece * kBM + row) * kD;
#pragma unroll
            for (int db = 0; db < 4; ++db)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 w4;
#pragma unroll
                    for (int j = 0; j < 4; ++j) w4[j] = o[db][4 * g + j];
                    *reinterpret_cast<f32x4*>(orow + 32 * db + 8 * g + 4 * hh) = w4;
                }
            if (hh == 0) {
                float* ml = P.ml_part + ((int64_t)piece * kBM + row) * 2;
                ml[0] = m_run * row_unit;
                ml[1] = l_tot;
            }
        }
    }
