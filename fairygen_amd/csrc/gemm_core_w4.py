"""The 4-wave / 512-register GEMM core of the convolution generator (gen_conv_w4.py imports it; it generates nothing itself).  It was
once a stand-alone generator, of the bias-GEMM gemm_w4_kernel, which left the library when the persistent GEMM of gen_gemm_p.py took
over the DiT Linear layers: what remains is the k-loop and its register map.

Tile: 256 output columns (W rows: the MFMA A operand) x 256 output rows (X rows: the MFMA B operand) x 64 k per step; 4 waves
as 2 (n) x 2 (m), each 128 x 128 = 4 x 4 accumulators of v_mfma_f32_32x32x16_bf16 = all 256 AGPRs; the accumulator holds, per
lane, ONE output row and 4 consecutive columns per register group (8-byte stores, lane-local bias).  Operand tiles go global
-> LDS by LDS-DMA (1 KiB per wave-instruction, XOR swizzle applied to the source chunk) into 2 stages of 64 KiB; fragments
are read one k-step ahead of their MFMAs into two register sets, and the last k-step of a stage is multiplied AFTER the
barrier beside the first fragment reads of the next stage, so neither LDS latency nor the barrier is exposed; every fragment
read feeds 4 MFMAs.  One vmcnt(0) + one barrier per 64 MFMAs.  The caller owns the k offsets of the two operands (SGPRs passed
to dma_piece / build_iteration), the prologue, the loop control and the epilogue.
"""
from asm_emit import Item, schedule, vr, ar, sr

DMA_EVERY_X2 = 4                    # LDS-DMA pieces are issued every DMA_EVERY_X2 / 2 MFMA gaps from the start of a K-step
STAGE, XOFF = 65536, 32768          # LDS: stage s at s*64 KiB: W tile (32 KiB) then X tile (32 KiB)
SB = 40
S = {k: v + SB for k, v in dict(XD=0, WD=4, CD=8, BD=12, WAVE=16, LDA=18, T=22, TMP0=23, TMP1=24, WDST=26, XDST=27, KW=28, TMP64=30,
                                ST0=32, ST1=34, ST2=36).items()}      # ST0..ST2: scratch of the caller's --stamp build
NSREG = 40                           # s[SB : SB+40] belong to the core; the caller's own SGPRs start above
# VGPR map (v0.. owned by the body)
F0, F1 = 0, 32                       # fragment sets: W frag ni at +4ni, X frag mi at +16+4mi
V_WRD, V_XRD = 64, 72                # [stage][ks]: 8 + 8 LDS read bases
V_DW, V_DX = 80, 88                  # 8 + 8 LDS-DMA source offsets (pieces of this wave)
V_T = 96                             # temporaries 96..127


def acc(ni, mi, j=0):
    return (ni * 4 + mi) * 16 + j


def emit_lane_setup(E):
    L, R, HH, SW, T0, T1, T2 = (V_T + i for i in range(7))
    E.e(f"v_mbcnt_lo_u32_b32 {vr(L)}, -1, 0")
    E.e(f"v_mbcnt_hi_u32_b32 {vr(L)}, -1, {vr(L)}")
    E.e(f"v_and_b32 {vr(R)}, 31, {vr(L)}")
    E.e(f"v_lshrrev_b32 {vr(HH)}, 5, {vr(L)}")
    # fragment read bases: (half*128 + r)*128 + (((2ks + hh) ^ ((r>>1)&7)) << 4), W half = wave>>1, X half = wave&1
    E.e(f"v_bfe_u32 {vr(SW)}, {vr(R)}, 1, 3")
    E.e(f"v_lshlrev_b32 {vr(T0)}, 7, {vr(R)}")
    E.e(f"s_lshr_b32 {sr(S['TMP0'])}, {sr(S['WAVE'])}, 1")
    E.e(f"s_lshl_b32 {sr(S['TMP0'])}, {sr(S['TMP0'])}, 14")
    E.e(f"s_and_b32 {sr(S['TMP1'])}, {sr(S['WAVE'])}, 1")
    E.e(f"s_lshl_b32 {sr(S['TMP1'])}, {sr(S['TMP1'])}, 14")
    E.e(f"s_add_u32 {sr(S['TMP1'])}, {sr(S['TMP1'])}, {XOFF}")
    for ks in range(4):
        E.e(f"v_or_b32 {vr(T1)}, {2 * ks}, {vr(HH)}")
        E.e(f"v_xor_b32 {vr(T1)}, {vr(T1)}, {vr(SW)}")
        E.e(f"v_lshl_add_u32 {vr(T1)}, {vr(T1)}, 4, {vr(T0)}")
        E.e(f"v_add_u32 {vr(V_WRD + ks)}, {sr(S['TMP0'])}, {vr(T1)}")
        E.e(f"v_add_u32 {vr(V_XRD + ks)}, {sr(S['TMP1'])}, {vr(T1)}")
        E.e(f"v_add_u32 {vr(V_WRD + 4 + ks)}, {STAGE}, {vr(V_WRD + ks)}")
        E.e(f"v_add_u32 {vr(V_XRD + 4 + ks)}, {STAGE}, {vr(V_XRD + ks)}")
    # LDS-DMA source offsets: piece i of this wave covers tile rows 64w + 8i .. +7; lane: row = 64w + 8i + (l>>3),
    # source chunk = (l&7) ^ ((row>>1)&7) = (l&7) ^ ((4(i&1) + (l>>4)) & 7)
    E.e(f"v_lshrrev_b32 {vr(T0)}, 3, {vr(L)}")                          # l>>3
    E.e(f"s_lshl_b32 {sr(S['TMP0'])}, {sr(S['WAVE'])}, 6")
    E.e(f"v_add_u32 {vr(T0)}, {sr(S['TMP0'])}, {vr(T0)}")               # 64w + (l>>3)
    E.e(f"v_lshrrev_b32 {vr(T1)}, 4, {vr(L)}")                          # l>>4
    E.e(f"v_and_b32 {vr(T2)}, 7, {vr(L)}")
    for i in range(8):
        E.e(f"v_add_u32 {vr(SW)}, {4 * (i & 1)}, {vr(T1)}")
        E.e(f"v_and_b32 {vr(SW)}, 7, {vr(SW)}")
        E.e(f"v_xor_b32 {vr(SW)}, {vr(SW)}, {vr(T2)}")
        E.e(f"v_lshlrev_b32 {vr(SW)}, 4, {vr(SW)}")                     # source chunk * 16
        E.e(f"v_add_u32 {vr(R)}, {8 * i}, {vr(T0)}")                    # row
        E.e(f"v_mul_lo_u32 {vr(V_DW + i)}, {vr(R)}, {sr(S['KW'])}")
        E.e(f"v_add_u32 {vr(V_DW + i)}, {vr(V_DW + i)}, {vr(SW)}")
        E.e(f"v_mul_lo_u32 {vr(V_DX + i)}, {vr(R)}, {sr(S['LDA'])}")
        E.e(f"v_add_u32 {vr(V_DX + i)}, {vr(V_DX + i)}, {vr(SW)}")
    E.nops(2)


def dma_piece(op, i, stage, koff):
    """One LDS-DMA piece of the W / X tile into `stage`; koff: the SGPR that holds the operand's k offset (scalar offset of the load)."""
    base, dst, rs = (V_DW, S["WDST"], S["WD"]) if op == "W" else (V_DX, S["XDST"], S["XD"])
    return [f"s_add_u32 m0, {sr(dst)}, {stage * STAGE + i * 1024}",
            "s_nop 0",
            f"buffer_load_dwordx4 {vr(base + i)}, {sr(rs, 4)}, {sr(koff)} offen lds"]


def frag_read(op, blk, fset, stage, ks):
    """ds_read_b128 of W fragment ni / X fragment mi of k-step ks into fragment set fset."""
    dst = fset + (0 if op == "W" else 16) + 4 * blk
    base = (V_WRD if op == "W" else V_XRD) + 4 * stage + ks
    return f"ds_read_b128 {vr(dst, 4)}, {vr(base)} offset:{blk * 4096}"


def mfma(ni, mi, fset):
    d = ar(acc(ni, mi), 16)
    return f"v_mfma_f32_32x32x16_bf16 {d}, {vr(fset + 4 * ni, 4)}, {vr(fset + 16 + 4 * mi, 4)}, {d}"


def build_iteration(E, stage, first, budget, koff_w, koff_x):
    """One K-step of 64 (tile t in LDS stage `stage`): block 0 = last k-step of tile t-1 (fragment set F1, read before the
    barrier), blocks 1..3 = k-steps 0..2 of tile t; reads of k-step s+1 beside the MFMAs of k-step s; the LDS-DMA of tile t+1
    goes to the other stage.  first: the peeled first iteration (no block 0)."""
    items = []
    add = items.append
    sets = [F1, F0, F1, F0]                       # fragment set multiplied by block b
    # reads: R(t,0)->F0 (needed by block 1), R(t,1)->F1 (block 2; F1 busy in block 0), R(t,2)->F0 (block 3; busy in block 1),
    # R(t,3)->F1 (next iteration's block 0; busy in block 2)
    for ks, (fset, busy_blk, need_blk) in enumerate([(F0, None, 1), (F1, 0, 2), (F0, 1, 3), (F1, 2, 4)]):
        for op in ("W", "X"):
            for blk in range(4):
                if busy_blk is None or (first and busy_blk == 0):
                    earliest = 0
                else:      # W fragment ni is multiplied in gaps 16b + 4ni .. +3, X fragment mi last in gap 16b + 12 + mi
                    earliest = 16 * busy_blk + (4 * blk + 3 if op == "W" else 12 + blk) + 2
                need = 16 * need_blk + (4 * blk if op == "W" else blk)
                deadline = min(need - 4, 60)
                add(Item(f"rd{ks}{op}{blk}", [frag_read(op, blk, fset, stage, ks)], 2, earliest=earliest, deadline=max(deadline, earliest),
                         lds=1))
    for n, (op, i) in enumerate([("W", i) for i in range(8)] + [("X", i) for i in range(8)]):
        g0 = 1 + (n * DMA_EVERY_X2) // 2
        add(Item(f"dma{op}{i}", dma_piece(op, i, stage ^ 1, koff_w if op == "W" else koff_x), 12, earliest=g0, deadline=g0 + 8))
    gaps, _ = schedule(items, 64, budget)
    lds_issued, lds_done, done_at = 0, 0, {}
    # reads of R(t-1,3) (set F1, block 0) completed before the barrier (lgkmcnt(0))
    for g in range(64):
        b, idx = g >> 4, g & 15
        ni, mi = idx >> 2, idx & 3
        fset = sets[b]
        if not (first and b == 0):
            ks = b - 1
            if b >= 1:
                need = max(done_at[f"rd{ks}W{ni}"], done_at[f"rd{ks}X{mi}"])
                if need > lds_done:
                    E.e(f"s_waitcnt lgkmcnt({min(lds_issued - need, 15)})")
                    lds_done = need if lds_issued - need <= 15 else lds_issued - 15
            E.e(mfma(ni, mi, fset))
        for it in gaps[g]:
            for ln in it.lines:
                E.e(ln)
            lds_issued += it.lds
            if it.lds:
                done_at[it.name] = lds_issued
    E.e("s_waitcnt vmcnt(0) lgkmcnt(0)")
    E.e("s_barrier")
