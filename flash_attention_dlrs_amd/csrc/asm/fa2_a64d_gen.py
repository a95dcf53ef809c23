#!/usr/bin/env python3
"""Generator of the gfx950 assembly kernels `fa2_fwd_a64d_<dtype>_<c|n>` -- FA-2 forward, HEAD SIZE 64, f16 / bf16: the a64 kernel
(fa2_a64_gen.py: 4 waves x 64 query rows, one wave per SIMD, persistent grid, continuous tile stream, LDS-DMA staging,
modulo-scheduled softmax, causal split row map) at d = 64.  The reference runs every power-of-two head size through one kernel
(/root/reference/src/flash_attention_kernels.py:17-32); here d = 64 ran on the 8-wave HIP kernels at 32-37 % of the matrix peak.

Half the columns: a 64-key step is 16 + 16 MFMAs of v_mfma_f32_32x32x16 (and the eight 16x16x32 row sums) against the same 64 x 64
scores of softmax -- the kernel is VALU-issue bound (~1 350 cycles of softmax per 1 150 of MFMA); its MFMA lists keep a64's 32 + 40
slots with an MFMA in every second product slot, and emit_phase hands each MFMA the fillers of the slots it stands for (later
runs take over what an earlier one has too much of).  Score layout, packed P, row sums, masks and rescale are a64's; rows are 128
bytes, so the tile images (8 KiB), the DMA pieces (two per wave and tile), the Q staging and the epilogue have the geometry of the
fp8 kernel (fa2_a8_gen.py).  N a multiple of 256.
"""
from __future__ import annotations


from .isa import A, EXEC, I, Label, M0, Reg, S, V, VCC, comment, label, waitcnt
from .stream_gen import (KARG_SIZE, NSLOT, SBUF, S_DBG, S_FINAL, S_FLAG, S_JOB, S_K32, S_K64, S_KARG, S_KDMA, S_KRS, S_KSN,
                         S_KT0, S_KW, S_LDSW, S_LG, S_N, S_NQ, S_NVRS, S_OSN, S_PASS, S_Q, S_QROW, S_QSB, S_QSH, S_QSN, S_SQ,
                         S_T, S_V32, S_V64, S_VDMA, S_VRS, S_VSN, S_VW, S_WAVE, S_WGID, S_X2, StreamGen)

# ------------------------------------------------------------------------------------------------- register map
# arch VGPRs
# SBUF = (0, 64) (stream_gen): two score buffers of 64 registers: group g = 2*qb + kb at +16 g (packed in place: P(qb, kstep = 2 kb + s) at + 4 s)
KF = 128                  # K fragments of the next tile: (kb, ks) at KF + 4 (4 kb + ks), ks = 0..3
V_KR = (160, 161, 162, 163)   # K row-read lane bases per 16-column step ks: chunk 2 ks + h
V_VR = (164, 165)         # V transposed-read lane bases per 32-column block db (the V ring's LDS offset included)
V_QR = (168, 169, 170, 171)   # Q row-read lane bases in the wave's slice
V_DKO, V_DVO = 172, 173   # LDS-DMA per-lane source offsets of K / V rows
V_DQ = (174, 175)         # ... of Q rows (even / odd 8-row group)
V_MC = (176, 177)         # running row maximum in the exp2 domain (c * max), per query block
V_CO = (178, 179)         # rescale coefficient per query block
V_MX = ((180, 181), (182, 183))  # row-max chains [qb][kb]
V_MSV = (184, 185)        # running maximum of the finished job
V_LANE = 186
V_EW, V_ER, V_EO, V_L2 = 187, 188, 189, 190   # epilogue: LDS write base, LDS read base, global store lane offset, L store lane offset
V_IMH = 191               # causal: i - 4 h (query row inside a 32-row block minus the lane half's key offset)
V_T = tuple(range(192, 202))     # temporaries (V_T[0], [2], .. even)
V_Z = 204                 # 4 registers, 4-aligned: the zero operand of the epilogue's clearing MFMAs
V_ONES = 208              # 4 registers: the 0 / 1 A operand of the row-sum MFMA (v_mfma_f32_16x16x32)
V_LACC = (216, 220)       # row-sum accumulators of the two query blocks (4 registers each; register 0 = the lane's own row)
V_ST_LAST, V_ST_ACC = 224, 225   # diagnostic builds: last stamp (low word), accumulators [3]
V_NINF = 231
NINF = V(V_NINF)
V_LSV = (232, 233)
V_PM = (236, 237, 238, 239, 240, 241, 242, 243)   # causal: AND masks of the eight packed P registers of a triangle group


# AGPRs
def A_O(qb, db):
    return A((qb * 2 + db) * 16, 16)


def A_Q(qb, ks):
    return A(64 + (qb * 4 + ks) * 4, 4)


def A_K(kb, ks):
    return V(KF + (kb * 4 + ks) * 4, 4)


def V_F(kstep, db):
    # V^T fragments in a[96:127]: read in phase A, whose MFMAs (QK^T) write arch VGPRs
    return A(96 + 4 * (2 * kstep + db), 4)


def swz_k(row):
    """K / Q tile image: 16-byte chunk c of row r at 128 r + 16 (c ^ swz_k(r)) (fa2_mfma8x.hip's, conflict-free for the row reads)"""
    return (((row >> 1) & 1) << 2) | ((row >> 2) & 3)


def swz_v(row):
    """V tile image: 16-byte chunk c of row r at 128 r + 16 (c ^ swz_v(r)): rows two apart swap the two 32-column blocks, so the 4 x 4
    rows x chunks of a transposing read fall on 32 different 8-byte bank slots"""
    return ((row >> 1) & 1) << 2


# SGPRs: the map shared by all four families is stream_gen's.
S_NDESC, S_DESC = S(98), S(99)   # (product builds: the debug pointer's registers) causal: the next / the current job walks its
#                                  non-diagonal key tiles in DESCENDING order (k_decode_next)

# LDS map (bytes)
KB = (0, 8192)
VBASE = 16384
VB = (0, 8192)                   # relative to VBASE (folded into the V read lane bases; absolute for the DMA)
EPI = 32768                      # + 16384 * wave: the wave's private slice: the next job's 64 Q rows land here by LDS-DMA (8 KiB,
                                 # K-tile image) on their way to a[128:159]; later the job's O rows leave through it
EPI_ROW = 136                    # (= 128 + 8) byte stride of an O row in the slice during the epilogue: 8-byte aligned for the
                                 # row read-back, the 4-byte column writes of 32 lanes are 2-way (free for ds_write_b32)
LDS_TOTAL = 32768 + 4 * 16384


class Gen(StreamGen):
    # the family's registers and LDS size, as the shared stream methods read them (stream_gen.StreamGen)
    V_T, V_ST_LAST, V_ST_ACC, V_MC, V_MX, V_CO, V_MSV, V_LACC, V_LANE, V_IMH, V_PM, NINF = \
        V_T, V_ST_LAST, V_ST_ACC, V_MC, V_MX, V_CO, V_MSV, V_LACC, V_LANE, V_IMH, V_PM, NINF
    S_NDESC, S_DESC = S_NDESC, S_DESC
    LDS_TOTAL = LDS_TOTAL
    FAMILY, MFMA = "a64d", "v_mfma_f32_32x32x16_{dtype}"
    CVT = {"bf16": "v_cvt_pk_bf16_f32", "f16": "v_cvt_pk_f16_f32"}
    DMA_PIECES, K_READS, V_READS = 2, 8, 16
    DMA_GAPS = (11, 15, 21, 25)
    # the seam's eight Q-staging pieces: four behind step 0's own K / V pieces, two in the quiet end of the next phase A, two in
    # front of step 1's own; the barrier wait of step 1 leaves those six in flight
    QS_GAPS = ((1, 5, 11, 15), (21, 25, 29, 33), (24, 28), (1, 5), 6)
    O_AGPRS, ROW_BYTES, L_SN = 64, 128, 2
    BRANCH_NEED, WALK_DOWN = None, True

    # ------------------------------------------------------------------ kernel prologue: arguments, lane constants
    def k_setup(self):
        e = self.e
        e(comment("kernel arguments"),
          I("s_load_dwordx8", S(4, 8), S_KARG, 0), I("s_load_dwordx4", S(12, 4), S_KARG, 32),
          I("s_load_dwordx16", S(16, 16), S_KARG, 48), I("s_load_dwordx4", S(32, 4), S_KARG, 112),
          I("s_load_dwordx8", S(36, 8), S_KARG, 128), I("s_load_dwordx4", S(44, 4), S_KARG, 160),
          I("s_load_dwordx2", S_DBG, S_KARG, 176), I("s_load_dword", S_LG, S_KARG, 184))
        lane, t0, t1, t2, t3 = V(V_LANE), V(V_T[0]), V(V_T[1]), V(V_T[2]), V(V_T[3])
        e(I("v_and_b32", lane, 63, V(0)), I("v_lshrrev_b32", t0, 6, V(0)), I("s_nop", 1), I("v_readfirstlane_b32", S_WAVE, t0), I("s_nop", 4),
          I("s_lshl_b32", S_LDSW, S_WAVE, 10))
        # i = lane & 31, h = lane >> 5
        # ---- K row-read bases: row i, chunk c = 4 ks + 2 u + h at 128 i + 16 (c ^ swz_k(i)), swz_k(i) = 4 ((i >> 1) & 1) | ((i >> 2) & 3)
        e(comment("K row-read lane bases"),
          I("v_and_b32", t0, 31, lane),                    # i
          I("v_bfe_u32", t1, t0, 1, 1), I("v_lshlrev_b32", t1, 2, t1),
          I("v_bfe_u32", t2, t0, 2, 2), I("v_or_b32", t1, t1, t2),          # swz_k(i)
          I("v_lshrrev_b32", t2, 5, lane), I("v_xor_b32", t1, t1, t2),      # h ^ swz_k(i)
          I("v_lshlrev_b32", t3, 7, t0))                   # 128 i
        for ks in range(4):     # chunk 2 ks + h
            e(I("v_xor_b32", t2, 2 * ks, t1), I("v_lshl_add_u32", V(V_KR[ks]), t2, 4, t3))
        # ---- V transposed-read bases (ds_read_b64_tr_b16): in a 16-lane group lane 4 q + p supplies key row 4 h + q, columns
        #      16 w + 4 p .. + 3 of the 32-column block db (w = (lane >> 4) & 1):
        #      VBASE + 128 (4 h + q) + 16 ((4 db + 2 w + (p >> 1)) ^ swz_v(row)) + 8 (p & 1),  swz_v(row) = 4 ((q >> 1) & 1)
        e(comment("V transposed-read lane bases"),
          I("v_bfe_u32", t0, lane, 2, 2),                  # q
          I("v_lshrrev_b32", t1, 5, lane), I("v_lshl_add_u32", t1, t1, 2, t0),          # 4 h + q
          I("v_lshlrev_b32", t1, 7, t1),                   # 128 row
          I("v_and_b32", t2, 1, lane), I("v_lshl_add_u32", t1, t2, 3, t1),              # + 8 (p & 1)
          I("v_add_u32", t1, VBASE, t1),
          I("v_bfe_u32", t2, lane, 4, 1), I("v_lshlrev_b32", t2, 1, t2),                # 2 w
          I("v_bfe_u32", t3, lane, 1, 1), I("v_or_b32", t2, t2, t3),                    # + (p >> 1)
          I("v_bfe_u32", t3, t0, 1, 1), I("v_lshlrev_b32", t3, 2, t3), I("v_xor_b32", t2, t2, t3))   # ^ swz_v
        for db in range(2):
            e(I("v_xor_b32", t3, 4 * db, t2), I("v_lshl_add_u32", V(V_VR[db]), t3, 4, t1))
        # ---- LDS-DMA lane source offsets: a piece is 8 rows x 128 bytes (rows 8 R ..); lane i lands at row 8 R + (i >> 3), 16-byte
        #      position i & 7 of the image, which holds chunk (i & 7) ^ swz_k(row) (K / Q) or (i & 7) ^ swz_v(row) (V).  Bit 3 of the row
        #      (swz_k only) is R & 1: the wave's parity for K (R = wave, wave + 4)
        e(comment("LDS-DMA per-lane source offsets"),
          I("v_lshrrev_b32", t1, 3, lane),                 # row_in
          I("v_and_b32", t0, 7, lane))                     # pos
        e(waitcnt(lgkmcnt=0, comment="kernel arguments are in"))
        e(I("s_and_b32", S_T[0], S_WAVE, 1))               # R & 1 for the K / V pieces
        # swz_k(row) = 4 ((row_in >> 1) & 1) | (((row_in >> 2) & 1) + 2 (R & 1))
        def swz_k_ops(dst, par):
            out = [I("v_bfe_u32", t2, t1, 1, 1), I("v_lshlrev_b32", t2, 2, t2), I("v_bfe_u32", t3, t1, 2, 1), I("v_or_b32", t2, t2, t3)]
            if isinstance(par, Reg):
                out += [I("s_lshl_b32", S_T[1], par, 1), I("v_or_b32", t2, S_T[1], t2)]
            elif par:
                out += [I("v_or_b32", t2, 2, t2)]
            return out + [I("v_xor_b32", t2, t2, t0), I("v_lshlrev_b32", dst, 4, t2)]       # 16 (pos ^ swz_k)
        e(swz_k_ops(t2, S_T[0]), I("v_mul_lo_u32", t3, t1, S_KSN), I("v_add_u32", V(V_DKO), t3, t2))
        for par in range(2):
            e(swz_k_ops(t2, par), I("v_mul_lo_u32", t3, t1, S_QSN), I("v_add_u32", V(V_DQ[par]), t3, t2))
        # swz_v(row) = 4 ((row_in >> 1) & 1)
        e(I("v_bfe_u32", t2, t1, 1, 1), I("v_lshlrev_b32", t2, 2, t2), I("v_xor_b32", t2, t2, t0), I("v_lshlrev_b32", t2, 4, t2),
          I("v_mul_lo_u32", t3, t1, S_VSN), I("v_add_u32", V(V_DVO), t3, t2))
        e(comment("Q row-read bases in the wave's slice"),
          I("s_lshl_b32", S_T[0], S_WAVE, 14), I("s_add_u32", S_T[0], S_T[0], EPI))
        e([I("v_add_u32", V(V_QR[k]), S_T[0], V(V_KR[k])) for k in range(4)])
        # ---- epilogue: the wave's slice holds a query block's 32 O rows (64 columns: 128 bytes) at a stride of EPI_ROW = 136 bytes.
        #      Write base (row i, + 8 h): slice + 136 i + 8 h;  read-back (a = lane >> 3, ec = lane & 7): slice + 136 a + 16 ec
        #      (+ 8 x 136 k: row 8 k + a), two ds_read_b64; store offset a * os_n + 16 ec
        e(comment("epilogue lane constants"),
          I("v_and_b32", t0, 31, lane), I("v_lshrrev_b32", t3, 5, lane),
          I("v_mul_u32_u24", t1, EPI_ROW, t0), I("v_lshl_add_u32", t1, t3, 3, t1), I("v_add_u32", V(V_EW), S_T[0], t1),
          I("v_lshrrev_b32", t0, 3, lane), I("v_and_b32", t1, 7, lane),
          I("v_mul_u32_u24", t2, EPI_ROW, t0), I("v_lshl_add_u32", t2, t1, 4, t2), I("v_add_u32", V(V_ER), S_T[0], t2),
          I("v_mul_lo_u32", t2, t0, S_OSN), I("v_lshl_add_u32", V(V_EO), t1, 4, t2),
          I("v_and_b32", t0, 31, lane), I("v_lshlrev_b32", V(V_L2), 1, t0))
        if self.stamps:
            e(I("s_lshl_b32", S_T[0], S_WGID, 2), I("s_add_u32", S_T[0], S_T[0], S_WAVE), I("s_mul_i32", S_T[0], S_T[0], 8 * NSLOT),
              I("s_add_u32", S_DBG.sub(0), S_DBG.sub(0), S_T[0]), I("s_addc_u32", S_DBG.sub(1), S_DBG.sub(1), 0))
            e(self.stamp(6, real=True), self.stamp(8))
            e([I("v_mov_b32", V(V_ST_ACC + k), 0) for k in range(3)], I("v_mov_b32", V(V_ST_LAST), 0))
        # ---- row sums on the matrix pipe: the 0 / 1 operand (lanes with (lane & 7) == 4 * ((lane >> 4) & 1) hold ones), accumulators
        one2 = 0x3F803F80 if self.dtype == "bf16" else 0x3C003C00
        e(comment("row-sum MFMA operand, accumulators, rescale factors"),
          I("v_bfe_u32", t1, lane, 4, 1), I("v_lshlrev_b32", t1, 2, t1), I("v_and_b32", t0, 7, lane),
          I("v_cmp_eq_u32", VCC, t0, t1), I("v_mov_b32", t2, one2))
        e([I("v_cndmask_b32", V(V_ONES + k), 0, t2, VCC) for k in range(4)])
        e([I("v_mov_b32", V(V_LACC[qb] + k), 0) for qb in range(2) for k in range(4)])
        e([I("v_mov_b32", V(V_CO[qb]), 1.0) for qb in range(2)])
        # ---- scalar constants
        e(I("s_lshl_b32", S_K32, S_KSN, 5), I("s_lshl_b32", S_V32, S_VSN, 5),
          I("s_lshl_b32", S_K64, S_KSN, 6), I("s_lshl_b32", S_V64, S_VSN, 6),
          I("s_lshl_b32", S_T[0], S_WAVE, 3), I("s_mul_i32", S_KW, S_T[0], S_KSN), I("s_mul_i32", S_VW, S_T[0], S_VSN),
          I("s_mov_b32", S_FLAG, 0), I("s_mov_b32", S_PASS, 0), I("s_mov_b32", S_FINAL, 0),
          I("s_mov_b32", S_JOB, S_WGID))
        if self.ragged and not self.causal:
            e(comment("ragged, non-causal: real keys in a job's last 256; -inf"),
              I("s_sub_u32", S_T[0], S_NQ, 1), I("s_lshl_b32", S_T[0], S_T[0], 8), I("s_sub_u32", S_KT0, S_N, S_T[0]),
              I("v_mov_b32", NINF, float("-inf")))
        if self.causal:
            e(comment("causal: lane constants of the diagonal mask"),
              I("v_and_b32", t0, 31, lane), I("v_lshrrev_b32", t3, 5, lane), I("v_lshlrev_b32", t3, 2, t3),
              I("v_sub_u32", V(V_IMH), t0, t3),   # i - 4 h
              I("v_mov_b32", NINF, float("-inf")))
            e(I("v_mov_b32", V(V_T[4]), 0xFFFF0000), I("v_mov_b32", V(V_T[5]), 0x0000FFFF))
            # packed P register j of a triangle group holds keys k0 = 2 (j & 1) + 8 (j >> 1) + 4 h and k0 + 1 of query i:
            # keep both (k0 + 1 <= i), the low one only (k0 == i) or none
            for j in range(8):
                k0 = 2 * (j & 1) + 8 * (j >> 1)
                e(I("v_cmp_ge_i32", VCC, V(V_IMH), k0 + 1), I("v_cndmask_b32", t1, 0, V(V_T[4]), VCC),
                  I("v_cmp_ge_i32", VCC, V(V_IMH), k0), I("v_cndmask_b32", t2, 0, V(V_T[5]), VCC),
                  I("v_or_b32", V(V_PM[j]), t1, t2))

    # ------------------------------------------------------------------ LDS-DMA
    def dma_piece(self, which, piece, buf):
        """one 1-KiB LDS-DMA piece of the next K / V tile into ring buffer `buf`: piece j = rows 8 R .. 8 R + 7 (whole 128-byte rows)
        with R = wave + 4 j, at 1024 R of the tile image"""
        if which == "k":
            rsrc, vl, base, s32, lds0 = S_KRS, V(V_DKO), S_KDMA, S_K32, KB[buf]
        else:
            rsrc, vl, base, s32, lds0 = S_VRS, V(V_DVO), S_VDMA, S_V32, VBASE + VB[buf]
        out = []
        so = base
        if piece:
            so = S_T[5]
            out.append(I("s_add_u32", so, base, s32))
        out.append(I("s_add_u32", M0, S_LDSW, lds0 + 4096 * piece))
        pre, ld = self.buf_op("buffer_load_dwordx4", None, vl, rsrc, so, lds=1, tag=f"dma {which}{piece}")
        return out + pre + [I("s_nop", 0), ld]

    def q_stage(self, b: Reg, hh: Reg, qi: Reg):
        """Q rows of job (b, hh, qi) of this wave -> the wave's LDS slice by LDS-DMA, in the K-tile image (8 pieces of 8 rows x
        128 bytes).  Returns (descriptor / offset setup, [pieces])"""
        setup = self.make_desc(S_SQ, S_Q, S_QSB, S_QSH, b, hh, S_QSN)
        setup += [I("s_lshl_b32", S_T[0], qi, 8), I("s_lshl_b32", S_T[1], S_WAVE, 5 if self.split else 6), I("s_add_u32", S_T[0], S_T[0], S_T[1]),
                  I("s_mul_i32", S_T[2], S_T[0], S_QSN),                # byte offset of the wave's first row
                  I("s_lshl_b32", S_T[3], S_QSN, 3),                    # 8 rows
                  I("s_lshl_b32", S_T[4], S_WAVE, 14), I("s_add_u32", S_T[4], S_T[4], EPI)]
        pieces = []   # (scalar set-up, load): the set-up ends one MFMA gap, the load opens the next (the MFMA between them is the
        # wait state the M0 write needs), like the K / V pieces of phase B
        for R in range(8):
            pc = []
            if R:
                pc.append(I("s_add_u32", S_T[2], S_T[2], S_T[3]))
            if self.split and R == 4:
                # split row map: the second query block starts 128 rows behind the first (96 = 12 x 8 rows further on)
                pc += [I("s_mul_i32", S_X2, S_T[3], 12), I("s_add_u32", S_T[2], S_T[2], S_X2)]
            pc.append(I("s_add_u32", M0, S_T[4], 1024 * R))
            pre, ld = self.buf_op("buffer_load_dwordx4", None, V(V_DQ[R & 1]), S_SQ, S_T[2], lds=1, tag=f"qdma R{R}")
            pieces.append((pc + pre, ld))
        return setup, pieces

    def q_reads(self):
        """the staged Q rows -> a[64:95] (fragment (qb, ks): rows 32 qb + i, 16-byte chunk 2 ks + h, as a K row read)"""
        out = []
        for qb in range(2):
            for ks in range(4):
                out.append(I("ds_read_b128", A_Q(qb, ks), V(V_QR[ks]), offset=4096 * qb, tag=f"qread qb{qb} ks{ks}"))
        return out

    # ------------------------------------------------------------------ the two phases
    def qk_mfmas(self, Y, cinit=None, qbs=(0, 1)):
        """S^T(next) chains g = 2 qb + kb into score buffer Y: 16 MFMAs in a list of 32 SLOTS (a64's phase-A time line): MFMA
        8 qb + 2 ks + kb stands in slot 2 (8 qb + 2 ks + kb), the other slots are None (emit_phase)"""
        assert cinit is None
        out = [None] * 32
        for qb in range(2):
            for ks in range(4):
                for kb in range(2):
                    d = V(Y + 16 * (2 * qb + kb), 16)
                    m = I(self.mfma, d, A_K(kb, ks), A_Q(qb, ks), d if ks else 0, tag=f"qk g{2 * qb + kb} ks{ks}")
                    out[2 * (8 * qb + 2 * ks + kb)] = m if qb in qbs else None
        return out

    def v_reads(self, buf):
        """16 transposed reads of the V tile in VB[buf]: fragment (kstep = 2 kb + s, db), u = 0, 1: keys 32 kb + 16 s + 8 u + 4 h + 0..3"""
        out = []
        for kstep in range(4):
            for db in range(2):
                f = V_F(kstep, db)
                for u in range(2):
                    imm = VB[buf] + 128 * (16 * kstep + 8 * u)
                    out.append(I("ds_read_b64_tr_b16", f.sub(2 * u, 2), V(V_VR[db]), offset=imm, tag=f"vread ks{kstep} db{db}"))
        return out

    def k_reads(self, buf):
        out = []
        for kb in range(2):
            for ks in range(4):
                out.append(I("ds_read_b128", A_K(kb, ks), V(V_KR[ks]), offset=KB[buf] + 4096 * kb, tag=f"kread kb{kb} ks{ks}"))
        return out

    def emit_phase(self, mfmas, gaps):
        """gaps[k] = fillers behind slot k of a64's time line: (order, [insts]) with order 0 = LDS / DMA loads, 1 = exp2, 2 = the rest,
        3 = last.  Only every fourth slot holds an MFMA here (64 cycles instead of 32): the fillers, in slot order, are cut into one
        contiguous run per MFMA (the slots it stands for), and a run that is longer than its MFMA's share of the phase's issue cost
        hands its tail to the next -- the kernel is VALU-issue bound, so what matters is that no MFMA waits behind a longer run than
        its neighbours'."""
        from .isa import issue_cost
        kept = [(k, m) for k, m in enumerate(mfmas) if m is not None]
        assert kept, "a phase without MFMAs is emitted by its caller"
        n, nk = len(mfmas), len(kept)
        ents = [(min(k * nk // n, nk - 1), ins) for k in range(n) for _, ins in sorted(gaps.get(k, []), key=lambda x: x[0])]
        cost = [sum(issue_cost(x) for x in ins) for _, ins in ents]
        length = [32.0 if "32x32x16" in m.op else 16.0 for _, m in kept]
        total, share = float(sum(cost)), [sum(length[:i + 1]) / sum(length) for i in range(nk)]
        out, pos, acc = [], 0, 0.0
        for idx, (_, m) in enumerate(kept):
            out.append(m)
            # a filler never moves in FRONT of the MFMA it followed (its origin run `ob`): runs only give work to later ones
            while pos < len(ents) and ents[pos][0] <= idx and \
                    (idx == nk - 1 or "slot_buckets" in self.abl or ents[pos][0] < idx or acc + cost[pos] / 2 <= total * share[idx]):
                out += ents[pos][1]
                acc += cost[pos]
                pos += 1
        assert pos == len(ents)
        return out

    def pv_mfmas(self, X, qbs=(0, 1)):
        """O^T[qb][db] += V^T(kstep, db) . P^T(qb, kstep) with P(qb, kstep = 2 kb + s) = X + 16 (2 qb + kb) + 4 s, in a64's 40 phase-B
        slots: per k-step four products in every second of its eight product slots, then the two row sums (v_mfma_f32_16x16x32
        against the 0 / 1 operand V_ONES: register 0 of V_LACC[qb] is the lane's own 16-key sum) in the two short slots"""
        out = [None] * 40
        mfma16 = "v_mfma_f32_16x16x32_" + self.dtype
        for kstep in range(4):
            kb, s = kstep >> 1, kstep & 1
            for db in range(2):
                for qb in range(2):
                    pf = V(X + 16 * (2 * qb + kb) + 4 * s, 4)
                    out[10 * kstep + 2 * (2 * db + qb)] = I(self.mfma, A_O(qb, db), V_F(kstep, db), pf, A_O(qb, db),
                                                            tag=f"pv ks{kstep} db{db} qb{qb}") if qb in qbs else None
            for qb in range(2):
                pf = V(X + 16 * (2 * qb + kb) + 4 * s, 4)
                out[10 * kstep + 8 + qb] = I(mfma16, V(V_LACC[qb], 4), V(V_ONES, 4), pf, V(V_LACC[qb], 4), tag=f"rowsum ks{kstep} qb{qb}") \
                    if qb in qbs and "no_rowsum" not in self.abl else None
        return out

    # ------------------------------------------------------------------ epilogue of the current job

    def k_epilogue(self):
        """1 / l (one Newton step), L = m + log2 l, O^T -> rows through the wave's LDS slice -> 16-byte row stores, O^T := 0.
        A query block's 32 rows of 128 bytes leave in four stores of eight rows; the stores of the first block are sprinkled through
        the arithmetic of the second, those of the second run under the MFMAs that zero O."""
        e = self.e
        t = [V(x) for x in V_T]
        e(comment("epilogue: l, 1/l, L; O^T -> rows through the wave's LDS slice -> global; O^T := 0"))
        # (the O and L descriptors of this job were formed in the seam's last phase B: epilogue_descs)
        e(I("s_nop", 15))  # last P.V MFMAs -> accumulator reads
        l = [t[0], t[3]]
        m2 = [t[1], t[5]]
        inv = [t[2], t[4]]    # (even registers: they are read as the low word of an aligned 64-bit operand below)
        for qb in range(2):   # register 0 of the row-sum accumulator is the lane's own complete row sum (both lane halves)
            e(I("v_mov_b32", l[qb], V(V_LACC[qb])))
        for qb in range(2):
            e(I("v_rcp_f32", inv[qb], l[qb]), I("v_log_f32", m2[qb], l[qb]))
        e(I("s_nop", 0))
        for qb in range(2):
            # one Newton step: inv += inv * (1 - l * inv)
            e(I("v_fma_f32", l[qb], -l[qb], inv[qb], 1.0), I("v_add_f32", m2[qb], m2[qb], V(V_MSV[qb])))
        for qb in range(2):
            e(I("v_fma_f32", inv[qb], l[qb], inv[qb], inv[qb]), I(self.cvt, m2[qb], m2[qb], m2[qb]))
        e(self.stamp_async(0))
        # O: 4 accumulators (four consecutive columns of one query) -> 2 packed registers -> ds_write_b64 at (row i, byte
        # 64 db + 16 g4 + 8 h); one query block at a time, a batch = one 32-column block.  (S[0] already holds the next job's first
        # scores and v[128:159] its K(1): rows and temporaries are score buffer 1, whose P was consumed by the job's last P.V.)
        rows = [V(SBUF[1] + 4 * k, 4) for k in range(4)]
        tset = [[V(SBUF[1] + 32 + 16 * sidx + k) for k in range(16)] for sidx in range(2)]

        def weave(*lists):
            out, idx = [], [0] * len(lists)
            while any(idx[k] < len(lists[k]) for k in range(len(lists))):
                for k in range(len(lists)):
                    if idx[k] < len(lists[k]):
                        out.append(lists[k][idx[k]])
                        idx[k] += 1
            return out

        def sprinkle(body, extras):
            """`extras` (instruction groups) spread evenly through `body`"""
            out, n = [], len(extras)
            for k, ins in enumerate(body):
                out.append(ins)
                j0, j1 = (k * n) // len(body), ((k + 1) * n) // len(body)
                for j in range(j0, j1):
                    out += extras[j]
            return out

        def row_stores(qb, off=S_T[0], stride=S_T[1], restride=False):
            """[[instructions of one row store]] of query block qb (its rows are back in `rows`): eight rows per store.  restride:
            the 8-row stride is formed again in front of every store (scalar code that uses `stride` runs between the stores)"""
            pre, st = self.buf_op("buffer_store_dwordx4", rows[0], V(V_EO), S_SQ, off)
            out = [[I("s_mul_i32", off, S_QROW[qb], S_OSN), I("s_lshl_b32", stride, S_OSN, 3)] + pre + [st]]
            for k in range(1, 4):
                pre, st = self.buf_op("buffer_store_dwordx4", rows[k], V(V_EO), S_SQ, off)
                out.append(([I("s_lshl_b32", stride, S_OSN, 3)] if restride else []) + [I("s_add_u32", off, off, stride)] + pre + [st])
            return out

        def read_back():
            out = []
            for k in range(4):   # whole rows: row 8 k + a, 16 bytes per lane as two 8-byte reads (the row stride is 8 mod 16)
                for u in range(2):
                    out.append(I("ds_read_b64", rows[k].sub(2 * u, 2), V(V_ER), offset=8 * EPI_ROW * k + 8 * u))
            return out

        for qb in range(2):
            stages = []  # per batch: [reads, muls, packs, writes]
            for db in range(2):
                tm = tset[db & 1]
                src = A_O(qb, db)
                rd = [I("v_accvgpr_read_b32", tm[k], src.sub(k)) for k in range(16)]
                mu = [I("v_pk_mul_f32", V(tm[k].idx, 2), V(tm[k].idx, 2), V(inv[qb].idx, 2), op_sel_hi=(1, 0)) for k in range(0, 16, 2)]
                cv = []
                for g4 in range(4):
                    cv += [I(self.cvt, tm[4 * g4], tm[4 * g4], tm[4 * g4 + 1]), I(self.cvt, tm[4 * g4 + 1], tm[4 * g4 + 2], tm[4 * g4 + 3])]
                wr = [I("ds_write_b64", V(V_EW), V(tm[4 * g4].idx, 2), offset=64 * db + 16 * g4) for g4 in range(4)]
                stages.append((rd, mu, cv, wr))
            head = stages[0][0] + weave(stages[0][1], stages[1][0]) + stages[0][2] + stages[0][3]
            tail = stages[1][1] + stages[1][2] + stages[1][3]
            e(head)
            if qb == 1:
                e(self.stamp_async(2))
                # the first block's rows have been on their way back from LDS since before this block started (four of this
                # block's writes are younger): wait for them once, then the row stores through the rest of this block
                e(waitcnt(lgkmcnt=4))
                e(sprinkle(tail, row_stores(0)))
            else:
                e(tail)
            e(read_back())
            e(self.stamp_async(1 if qb == 0 else 3))
        # O^T := 0 and row sums := 0 for the next job; O on the matrix pipe: four MFMAs on zero operands clear 16 accumulators each
        z = V(V_Z, 4)
        e([I("v_mov_b32", V(V_LACC[qb] + k), 0) for qb in range(2) for k in range(4)])
        e([I("v_mov_b32", z.sub(k), 0) for k in range(4)], I("s_nop", 1))
        zero = [I(self.mfma, A_O(qb, db), z, z, 0) for qb in range(2) for db in range(2)]
        # (offset / stride registers the job bookkeeping below leaves alone: k_promote and k_advance use S_T[0..4], [6], [7])
        st1 = row_stores(1, off=S_T[5], stride=S_T[6], restride=True)
        e(zero[0])
        e(self.stamp_async(4))
        e(waitcnt(lgkmcnt=0))
        e(self.stamp_async_flush((13, 14, 15, 20, 21)))   # (before the scalar code below: it uses the stamp registers)
        # L store (lanes 0..31), in the I/O dtype: in front of the job bookkeeping (it needs this job's row numbers and S_T)
        e(I("s_lshr_b64", EXEC, EXEC, 32))
        for qb in range(2):
            pre, st = self.buf_op("buffer_store_short", m2[qb], V(V_L2), S_NVRS, S_T[0])
            e(I("s_lshl_b32", S_T[0], S_QROW[qb], 1), pre, st)
        e(I("s_mov_b64", EXEC, -1))
        for k in range(4):
            e(st1[k])
            if k < 3:
                e(zero[1 + k])
            if k == 0:
                # Job bookkeeping in the shadow of the row stores: the next job becomes the current one and the job after it is
                # decoded.  S_FINAL still says "this job is the workgroup's last" for the branch behind the epilogue: it is put
                # aside in S_FLAG (idle between steps)
                l_last = self.lab("epi_last")
                e(I("s_mov_b32", S_FLAG, S_FINAL), I("s_cmp_lg_u32", S_FINAL, 0), I("s_cbranch_scc1", Label(l_last)))
                self.k_promote()
                self.k_advance(vt=(tset[0][4], tset[0][5]))
                e(label(l_last))


def product_gens():
    """the kernels of this generator that ship in libfa2_hip.so's code object (built by fa2_a64_gen.main)"""
    out = []
    for dtype in ("bf16", "f16"):
        for causal in (False, True):
            for ragged in (False, True):
                g = Gen(dtype, causal, ragged=ragged)
                g.build()
                out.append(g)
    return out
