#!/usr/bin/env python3
"""Generator of the gfx950 assembly kernels `fa2_fwd_a64_<dtype>_<c|n>` -- FA-2 forward, d = 128, f16 / bf16.

Reference arithmetic: /root/reference/src/flash_attention_kernels.py:84-108 (exp2-domain online softmax in fp32, P rounded
RTNE to the I/O dtype before P.V, O /= l once at the end, L = m + log2 l), as in fa2_mfma16h.hip.

Structure (cdna_hip_programming.md, "4-wave, one-wave-per-SIMD, persistent structure"):
  * workgroup = 4 waves = one 256-row Q block; a wave owns two 32-row query blocks (qb = 0, 1) and the WHOLE 512-entry
    register file: O^T in a[0:127], Q in a[128:191], the V^T fragments in a[192:255]; two score buffers, the current
    K tile and the softmax state in the arch VGPRs;
  * swapped products: S^T[key][query] = K.Q^T, O^T[d][query] += V^T.P^T on v_mfma_f32_32x32x16 -- a lane owns one query
    row per query block, P never leaves the registers (the S accumulator, packed in place, is the B operand of P.V);
  * 64-key K/V tiles arrive by LDS-DMA (buffer_load ... lds) into rings of FOUR K and four V buffers; LDS image = 8-row x
    32-column subtiles of 512 B with the 16-byte slots XOR-swizzled (T10 image (a)): row reads (ds_read_b128) and
    transposed reads (ds_read_b64_tr_b16) are conflict-free and need two per-lane base registers each, the rest is an
    immediate;
  * per tile t two phases of 32 MFMAs:  A(t) = QK^T(t+1) || finish-softmax(t) (exp2, row sums, cvt) || V(t) tr-reads
                                        B(t) = P.V(t)    || start-softmax(t+1) (row max, decision, s*c - m) || K(t+2) reads
                                                         || LDS-DMA of V(t+3), K(t+4)
    ONE barrier per tile (between A and B) behind a COUNTED `s_waitcnt vmcnt(8)`: a tile's DMA pieces have two tile steps
    to land.  The loop body is four tiles (buffer indices and score-buffer parity are immediates);
  * the tile stream is CONTINUOUS across jobs: every job has a multiple of four tiles, and its last body (the "seam")
    already streams the next job's K(0..3), V(0..2) and Q rows and computes its first QK^T; only the epilogue (O through
    the wave's LDS slice, L) sits between two jobs;
  * persistent grid: a workgroup walks its jobs (non-causal: one Q block; causal: the pair (nq-1-u, u)).

The instruction stream is built as isa.Inst objects: printed to a .s file for the assembler, checked by check.py (wait
states) and executed by emu.py in the CPU test-suite (tests/test_asm_emu.py) against an fp64 reference.
"""
from __future__ import annotations

import argparse
import sys

from .isa import A, EXEC, I, Label, M0, Reg, S, V, VCC, comment, label, waitcnt
from .stream_gen import (KARG_SIZE, NSLOT, SBUF, S_DBG, S_FINAL, S_FLAG, S_JOB, S_K32, S_K64, S_KARG, S_KDMA, S_KRS, S_KSN,
                         S_KT0, S_KW, S_LDSW, S_LG, S_N, S_NQ, S_NVRS, S_OSN, S_PASS, S_Q, S_QROW, S_QSB, S_QSH, S_QSN, S_SQ,
                         S_T, S_V32, S_V64, S_VDMA, S_VRS, S_VSN, S_VW, S_WAVE, S_WGID, S_X2, StreamGen, module_text)

# ------------------------------------------------------------------------------------------------- register map
# arch VGPRs
# SBUF = (0, 64) (stream_gen): two score buffers of 64 registers: group g = 2*qb + kb at +16 g
VF = 128                  # V^T fragments: (kstep, db) at VF + 4 * (4 * kstep + db)
V_KRE, V_KRO = 192, 193   # K row-read lane bases (even / odd k-step)
V_VR0, V_VR1 = 194, 195   # V transposed-read lane bases (u = 0 / 1), the V ring's LDS offset included
V_DKO, V_DVO = 196, 197   # LDS-DMA per-lane source offsets (K / V row stride)
V_MC = (198, 199)         # running row maximum in the exp2 domain (c * max), per query block
V_RS = ((200, 201), (202, 203))  # (unused: the row sums live in V_LACC)
V_MX = ((204, 205), (206, 207))  # row-max chains [qb][kb]
V_CO = (208, 209)         # rescale coefficient per query block
V_T = tuple(range(210, 220))     # temporaries (V_T[2] = v212 is 4-aligned: a zero MFMA operand in the epilogue)
V_QOFF = 220              # (unused)
V_LANE = 221
V_EW = 222                # epilogue LDS write base (row i, +8h)
V_ESW = 223               # (unused)
V_ER = 224                # epilogue LDS read base
V_EO = 225                # epilogue global store lane offset (os_n)
V_L2 = 226                # L store lane offset
V_ST_LAST, V_ST_ACC = 227, 228   # diagnostic builds: last stamp (low word), accumulators [3] (228..230)
V_NINF = 231              # causal: -inf (a literal would be the second constant-bus operand beside VCC)
NINF = V(V_NINF)
V_DKO2, V_DVO2 = 232, 233  # V_DKO / V_DVO + 128 (second half of an 8-row piece)
V_LSV = (234, 235)        # [0]: read-back address of the epilogue; [1] = V_PM[5] in the causal kernels
V_MSV = (236, 237)        # running maximum of the finished job
V_ONES = 244              # 4 registers: the 0 / 1 A operand of the row-sum MFMA (v_mfma_f32_16x16x32)
V_LACC = (248, 252)       # row-sum accumulators of the two query blocks (4 registers each; register 0 = the lane's own row)
V_DQE, V_DQO = 240, 241   # LDS-DMA per-lane source offsets of the Q rows (row stride qs_n; even / odd 8-row group)
V_QRE, V_QRO = 242, 243   # Q row-read lane bases in the wave's slice (even / odd k-step)
V_IMH = 238               # causal: i - 4 h (query row inside a 32-row block minus the lane half's key offset)
V_PM = (200, 201, 202, 203, 220, 235, 221, 239)   # causal: AND masks of the eight packed P registers of a triangle group (221 =
#                           V_LANE, dead after the set-up)


# AGPRs
def A_O(qb, db):
    return A((qb * 4 + db) * 16, 16)


def A_Q(qb, ks):
    return A(128 + (qb * 8 + ks) * 4, 4)


def A_K(kb, ks):
    # the K tile lives in ARCH VGPRs v[128:191]: ds_read into accumulator registers while MFMAs write accumulators was
    # measured 470 cycles per tile slower (and skews the four waves at the barrier)
    return V(VF + (kb * 8 + ks) * 4, 4)


def V_F(kstep, db):
    # V^T fragments in a[192:255]: read in phase A, whose MFMAs (QK^T) write arch VGPRs
    return A(192 + 4 * (4 * kstep + db), 4)


# SGPRs: the map shared by all four families is stream_gen's.
S_NDESC, S_DESC = S(98), S(99)   # (product builds: the debug pointer's registers) causal: the next / the current job walks its
#                                  non-diagonal key tiles in DESCENDING order (k_decode_next)

# LDS map (bytes)
KB = (0, 16384)
VBASE = 32768
VB = (0, 16384)                  # relative to VBASE (folded into the V read lane bases; absolute for the DMA)
EPI = 65536                      # + 16384 * wave: the wave's private 64 x 256-byte slice: the next job's Q rows land here by
                                 # LDS-DMA (K-tile image) on their way to a[128:191]; later the job's O rows leave through it
EPI_ROW = 272                    # (= 256 + 16, formed with shifts in k_setup) byte stride of an O row in the slice during the epilogue (k_setup)
LDS_TOTAL = 131072


class Gen(StreamGen):
    # the family's registers and LDS size, as the shared stream methods read them (stream_gen.StreamGen)
    V_T, V_ST_LAST, V_ST_ACC, V_MC, V_MX, V_CO, V_MSV, V_LACC, V_LANE, V_IMH, V_PM, NINF = \
        V_T, V_ST_LAST, V_ST_ACC, V_MC, V_MX, V_CO, V_MSV, V_LACC, V_LANE, V_IMH, V_PM, NINF
    S_NDESC, S_DESC = S_NDESC, S_DESC
    LDS_TOTAL = LDS_TOTAL
    FAMILY, MFMA = "a64", "v_mfma_f32_32x32x16_{dtype}"
    CVT = {"bf16": "v_cvt_pk_bf16_f32", "f16": "v_cvt_pk_f16_f32"}
    DMA_PIECES, K_READS, V_READS = 4, 16, 32
    DMA_GAPS = (11, 13, 15, 17, 21, 23, 25, 27)
    # the seam's sixteen Q-staging pieces: eight behind step 0's own K / V pieces, four in the quiet end of the next phase A, four in
    # front of step 1's own (vmcnt(8 / 12 + ...))
    QS_GAPS = ((1, 3, 5, 7, 11, 13, 15, 17), (21, 23, 25, 27, 31, 33, 35, 37), (24, 26, 28, 30), (1, 3, 5, 7), 12)
    O_AGPRS, ROW_BYTES, L_SN = 128, 256, 2
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
          I("s_lshl_b32", S_LDSW, S_WAVE, 11))
        # i = lane & 31, h = lane >> 5
        # ---- K row-read bases: 2048 (i >> 3) + 64 (i & 7) + 16 ((2 e + h) ^ ((i >> 2) & 3))
        e(comment("K row-read lane bases"),
          I("v_and_b32", t0, 31, lane),                    # i
          I("v_lshrrev_b32", t1, 3, t0), I("v_lshlrev_b32", t1, 11, t1),   # 2048 (i >> 3)
          I("v_and_b32", t2, 7, t0), I("v_lshl_add_u32", t1, t2, 6, t1),   # + 64 (i & 7)
          I("v_bfe_u32", t2, t0, 2, 2),                    # g = (i >> 2) & 3
          I("v_lshrrev_b32", t3, 5, lane),                 # h
          I("v_xor_b32", t2, t2, t3),                      # h ^ g          (even k-step: chunk slot (0 + h) ^ g)
          I("v_lshl_add_u32", V(V_KRE), t2, 4, t1),
          I("v_xor_b32", t2, 2, t2),                       # (2 + h) ^ g
          I("v_lshl_add_u32", V(V_KRO), t2, 4, t1))
        # ---- V transposed-read bases: VBASE + 64 (4 h + q) + 16 ((2 w + (p >> 1)) ^ ((2 u + h) & 3)) + 8 (p & 1)
        #      w = (lane >> 4) & 1, q = (lane >> 2) & 3, p = lane & 3
        e(comment("V transposed-read lane bases"),
          I("v_bfe_u32", t0, lane, 2, 2),                  # q
          I("v_lshrrev_b32", t3, 5, lane),                 # h
          I("v_lshl_add_u32", t0, t3, 2, t0),              # 4 h + q
          I("v_lshlrev_b32", t0, 6, t0),                   # 64 (4 h + q)
          I("v_and_b32", t1, 1, lane), I("v_lshl_add_u32", t0, t1, 3, t0),  # + 8 (p & 1)
          I("v_add_u32", t0, VBASE, t0),
          I("v_bfe_u32", t1, lane, 4, 1), I("v_lshlrev_b32", t1, 1, t1),    # 2 w
          I("v_bfe_u32", t2, lane, 1, 1), I("v_or_b32", t1, t1, t2),        # 2 w + (p >> 1)
          I("v_xor_b32", t2, t1, t3),                      # u = 0: ^ h
          I("v_lshl_add_u32", V(V_VR0), t2, 4, t0),
          I("v_xor_b32", t2, 2, t2),                       # u = 1: ^ (2 + h)
          I("v_lshl_add_u32", V(V_VR1), t2, 4, t0))
        # ---- LDS-DMA lane source offsets: l' = lane & 31: row_in = l' >> 2, slot = l' & 3, sub = lane >> 5
        #      chunk = 4 sub + (slot ^ (2 (wave & 1) + (l' >> 4)));  offset = row_in * stride + 16 chunk
        e(comment("LDS-DMA per-lane source offsets"),
          I("v_and_b32", t0, 3, lane),                     # slot
          I("v_bfe_u32", t1, lane, 4, 1),                  # l' >> 4
          I("s_and_b32", S_T[0], S_WAVE, 1), I("s_lshl_b32", S_T[0], S_T[0], 1),
          I("v_or_b32", t1, S_T[0], t1),
          I("v_xor_b32", t0, t0, t1),
          I("v_lshrrev_b32", t1, 5, lane), I("v_lshl_or_b32", t0, t1, 2, t0),   # 4 sub + ...
          I("v_lshlrev_b32", t0, 4, t0),                   # 16 chunk
          I("v_bfe_u32", t1, lane, 2, 3))                  # row_in
        e(waitcnt(lgkmcnt=0, comment="kernel arguments are in"))
        e(I("v_mul_lo_u32", t2, t1, S_KSN), I("v_add_u32", V(V_DKO), t2, t0), I("v_add_u32", V(V_DKO2), 128, V(V_DKO)),
          I("v_mul_lo_u32", t2, t1, S_VSN), I("v_add_u32", V(V_DVO), t2, t0), I("v_add_u32", V(V_DVO2), 128, V(V_DVO)))
        # ---- Q rows: the same piece shape for the 8-row groups R = 0..7 of the wave's 64 rows; the slot XOR is 2 (R & 1) + (l' >> 4)
        e(comment("Q staging: LDS-DMA lane offsets (even / odd row group) and row-read bases in the wave's slice"),
          I("v_and_b32", t0, 3, lane), I("v_bfe_u32", t2, lane, 4, 1),
          I("v_xor_b32", t3, t0, t2),                       # even R: slot ^ (l' >> 4)
          I("v_lshrrev_b32", t2, 5, lane), I("v_lshl_or_b32", t3, t2, 2, t3), I("v_lshlrev_b32", t3, 4, t3),
          I("v_mul_lo_u32", t2, t1, S_QSN), I("v_add_u32", V(V_DQE), t2, t3),
          I("v_xor_b32", t3, 32, t3),                       # odd R: slot ^ (2 + (l' >> 4)): bit 1 of the slot = bit 5 of 16 * chunk
          I("v_add_u32", V(V_DQO), t2, t3),
          I("s_lshl_b32", S_T[0], S_WAVE, 14), I("s_add_u32", S_T[0], S_T[0], EPI),
          I("v_add_u32", V(V_QRE), S_T[0], V(V_KRE)), I("v_add_u32", V(V_QRO), S_T[0], V(V_KRO)))
        # ---- epilogue: the wave's slice holds a query block's 32 O rows at a stride of EPI_ROW = 272 bytes (256 + 16: the
        #      8-byte writes of a column group and the 16-byte row reads both spread over all banks, and every address is a lane
        #      base plus an immediate).  Write base EPI + 16384 wave + 272 i + 8 h
        e(comment("epilogue lane constants"),
          I("v_and_b32", t0, 31, lane), I("v_lshrrev_b32", t3, 5, lane),
          I("v_lshlrev_b32", t1, 8, t0), I("v_lshl_add_u32", t1, t0, 4, t1),    # 272 i
          I("v_lshl_add_u32", t1, t3, 3, t1), I("v_add_u32", V(V_EW), S_T[0], t1))
        # read-back: a = lane >> 4, ec = lane & 15: base + 272 a + 16 ec (+ 4 x 272 k: row 4 k + a); store offset a * os_n + 16 ec
        e(I("v_lshrrev_b32", t0, 4, lane), I("v_and_b32", t1, 15, lane),
          I("v_lshlrev_b32", t2, 8, t0), I("v_lshl_add_u32", t2, t0, 4, t2),    # 272 a
          I("v_lshl_add_u32", t2, t1, 4, t2), I("v_add_u32", V(V_ER), S_T[0], t2),
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
        """one 1-KiB LDS-DMA piece of the next K / V tile into ring buffer `buf`.  piece j: rows 8 R .. 8 R + 7 with
        R = wave (j < 2) or wave + 4, 128-byte half j & 1 (the +128 rides in the second lane-offset register)"""
        if which == "k":
            rsrc, vl, vl2, base, s32, lds0 = S_KRS, V(V_DKO), V(V_DKO2), S_KDMA, S_K32, KB[buf]
        else:
            rsrc, vl, vl2, base, s32, lds0 = S_VRS, V(V_DVO), V(V_DVO2), S_VDMA, S_V32, VBASE + VB[buf]
        out = []
        so = base
        if piece >= 2:
            so = S_T[5]
            out.append(I("s_add_u32", so, base, s32))
        out.append(I("s_add_u32", M0, S_LDSW, lds0 + (0, 1024, 8192, 9216)[piece]))
        pre, ld = self.buf_op("buffer_load_dwordx4", None, vl2 if piece & 1 else vl, rsrc, so, lds=1, tag=f"dma {which}{piece}")
        return out + pre + [I("s_nop", 0), ld]

    def q_stage(self, b: Reg, hh: Reg, qi: Reg):
        """Q rows of job (b, hh, qi) of this wave -> the wave's LDS slice by LDS-DMA, in the K-tile image (16 pieces of 8 rows x
        128 bytes: coalesced, ~25 cycles of issue each; the same rows fetched straight into the MFMA operand layout -- 32 rows x
        32 bytes per instruction -- cost ~210 cycles per load).  Returns (descriptor / offset setup, [pieces])"""
        setup = self.make_desc(S_SQ, S_Q, S_QSB, S_QSH, b, hh, S_QSN)
        setup += [I("s_lshl_b32", S_T[0], qi, 8), I("s_lshl_b32", S_T[1], S_WAVE, 5 if self.split else 6), I("s_add_u32", S_T[0], S_T[0], S_T[1]),
                  I("s_mul_i32", S_T[2], S_T[0], S_QSN),                # byte offset of the wave's first row
                  I("s_lshl_b32", S_T[3], S_QSN, 3),                    # 8 rows
                  I("s_lshl_b32", S_T[4], S_WAVE, 14), I("s_add_u32", S_T[4], S_T[4], EPI)]
        pieces = []   # (scalar set-up, load): the set-up ends one MFMA gap, the load opens the next (the MFMA between them is the
        # wait state the M0 write needs), like the K / V pieces of phase B
        for R in range(8):
            for half in range(2):
                pc = []
                so = S_T[2]
                if self.split and R == 4 and not half:
                    # split row map: the second query block starts 128 rows behind the first (96 = 12 x 8 rows further on)
                    pc += [I("s_mul_i32", S_X2, S_T[3], 12), I("s_add_u32", S_T[2], S_T[2], S_X2)]
                if half:
                    so = S_T[5]
                    pc.append(I("s_add_u32", so, S_T[2], 128))
                    if R < 7:
                        pc.append(I("s_add_u32", S_T[2], S_T[2], S_T[3]))
                pc.append(I("s_add_u32", M0, S_T[4], 2048 * R + 1024 * half))
                pre, ld = self.buf_op("buffer_load_dwordx4", None, V(V_DQO if R & 1 else V_DQE), S_SQ, so, lds=1, tag=f"qdma R{R} h{half}")
                pieces.append((pc + pre, ld))
        return setup, pieces

    def q_reads(self):
        """the staged Q rows -> a[128:191] (fragment (qb, ks) = rows 32 qb + i, 16-byte chunk 2 ks + h, as a K row read)"""
        out = []
        for qb in range(2):
            for ks in range(8):
                out.append(I("ds_read_b128", A_Q(qb, ks), V(V_QRO if ks & 1 else V_QRE), offset=8192 * qb + 512 * (ks >> 1), tag=f"qread qb{qb} ks{ks}"))
        return out

    # ------------------------------------------------------------------ the two phases
    def qk_mfmas(self, Y, cinit=None, qbs=(0, 1)):
        """S^T(next) chains g = 2 qb + kb into score buffer Y.  cinit[g]: None -> C = 0, Reg -> C operand of the first MFMA.
        qbs: the query blocks whose chains are computed -- the others' MFMAs are None in the returned list (emit_phase)"""
        out = []
        if "qk_chain_order" in self.abl:     # (the round's first order: one chain after the other)
            order = [(g, ks) for g in range(4) for ks in range(8)]
        else:
            # the two chains of a query block interleaved: consecutive MFMAs share their B operand (the Q fragment) -- half the
            # operand toggling of the matrix pipe's inputs, and no MFMA follows the one it accumulates onto
            order = [(2 * qb + kb, ks) for qb in range(2) for ks in range(8) for kb in range(2)]
        for g, ks in order:
            qb, kb = g >> 1, g & 1
            d = V(Y + 16 * g, 16)
            c = d if ks else (cinit[g] if cinit and cinit[g] is not None else 0)
            out.append(I(self.mfma, d, A_K(kb, ks), A_Q(qb, ks), c, tag=f"qk g{g} ks{ks}") if qb in qbs else None)
        return out

    def v_reads(self, buf):
        """32 transposed reads of the V tile in VB[buf]: fragment (kstep, db) <- u = 0, 1"""
        out = []
        for kstep in range(4):
            for db in range(4):
                f = V_F(kstep, db)
                for u in range(2):
                    imm = VB[buf] + 2048 * (2 * kstep + u) + 512 * db
                    out.append(I("ds_read_b64_tr_b16", f.sub(2 * u, 2), V(V_VR1 if u else V_VR0), offset=imm, tag=f"vread ks{kstep} db{db}"))
        return out

    def k_reads(self, buf):
        out = []
        for kb in range(2):
            for ks in range(8):
                imm = KB[buf] + 8192 * kb + 512 * (ks >> 1)
                out.append(I("ds_read_b128", A_K(kb, ks), V(V_KRO if ks & 1 else V_KRE), offset=imm, tag=f"kread kb{kb} ks{ks}"))
        return out

    def emit_phase(self, mfmas, gaps):
        """gaps[k] = fillers behind MFMA k: (order, [insts]) with order 0 = LDS / DMA loads, 1 = exp2, 2 = the rest, 3 = last"""
        out = []
        kept = [k for k, m in enumerate(mfmas) if m is not None]
        if len(kept) == len(mfmas):
            for k, m in enumerate(mfmas):
                out.append(m)
                for _, ins in sorted(gaps.get(k, []), key=lambda x: x[0]):
                    out += ins
            return out
        # some MFMAs are left out (a query block the tile is hidden from): the fillers of the original gaps, each gap's group
        # kept whole and in the original order, are spread over the remaining MFMAs in proportion -- a filler never moves in
        # front of an MFMA it followed (check.fix pads what lands too close behind one)
        n, nk = len(mfmas), len(kept)
        assert nk > 0, "a phase without MFMAs is emitted by its caller"
        buckets = [[] for _ in range(nk)]
        for k in range(n):
            for _, ins in sorted(gaps.get(k, []), key=lambda x: x[0]):
                buckets[min(k * nk // n, nk - 1)] += ins
        for idx, k in enumerate(kept):
            out.append(mfmas[k])
            out += buckets[idx]
        return out

    def pv_mfmas(self, X, qbs=(0, 1)):
        """O^T[qb][db] += V^T(kstep, db) . P^T(qb, kstep) with P(qb, kstep = 2 kb + s) = X + 16 (2 qb + kb) + 4 s; behind each
        k-step the row sums of its two P fragments on the matrix pipe: a 16x16x32 MFMA against the 0 / 1 operand V_ONES puts
        the 16-key sum of the lane's own query into register 0 of V_LACC[qb] (fa2_mfma16h.hip, FA2_H_MSUM, has the lane maths)"""
        out = []
        mfma16 = "v_mfma_f32_16x16x32_" + self.dtype
        for kstep in range(4):
            kb, s = kstep >> 1, kstep & 1
            for db in range(4):
                for qb in range(2):
                    pf = V(X + 16 * (2 * qb + kb) + 4 * s, 4)
                    out.append(I(self.mfma, A_O(qb, db), V_F(kstep, db), pf, A_O(qb, db), tag=f"pv ks{kstep} db{db} qb{qb}")
                               if qb in qbs else None)
            for qb in range(2):
                pf = V(X + 16 * (2 * qb + kb) + 4 * s, 4)
                out.append(I(mfma16, V(V_LACC[qb], 4), V(V_ONES, 4), pf, V(V_LACC[qb], 4), tag=f"rowsum ks{kstep} qb{qb}")
                           if qb in qbs and "no_rowsum" not in self.abl else None)   # (no_rowsum: timing-only, l stays 0)
        return out

    # ------------------------------------------------------------------ epilogue of the current job

    def k_epilogue(self):
        """1 / l (one Newton step), L = m + log2 l, O^T -> rows through the wave's LDS slice -> 16-byte row stores, O^T := 0.
        A workgroup's O tile is 64 KiB and the CU's vector-memory path takes 64 bytes per cycle: the row stores of the first
        query block are sprinkled through the arithmetic of the second (back to back they cost ~85 cycles each with all four
        waves storing at once), those of the second run under the MFMAs that zero O and the L arithmetic that is left."""
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
        self.atmp_regs = (V_T[0], V_T[3])     # (the row sums are consumed: V_T[6..9] are LDS addresses from here on)
        # O: 4 accumulators -> 2 packed registers -> ds_write_b64 at (row i, chunk 4 db + g4, +8 h); one query block at a time.
        # (S[0] already holds the next job's first scores and v[128:191] its K(1): rows and temporaries are score buffer 1,
        # whose P was consumed by the job's last P.V.)  A batch = the four 8-byte groups of one 32-column block; the stages
        # of consecutive batches (accumulator reads | scale | pack, address | LDS write) are woven so that no instruction
        # waits on its predecessor.
        rows = [V(SBUF[1] + 4 * k, 4) for k in range(8)]
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
            """[[instructions of one row store]] of query block qb (its rows are back in `rows`).  restride: the 4-row stride is
            formed again in front of every store (scalar code that uses `stride` runs between the stores)"""
            omods = dict(nt=1) if "o_nt" in self.abl else dict(sc1=1) if "o_sc1" in self.abl else {}    # (A/B: streaming O stores)
            pre, st = self.buf_op("buffer_store_dwordx4", rows[0], V(V_EO), S_SQ, off, **omods)
            out = [[I("s_mul_i32", off, S_QROW[qb], S_OSN), I("s_lshl_b32", stride, S_OSN, 2)] + pre + [st]]
            for k in range(1, 8):
                pre, st = self.buf_op("buffer_store_dwordx4", rows[k], V(V_EO), S_SQ, off, **omods)
                out.append(([I("s_lshl_b32", stride, S_OSN, 2)] if restride else []) + [I("s_add_u32", off, off, stride)] + pre + [st])
            return out

        def read_back():
            out = []
            for k in range(8):   # whole rows: row 4 k + a
                out.append(I("ds_read_b128", rows[k], V(V_ER), offset=4 * EPI_ROW * k))
            return out

        for qb in range(2):
            stages = []  # per batch: [reads, muls + address, packs, writes]
            for db in range(4):
                tm = tset[db & 1]
                src = A_O(qb, db)
                rd = [I("v_accvgpr_read_b32", tm[k], src.sub(k)) for k in range(16)]
                # (packed fp32 multiplies: half the instructions; beside an MFMA they would cost ~50 cycles each, here the
                # matrix pipe is idle and every VALU instruction takes the same ~5.8 cycles at one wave per SIMD)
                mu = [I("v_pk_mul_f32", V(tm[k].idx, 2), V(tm[k].idx, 2), V(inv[qb].idx, 2), op_sel_hi=(1, 0)) for k in range(0, 16, 2)]
                cv = []
                for g4 in range(4):
                    cv += [I(self.cvt, tm[4 * g4], tm[4 * g4], tm[4 * g4 + 1]), I(self.cvt, tm[4 * g4 + 1], tm[4 * g4 + 2], tm[4 * g4 + 3])]
                wr = [I("ds_write_b64", V(V_EW), V(tm[4 * g4].idx, 2), offset=16 * (4 * db + g4)) for g4 in range(4)]
                stages.append((rd, mu, cv, wr))
            # software pipeline over the four batches (two register sets): batch b + 1 is read while batch b is scaled, ...
            head = stages[0][0] + weave(stages[0][1], stages[1][0]) + stages[0][2] + stages[0][3]
            tail = weave(stages[1][1], stages[2][0]) + stages[1][2] + stages[1][3] + weave(stages[2][1], stages[3][0]) + \
                stages[2][2] + stages[2][3] + stages[3][1] + stages[3][2] + stages[3][3]
            e(head)
            if qb == 1:
                e(self.stamp_async(2))
                # the first block's rows have been on their way back from LDS since before this block started (four of this
                # block's writes are younger): wait for them once, then one row store every ~25 instructions
                e(waitcnt(lgkmcnt=4))
                e(sprinkle(tail, row_stores(0)))
            else:
                e(tail)
            e(read_back())
            e(self.stamp_async(1 if qb == 0 else 3))
        # O^T := 0 and row sums := 0 for the next job; O on the matrix pipe (8 MFMAs instead of 128 v_accvgpr_write)
        z = V(SBUF[1] + 32, 4)    # (the second block's temporaries: free again)
        e([I("v_mov_b32", V(V_LACC[qb] + k), 0) for qb in range(2) for k in range(4)])
        e([I("v_mov_b32", z.sub(k), 0) for k in range(4)], I("s_nop", 1))
        # (the wave can issue one of these every 32 cycles and one row store every ~75 with all four waves storing: interleaved,
        # the stores hide the MFMAs; two MFMAs go first, under the read-back's LDS round trip)
        zero = [I(self.mfma, A_O(qb, db), z, z, 0) for qb in range(2) for db in range(4)]
        # (offset / stride registers the job bookkeeping below leaves alone: k_promote and k_advance use S_T[0..4], [6], [7])
        st1 = row_stores(1, off=S_T[5], stride=S_T[6], restride=True)
        e(zero[0], zero[1])
        e(self.stamp_async(4))
        e(waitcnt(lgkmcnt=0))
        e(self.stamp_async_flush((13, 14, 15, 20, 21)))   # (before the scalar code below: it uses the stamp registers)
        # L store (lanes 0..31), in the I/O dtype: in front of the job bookkeeping (it needs this job's row numbers and S_T)
        e(I("s_lshr_b64", EXEC, EXEC, 32))
        for qb in range(2):
            pre, st = self.buf_op("buffer_store_short", m2[qb], V(V_L2), S_NVRS, S_T[0])
            e(I("s_lshl_b32", S_T[0], S_QROW[qb], 1), pre, st)
        e(I("s_mov_b64", EXEC, -1))
        for k in range(8):
            e(st1[k])
            if k + 2 < 8:
                e(zero[k + 2])
            if k == 1:
                # Job bookkeeping in the shadow of the row stores (the vector-memory path takes ~75 cycles per store with four
                # waves storing: the scalar code runs while the first two drain): the next job becomes the current one and the
                # job after it is decoded -- ~200 cycles that used to stand in front of the seam.  S_FINAL still says "this
                # job is the workgroup's last" for the branch behind the epilogue: it is put aside in S_FLAG (idle between steps)
                l_last = self.lab("epi_last")
                e(I("s_mov_b32", S_FLAG, S_FINAL), I("s_cmp_lg_u32", S_FINAL, 0), I("s_cbranch_scc1", Label(l_last)))
                self.k_promote()
                self.k_advance(vt=(tset[0][4], tset[0][5]))     # (not z: SBUF[1] + 32..35 is the zero MFMAs' operand)
                e(label(l_last))
        self.atmp_regs = (V_T[8], V_T[9])


ABLATIONS = {"novmwait": ("novmwait",), "nobarrier": ("nobarrier",),
             "nodma": ("nodma",), "nokread": ("nokread",), "nostart": ("nostart",), "nofinish": ("nofinish",),
             "novread": ("novread",), "mfmaonly": ("nodma", "nokread", "nostart", "nofinish", "novread"),
             "nomx": ("no_mx",), "nodec": ("no_dec",), "nofire": ("no_fire",), "nof": ("no_f",), "noe": ("no_e",), "nocv": ("no_cv",),
             "nofecv": ("no_f", "no_e", "no_cv"), "nolds": ("nokread", "novread", "nodma"),
             "nobar_nostart": ("nobarrier", "nostart"), "nobar_nolds": ("nobarrier", "nokread", "novread", "nodma"),
             "skew": ("skew",), "valuonly": ("nokread", "novread", "nodma", "no_fire"),
             "fire_nobranch": ("fire_nobranch",)}


# named variants of the experiments build (make experiments; FA2_A64_KERNEL=fa2_fwd_a64_bf16_<c|n>_<tag> selects one per launch:
# benchmarks/variants.py interleaves them in one process, which resolves +-0.3 % -- across gpurun calls boxes differ by 7 %).
# Measured that way on c3 causal: nolean -1.0 %; plan capacities (6, 26) / (6, 24) / (5, 26) / (5, 25) +-0.3 %, (7, 28) -1.7 %;
# one-chain-after-the-other QK^T order -0.2 %; zero-operand K and V^T fragments for hidden tiles +0.4 % / 0 (dropped for the
# lean bodies); V reads doubled up in 2 instead of 4 gaps 0.  Split row map (the default since) against the contiguous one with
# lean bodies ("nosplit"): +0.9 / +1.1 % on two boxes, bit-identical outputs (benchmarks/a64_variant_equal.py); its DMA pieces
# issued in the first gaps of the short steps: 0.
VARIANTS = {"base": dict(), "nosplit": dict(split=False), "fullmax": dict(abl=("full_max",)), "prologue_old": dict(abl=("prologue_old",)), "o_nt": dict(abl=("o_nt",)), "o_sc1": dict(abl=("o_sc1",)),
            "norowsum": dict(abl=("no_rowsum",))}     # (norowsum: timing-only bound of what the row-sum MFMAs cost; outputs are wrong)


def module_text(gens):
    head = ['.amdgcn_target "amdgcn-amd-amdhsa--gfx950"', ".amdhsa_code_object_version 6", ".text", ""]
    body = "\n".join(head) + "\n".join(g.text() for g in gens)
    md = ["", ".amdgpu_metadata", "---", "amdhsa.kernels:"] + [g.metadata() for g in gens] + [
        "amdhsa.target: amdgcn-amd-amdhsa--gfx950", "amdhsa.version:", "  - 1", "  - 2", "...", ".end_amdgpu_metadata", ""]
    return body + "\n".join(md)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--output", required=True)
    ap.add_argument("--stamps", action="store_true", help="diagnostic build: job-timeline stamps into the debug buffer")
    ap.add_argument("--variants", action="store_true", help="experiments build: the product kernels plus named variants (A/B in one process)")
    args = ap.parse_args(argv)
    from .check import check
    gens = []
    for dtype, causal, ragged in [(dt, c, False) for dt in ("bf16", "f16") for c in (False, True)] + \
            ([] if args.stamps else [(dt, c, True) for dt in ("bf16", "f16") for c in (False, True)]):
        g = Gen(dtype, causal, stamps=args.stamps, ragged=ragged)
        g.build()
        gens.append(g)
    if not args.stamps:   # the same structure on v_mfma_f32_16x16x32 (fa2_a16_gen.py): same code object, same argument block
        from .fa2_a16_gen import product_gens
        from .fa2_a8_gen import product_gens as product_gens8
        from .fa2_a64d_gen import product_gens as product_gens_d64
        gens += product_gens() + product_gens8() + product_gens_d64()
    for g in gens:    # (the shipped kernels: wait states checked)
        errs = check(g.prog)
        if errs:
            print(f"{g.name}: {len(errs)} wait-state violations", file=sys.stderr)
            return 1
    if args.stamps:  # timing-only ablations ride in the diagnostic code object
        g = Gen("bf16", True, name="fa2_fwd_a64_bf16_c_lite", stamps=True, abl=("lite",))
        g.build()
        gens.append(g)
        g = Gen("bf16", True, name="fa2_fwd_a64_bf16_c_lite_nosplit", stamps=True, abl=("lite",), split=False)
        g.build()
        gens.append(g)
        g = Gen("bf16", True, name="fa2_fwd_a64_bf16_c_lite_noqreads", stamps=True, abl=("lite", "noqreads"))
        g.build()
        gens.append(g)
        for nm, abl in [("lite", ())] + list(ABLATIONS.items()):
            g = Gen("bf16", False, name=f"fa2_fwd_a64_bf16_n_{nm}", stamps=True, abl=tuple(abl) + ("lite",))
            g.build()
            gens.append(g)
    if args.stamps:     # ... and of the 16x16x32 form (non-causal: its stamp registers are the causal kernels' mask registers)
        from .fa2_a16_gen import Gen as Gen16
        for nm, abl in [("lite", ())] + list(ABLATIONS.items()):
            g = Gen16("bf16", False, name=f"fa2_fwd_a16_bf16_n_{nm}", stamps=True, abl=tuple(abl) + ("lite",))
            g.build()
            gens.append(g)
        g = Gen16("bf16", True, name="fa2_fwd_a16_bf16_c_lite", stamps=True, abl=("lite",))
        g.build()
        gens.append(g)
        from .fa2_a8_gen import Gen as Gen8      # ... and of the fp8 form
        g = Gen8("e4m3", False, stamps=True)     # (the plain name: the launcher looks it up before FA2_A64_KERNEL replaces it)
        g.build()
        gens.append(g)
        for nm, abl in [("lite", ())] + list(ABLATIONS.items()):
            g = Gen8("e4m3", False, name=f"fa2_fwd_a8_e4m3_n_{nm}", stamps=True, abl=tuple(abl) + ("lite",))
            g.build()
            gens.append(g)
    if args.variants:   # selected at run time through FA2_A64_KERNEL in the experiments library (benchmarks/variants.py)
        for tag, kw in VARIANTS.items():
            for causal in (False, True):
                g = Gen("bf16", causal, name=f"fa2_fwd_a64_bf16_{'c' if causal else 'n'}_{tag}", **kw)
                g.build()
                gens.append(g)
        from .fa2_a8_gen import variant_gens as variant_gens8
        gens += variant_gens8()
        g = Gen("f16", True, name="fa2_fwd_a64_f16_c_noexact", abl=("fire_noexact",))     # (A/B: the firing path without its exact-maximum exit)
        g.build()
        gens.append(g)
    with open(args.output, "w") as f:
        f.write(module_text(gens))
    return 0


if __name__ == "__main__":
    sys.exit(main())
