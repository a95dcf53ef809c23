#!/usr/bin/env python3
"""Generator of the gfx950 assembly kernels `fa2_fwd_a8_<e4m3|e5m2>_<c|n>` -- FA-2 forward, d = 128, OCP fp8 (BASELINE.json
configs[4]): the a64 structure (fa2_a64_gen.py: 4 waves x 64 query rows, one wave per SIMD with all 512 registers, persistent
grid, continuous tile stream, LDS-DMA staging, modulo-scheduled softmax) on the double-rate fp8 matrix path,
v_mfma_f32_32x32x64_f8f6f4 -- QK^T on the plain form, P.V on the BLOCK-SCALED one (Gen.scaled): the running maximum is an integer,
the O accumulators stay relative to the job's first maximum and P's E8M0 scale operand carries the power of two between them, so O is
never rescaled (a rescale costs the one wave of a SIMD ~900 cycles with the other three at the barrier; fp8 P leaves only 8.5 log2
units of deferral).

Reference arithmetic: /root/reference/src/flash_attention_kernels.py:84-108 with the reference's fp8 dtype path
(src/flash_attention_torch.py:14-15): fp32 S, m, l, O; P rounded RTNE to fp8 before P.V; O / l and L rounded to fp8 on store --
as fa2_mfma8x.hip, whose layouts (validated on the device) this kernel takes over:
  * S^T(kb, qb) = K(kb) . Q(qb)^T over d = 128 is TWO MFMAs (ks = 0, 1): a lane (row i, half h) supplies 32 bytes per step --
    the 16-byte chunks 4 ks + h and 4 ks + 2 + h of its row (k is a summation index: any assignment both operands share);
  * the accumulator layout is the 32x32 one of the bf16 kernels (lane: query i, register r: key (r & 3) + 8 (r >> 2) + 4 h), so
    the softmax plan is a64's; packed in place to fp8, the 32 P values of a lane -- k slot 16 kb + r -- are the first eight
    registers of the query block's score registers: the B operand of O^T(qb, db) += V^T(db) . P^T(qb), ONE MFMA over 64 keys;
  * the matching V^T operand is four ds_read_b64_tr_b8 (eight keys each; lane map measured in round 1,
    profiles/r01/ds_read_b64_tr_b8_lane_map.txt);
  * row sums: v_mfma_f32_16x16x128_f8f6f4 against a 0 / 1 operand (register 0 of its accumulator is the lane's own row sum).
A 64-key step is 8 + 8 MFMAs of 64 cycles and two of 32: the MFMA lists keep a64's 32 + 40 SLOTS with a real MFMA in every fourth
-- emit_phase gives each MFMA the fillers of the slots it stands for, in order -- so the time line, the seam and the job stream
are a64's.  Per step a wave issues ~1 350 cycles of softmax against 1 090 of MFMA: the kernel is VALU-issue bound.
N >= 256, ragged forms for N that is not a multiple of 256 (the other fp8 shapes stay on fa2_mfma8x.hip).  Causal: fa2_a64_gen.py's split row map, seam bodies and lazy
masking; the packed-P masks are byte masks (four keys per register), and the firing path of a lazily masked tile leaves again when
the exact maximum does not pass the threshold (the oracle's decision).
"""
from __future__ import annotations


from .isa import A, EXEC, I, Label, M0, Reg, S, V, VCC, comment, label, waitcnt
from .stream_gen import (KARG_SIZE, NSLOT, SBUF, S_C, S_DBG, S_FINAL, S_FIRE, S_FLAG, S_JOB, S_K32, S_K64, S_KARG, S_KDMA,
                         S_KRS, S_KSN, S_KT0, S_KW, S_LDSW, S_LG, S_N, S_NQ, S_NVRS, S_OSN, S_PASS, S_Q, S_QROW, S_QSB, S_QSH,
                         S_QSN, S_SQ, S_T, S_THR, S_V32, S_V64, S_VDMA, S_VRS, S_VSN, S_VW, S_WAVE, S_WGID, S_X2, StreamGen)

# ------------------------------------------------------------------------------------------------- register map
# arch VGPRs
# SBUF = (0, 64) (stream_gen): two score buffers of 64 registers: group g = 2*qb + kb at +16 g; packed P(qb): the first 8 of + 32 qb
KF = 128                  # K fragments of the next tile: (kb, ks) at KF + 8 (2 kb + ks), 8 registers each
V_KR = (160, 161, 162, 163)   # K row-read lane bases, per (ks, u): chunk 4 ks + 2 u + h
V_VR = (164, 165, 166, 167)   # V transposed-read lane bases per 32-column block db (the V ring's LDS offset included)
V_QR = (168, 169, 170, 171)   # Q row-read lane bases in the wave's slice
V_DKO, V_DVO = 172, 173   # LDS-DMA per-lane source offsets of K / V rows (the wave's piece parity folded in)
V_DQ = (174, 175)         # ... of Q rows (even / odd 8-row group)
V_MC = (176, 177)         # running row maximum in the exp2 domain (c * max), per query block
V_CO = (178, 179)         # rescale coefficient per query block
V_MX = ((180, 181), (182, 183))  # row-max chains [qb][kb]
V_MSV = (184, 185)        # running maximum of the finished job
V_LANE = 186
V_EW, V_ER, V_EO, V_L2 = 187, 188, 189, 190   # epilogue: LDS write base, LDS read base, global store lane offset, L store lane offset
V_T = tuple(range(192, 202))     # temporaries (V_T[0], [2], .. even; V_T[2] = v194 ... the zero MFMA operand is V_Z)
V_Z = 204                 # 4 registers, 4-aligned: the zero operand of the epilogue's clearing MFMAs
V_ONES = 208              # 8 registers: the 0 / 1 A operand of the row-sum MFMA (v_mfma_f32_16x16x128_f8f6f4)
V_LACC = (216, 220)       # row-sum accumulators of the two query blocks (4 registers each; register 0 = the lane's own row)
V_ST_LAST, V_ST_ACC = 224, 225   # diagnostic builds: last stamp (low word), accumulators [3]
V_NINF = 231
NINF = V(V_NINF)
# block-scaled P.V (Gen.scaled): the running maximum moves in INTEGER steps and O is never rescaled -- the power of two goes into the
# MFMA's per-lane scale operand of P instead
V_B = (232, 233)          # 127 - m_O per query block (m_O: the integer reference of the O accumulators): scale byte = m + V_B
V_SCL = (234, 235)        # the E8M0 scale byte (byte 0) of the P operands whose P.V runs: 127 + (m - m_O)
V_SCP = (236, 237)        # ... the one that takes over at the end of this phase B (a decision of the tile that starts)
V_CO2 = (238, 239)        # guard path (m - m_O would pass KMAX): the factor 2^-(m - m_O) that re-bases O
V_S127 = 240              # the scale byte of the V^T operand: 127 = 2^0
V_IMH = 241               # causal: i - 4 h (query row inside a 32-row block minus the lane half's key offset)
V_PM = (242, 243, 244, 245)   # causal: AND masks of the four packed P registers (four fp8 each) of a triangle group
KMAX = 64                 # largest m - m_O before O is re-based: 2^(64 + 8.5) N max|V| stays far inside fp32, 2^-64 / l above its denormals


# AGPRs
def A_O(qb, db):
    return A((qb * 4 + db) * 16, 16)


def A_Q(qb, ks):
    return A(128 + (qb * 2 + ks) * 8, 8)


def A_K(kb, ks):
    return V(KF + (kb * 2 + ks) * 8, 8)


def V_F(db):
    # V^T fragments in a[192:223]: read in phase A, whose MFMAs (QK^T) write arch VGPRs
    return A(192 + 8 * db, 8)


def P_OP(X, qb):
    """the packed P^T(qb): 32 fp8 per lane, k slot 16 kb + r"""
    return V(X + 32 * qb, 8)


def swz_k(row):
    """K / Q tile image: 16-byte chunk c of row r at 128 r + 16 (c ^ swz_k(r)) (fa2_mfma8x.hip)"""
    return (((row >> 1) & 1) << 2) | ((row >> 2) & 3)


def swz_v(row):
    """V tile image: 32-byte unit u of row r at 128 r + 32 (u ^ swz_v(r))"""
    return ((row >> 1) & 1) | (((row >> 3) & 1) << 1)


# SGPRs: the map shared by all four families is stream_gen's.
S_NDESC, S_DESC = S(98), S(99)   # (product builds: the debug pointer's registers) causal: the next / the current job walks its
#                                  non-diagonal key tiles in DESCENDING order (k_decode_next)

# LDS map (bytes)
KB = (0, 8192, 16384, 24576)     # rings of up to four 8-KiB buffers (Gen.R of them are used)
VBASE = 32768
VB = (0, 8192, 16384, 24576)     # relative to VBASE (folded into the V read lane bases; absolute for the DMA)
EPI = 65536                      # + 16384 * wave: the wave's private slice: the next job's 64 Q rows land here by LDS-DMA (8 KiB,
                                 # K-tile image) on their way to a[128:159]; later the job's O rows leave through it
EPI_ROW = 136                    # (= 128 + 8) byte stride of an O row in the slice during the epilogue: 8-byte aligned for the
                                 # row read-back, the 4-byte column writes of 32 lanes are 2-way (free for ds_write_b32)
LDS_TOTAL = 65536 + 4 * 16384


class Gen(StreamGen):
    # the family's registers and LDS size, as the shared stream methods read them (stream_gen.StreamGen)
    V_T, V_ST_LAST, V_ST_ACC, V_MC, V_MX, V_CO, V_MSV, V_LACC, V_LANE, V_IMH, V_PM, NINF = \
        V_T, V_ST_LAST, V_ST_ACC, V_MC, V_MX, V_CO, V_MSV, V_LACC, V_LANE, V_IMH, V_PM, NINF
    S_NDESC, S_DESC = S_NDESC, S_DESC
    LDS_TOTAL = LDS_TOTAL
    FAMILY, MFMA = "a8", "v_mfma_f32_32x32x64_f8f6f4"
    CVT = {"e4m3": "v_cvt_pk_fp8_f32", "e5m2": "v_cvt_pk_bf8_f32"}
    DMA_PIECES, K_READS, V_READS = 2, 8, 16
    DMA_GAPS = (11, 15, 21, 25)
    # the seam's eight Q-staging pieces: four behind step 0's own K / V pieces, two in the quiet end of the next phase A, two in
    # front of step 1's own; the barrier wait of step 1 leaves those six in flight
    QS_GAPS = ((1, 5, 11, 15), (21, 25, 29, 33), (24, 28), (1, 5), 6)
    O_AGPRS, ROW_BYTES, L_SN = 128, 128, 1
    BRANCH_NEED, WALK_DOWN = 20, True

    def __init__(self, dtype="bf16", causal=False, name=None, stamps=False, abl=(), ring=(2, 3, 2), vread_double=4, ragged=False,
                 caps=(5, 24), split=True, scaled=True):
        assert split or not causal, "a8: the causal kernels use the split row map"
        # scaled: P.V on v_mfma_scale_f32_32x32x64_f8f6f4.  fp8 P leaves 8.5 log2 units of deferral (e4m3 tops out at 448): on N(0, 1)
        # inputs at scale 1 (scores of sigma 16) a row's maximum passes it in a quarter of the tile steps, and a rescale of 64
        # accumulators costs the one wave of a SIMD ~900 cycles with the other three waiting at the barrier.  Here the running maximum
        # is an INTEGER (the ceiling of the row maximum in the exp2 domain), O stays relative to the job's first maximum m_O, and
        # the P operand carries 2^(m - m_O) as its E8M0 block scale: raising m costs a dozen VALU operations and no accumulator
        # access (the row sums, four registers, are scaled by an exact power of two).  The guard re-bases O when m - m_O passes KMAX.
        self.scaled = scaled
        self.fmt = dict(cbsz=1, blgp=1) if dtype == "e5m2" else {}     # operand formats of the f8f6f4 MFMAs (0 = e4m3, 1 = e5m2)
        name = name or f"fa2_fwd_a8_{dtype}_{'c' if causal else 'n'}{'r' if ragged else ''}{'' if scaled else '_unscaled'}"
        super().__init__(dtype, causal, name, stamps, abl, ring, vread_double, ragged, caps, split)

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
        for k in range(4):      # k = 2 ks + u: chunk 4 ks + 2 u + h = 2 k + h
            e(I("v_xor_b32", t2, 2 * k, t1), I("v_lshl_add_u32", V(V_KR[k]), t2, 4, t3))
        # ---- V transposed-read bases (ds_read_b64_tr_b8): in a 16-lane group lane ls = 2 s + par supplies the 8-byte segment of key
        #      row 4 h + s (s < 4) or 4 h + 8 + (s - 4) at columns 16 q16 + 8 par of the 32-column block db:
        #      VBASE + 128 row + 32 (db ^ swz_v(row)) + 16 q16 + 8 par,  swz_v(row) = ((s & 3) >> 1) | ((s >> 2) << 1)
        e(comment("V transposed-read lane bases"),
          I("v_bfe_u32", t0, lane, 1, 3),                  # s
          I("v_and_b32", t1, 3, t0), I("v_lshrrev_b32", t2, 2, t0), I("v_lshl_add_u32", t1, t2, 3, t1),   # (s & 3) + 8 (s >> 2)
          I("v_lshrrev_b32", t2, 5, lane), I("v_lshl_add_u32", t1, t2, 2, t1),                            # + 4 h = row
          I("v_lshlrev_b32", t1, 7, t1),                   # 128 row
          I("v_bfe_u32", t2, lane, 4, 1), I("v_lshl_add_u32", t1, t2, 4, t1),                             # + 16 q16
          I("v_and_b32", t2, 1, lane), I("v_lshl_add_u32", t1, t2, 3, t1),                                # + 8 par
          I("v_add_u32", t1, VBASE, t1),
          I("v_bfe_u32", t2, t0, 1, 1), I("v_lshrrev_b32", t3, 2, t0), I("v_lshl_or_b32", t2, t3, 1, t2))  # swz_v
        for db in range(4):
            e(I("v_xor_b32", t3, db, t2), I("v_lshl_add_u32", V(V_VR[db]), t3, 5, t1))
        # ---- LDS-DMA lane source offsets: a piece is 8 rows x 128 bytes (rows 8 R ..); lane i lands at row 8 R + (i >> 3), 16-byte
        #      position i & 7 of the image.  K / Q image: that position holds chunk (i & 7) ^ swz_k(row); V image: unit
        #      ((i & 7) >> 1) ^ swz_v(row), half i & 1.  Bit 3 of the row is R & 1: the wave's parity for K / V (R = wave, wave + 4)
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
        # swz_v(row) = ((row_in >> 1) & 1) | 2 (R & 1): unit (pos >> 1) ^ swz_v, half pos & 1
        e(I("v_bfe_u32", t2, t1, 1, 1), I("s_lshl_b32", S_T[1], S_T[0], 1), I("v_or_b32", t2, S_T[1], t2),
          I("v_lshrrev_b32", t3, 1, t0), I("v_xor_b32", t2, t2, t3), I("v_lshlrev_b32", t2, 5, t2),
          I("v_and_b32", t3, 1, t0), I("v_lshl_add_u32", t2, t3, 4, t2),
          I("v_mul_lo_u32", t3, t1, S_VSN), I("v_add_u32", V(V_DVO), t3, t2))
        e(comment("Q row-read bases in the wave's slice"),
          I("s_lshl_b32", S_T[0], S_WAVE, 14), I("s_add_u32", S_T[0], S_T[0], EPI))
        e([I("v_add_u32", V(V_QR[k]), S_T[0], V(V_KR[k])) for k in range(4)])
        # ---- epilogue: the wave's slice holds a query block's 32 O rows (128 bytes of fp8) at a stride of EPI_ROW = 136 bytes.
        #      Write base (row i, + 4 h): slice + 136 i + 4 h;  read-back (a = lane >> 3, ec = lane & 7): slice + 136 a + 16 ec
        #      (+ 8 x 136 k: row 8 k + a), two ds_read_b64; store offset a * os_n + 16 ec
        e(comment("epilogue lane constants"),
          I("v_and_b32", t0, 31, lane), I("v_lshrrev_b32", t3, 5, lane),
          I("v_mul_u32_u24", t1, EPI_ROW, t0), I("v_lshl_add_u32", t1, t3, 2, t1), I("v_add_u32", V(V_EW), S_T[0], t1),
          I("v_lshrrev_b32", t0, 3, lane), I("v_and_b32", t1, 7, lane),
          I("v_mul_u32_u24", t2, EPI_ROW, t0), I("v_lshl_add_u32", t2, t1, 4, t2), I("v_add_u32", V(V_ER), S_T[0], t2),
          I("v_mul_lo_u32", t2, t0, S_OSN), I("v_lshl_add_u32", V(V_EO), t1, 4, t2),
          I("v_and_b32", V(V_L2), 31, lane))
        if self.stamps:
            e(I("s_lshl_b32", S_T[0], S_WGID, 2), I("s_add_u32", S_T[0], S_T[0], S_WAVE), I("s_mul_i32", S_T[0], S_T[0], 8 * NSLOT),
              I("s_add_u32", S_DBG.sub(0), S_DBG.sub(0), S_T[0]), I("s_addc_u32", S_DBG.sub(1), S_DBG.sub(1), 0))
            e(self.stamp(6, real=True), self.stamp(8))
            e([I("v_mov_b32", V(V_ST_ACC + k), 0) for k in range(3)], I("v_mov_b32", V(V_ST_LAST), 0))
        # ---- row sums on the matrix pipe (v_mfma_f32_16x16x128: B operand = the lane's 32 packed P, read as k range g = lane >> 4 of
        #      column lane & 15; output register 0 of lane (g, n) is row 4 g).  Query i = lane & 31 lives in k ranges g with
        #      (g & 1) == (i >> 4): the 0 / 1 A operand of lane (g', m) -- row m, k range g' -- is all ones iff ((m >> 2) & 1) == (g' & 1)
        one4 = 0x38383838 if self.dtype == "e4m3" else 0x3C3C3C3C
        e(comment("row-sum MFMA operand, accumulators, rescale factors"),
          I("v_bfe_u32", t0, lane, 2, 1), I("v_bfe_u32", t1, lane, 4, 1), I("v_cmp_eq_u32", VCC, t0, t1), I("v_mov_b32", t2, one4))
        e([I("v_cndmask_b32", V(V_ONES + k), 0, t2, VCC) for k in range(8)])
        e([I("v_mov_b32", V(V_LACC[qb] + k), 0) for qb in range(2) for k in range(4)])
        e([I("v_mov_b32", V(V_CO[qb]), 1.0) for qb in range(2)])
        if self.scaled:
            e([I("v_mov_b32", V(r), 127) for r in V_SCL + V_SCP + (V_S127,)], [I("v_mov_b32", V(r), 0) for r in V_B],
              [I("v_mov_b32", V(r), 1.0) for r in V_CO2])
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
            # packed P register p of a triangle group holds, in byte b, the score of key b + 8 p + 4 h of the group's 32 against
            # query i: kept iff key <= i
            for p_ in range(4):
                for b in range(4):
                    e(I("v_cmp_ge_i32", VCC, V(V_IMH), 8 * p_ + b), I("v_mov_b32", t2, 0xFF << (8 * b)))
                    if b == 0:
                        e(I("v_cndmask_b32", V(V_PM[p_]), 0, t2, VCC))
                    else:
                        e(I("v_cndmask_b32", t1, 0, t2, VCC), I("v_or_b32", V(V_PM[p_]), V(V_PM[p_]), t1))

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
        """the staged Q rows -> a[128:159] (fragment (qb, ks): rows 32 qb + i, chunks 4 ks + h and 4 ks + 2 + h, as a K row read)"""
        out = []
        for qb in range(2):
            for ks in range(2):
                for u in range(2):
                    out.append(I("ds_read_b128", A_Q(qb, ks).sub(4 * u, 4), V(V_QR[2 * ks + u]), offset=4096 * qb, tag=f"qread qb{qb} ks{ks}"))
        return out

    # ------------------------------------------------------------------ the two phases
    def qk_mfmas(self, Y, cinit=None, qbs=(0, 1)):
        """S^T(next) chains g = 2 qb + kb into score buffer Y: 8 MFMAs of 64 cycles in a list of 32 SLOTS (a64's phase-A time line):
        MFMA 4 qb + 2 ks + kb stands in slot 4 (4 qb + 2 ks + kb), the other slots are None -- emit_phase hands their fillers to
        the MFMA in front of them, in order"""
        assert cinit is None
        out = [None] * 32
        for qb in range(2):
            for ks in range(2):
                for kb in range(2):
                    d = V(Y + 16 * (2 * qb + kb), 16)
                    m = I(self.mfma, d, A_K(kb, ks), A_Q(qb, ks), d if ks else 0, tag=f"qk g{2 * qb + kb} ks{ks}", **self.fmt)
                    out[4 * (4 * qb + 2 * ks + kb)] = m if qb in qbs else None
        return out

    def v_reads(self, buf):
        """16 transposed reads of the V tile in VB[buf]: fragment db, register pair p (keys 32 (p >> 2) + 8 (p & 3) + 4 h + 0..3 and
        the same 8 further on)"""
        out = []
        for db in range(4):
            f = V_F(db)
            for p in (0, 2, 4, 6):
                imm = VB[buf] + 128 * (32 * (p >> 2) + 8 * (p & 3))
                out.append(I("ds_read_b64_tr_b8", f.sub(p, 2), V(V_VR[db]), offset=imm, tag=f"vread db{db} p{p}"))
        return out

    def k_reads(self, buf):
        out = []
        for kb in range(2):
            for ks in range(2):
                for u in range(2):
                    out.append(I("ds_read_b128", A_K(kb, ks).sub(4 * u, 4), V(V_KR[2 * ks + u]), offset=KB[buf] + 4096 * kb, tag=f"kread kb{kb} ks{ks}"))
        return out

    # ------------------------------------------------------------------ the softmax of one tile as a list of placed operations

    def tile_op(self, Sb, kind, payload, init, lazy=None):
        """the instructions of one placed operation, for the tile whose scores live in score buffer Sb.
        lazy = (jd, cond): the tile is diagonal tile jd of its job (if cond holds) and masked lazily (mask_lazy)"""
        if kind in ("ms", "mr", "pm"):
            return self.mask_lazy(Sb, kind, payload, lazy)
        if kind == "mx":
            g, j = payload
            qb, kb = g >> 1, g & 1
            mx = V(V_MX[qb][kb])
            y = lambda r: V(Sb + 16 * g + r)
            if j == 0:
                return [I("v_max3_f32", mx, y(0), y(1), y(2), tag=f"max g{g}")]
            if j == 7:
                return [I("v_max_f32", mx, mx, y(15), tag=f"max g{g}")]
            return [I("v_max3_f32", mx, mx, y(2 * j + 1), y(2 * j + 2), tag=f"max g{g}")]
        if kind == "dec":
            qb, part = payload
            a, b = V(V_MX[qb][0]), V(V_MX[qb][1])
            d = V(V_T[qb])
            # A row's 64 scores of a tile sit in two lanes (h = 0, 1).  Whether the running maximum must move is decided on the
            # lanes' PARTIAL maxima: some lane exceeds the threshold exactly when the row's maximum does -- so the exchange with
            # lane ^ 32 (move, swap, max: three operations per query block and tile) happens only where the complete maximum is
            # used: in a job's first tile (it sets m) and at the head of the rare firing path.  "full_max": the exchange in
            # every tile, as until the end of round 2 (A/B variant)
            full = init or "full_max" in self.abl
            if part == 0:
                return [I("v_max_f32", a, a, b)] + ([I("v_mov_b32", b, a)] if full else [])
            if part == 1:
                return [I("v_permlane32_swap_b32", a, b)] if full else []
            if part == 2:
                if init and self.scaled:    # (an integer reference: every later m is m_O plus an integer, every factor an exact power of two)
                    return [I("v_max_f32", a, a, b), I("v_mul_f32", V(V_MC[qb]), S_C, a), I("v_ceil_f32", V(V_MC[qb]), V(V_MC[qb])),
                            I("v_sub_f32", V(V_B[qb]), 127.0, V(V_MC[qb]))]
                if init:
                    return [I("v_max_f32", a, a, b), I("v_mul_f32", V(V_MC[qb]), S_C, a)]
                return ([I("v_max_f32", a, a, b)] if full else []) + [I("v_fma_f32", d, a, S_C, -V(V_MC[qb]))]
            if init:
                return []
            if part == 3:
                return [I("v_cmp_gt_f32", S_FIRE[qb], d, S_THR)]
            if "fire_nobranch" in self.abl:       # (timing-only: the compare without its branch)
                return []
            l_fire, l_back = self.lab("fire"), self.lab("fire_back")
            # rare: raise this query block's running maximum now (every s' = s * c - m of the PREVIOUS tile has been formed:
            # plan order), remember the factor; O and the row sums are scaled at the end of the coming phase B
            t2, t3 = V(V_T[2 + 2 * qb]), V(V_T[3 + 2 * qb])
            exact = self.fire_exact(Sb, qb, lazy) if lazy is not None else []
            swap = [] if "full_max" in self.abl else [I("v_mov_b32", b, a), I("v_permlane32_swap_b32", a, b), I("v_max_f32", a, a, b)]
            if self.scaled:
                # m := max(m, ceil(c * max)) -- an integer step; the row sums (relative to m) take the exact factor 2^(m_old - m) at
                # the end of this phase B, where the new scale byte 127 + (m - m_O) becomes the P operands' (this phase's P.V still
                # runs on the tile that was rounded against the old m).  Guard: m - m_O > KMAX -> O is re-based to m as well
                l_guard, l_gback = self.lab("guard"), self.lab("guard_back")
                if exact:    # (a lazily masked diagonal tile: the partial maxima ran over hidden keys too -- with the exact maximum in
                    #           hand, leave unless a row really passes the threshold, as the oracle's deferred mode decides)
                    swap = swap + [I("v_fma_f32", t3, a, S_C, -V(V_MC[qb])), I("v_cmp_lt_f32", VCC, S_THR, t3), I("s_nop", 3),
                                   I("s_cbranch_vccz", Label(l_back))]
                self.ool.append([label(l_fire)] + exact + swap +
                                [I("v_mul_f32", t2, S_C, a), I("v_ceil_f32", t2, t2), I("v_max_f32", t2, t2, V(V_MC[qb])),
                                 I("v_sub_f32", t3, V(V_MC[qb]), t2), I("v_mov_b32", V(V_MC[qb]), t2), I("v_exp_f32", V(V_CO[qb]), t3),
                                 I("v_add_f32", t3, t2, V(V_B[qb])), I("v_cvt_u32_f32", V(V_SCP[qb]), t3),
                                 I("v_cmp_lt_f32", VCC, 127.0 + KMAX, t3), I("s_or_b32", S_FLAG, S_FLAG, 1 << qb),
                                 I("s_cbranch_vccnz", Label(l_guard)), label(l_gback), I("s_branch", Label(l_back)),
                                 label(l_guard), I("v_sub_f32", t3, 127.0, t3), I("v_exp_f32", V(V_CO2[qb]), t3),
                                 I("v_sub_f32", V(V_B[qb]), 127.0, t2), I("v_mov_b32", V(V_SCP[qb]), 127),
                                 I("s_or_b32", S_FLAG, S_FLAG, 4 << qb), I("s_branch", Label(l_gback))])
                return [I("s_cmp_lg_u64", S_FIRE[qb], 0), I("s_cbranch_scc1", Label(l_fire)), label(l_back)]
            self.ool.append([label(l_fire)] + exact + swap + [I("v_mul_f32", t2, S_C, a), I("v_max_f32", t2, t2, V(V_MC[qb])),
                             I("v_sub_f32", t3, V(V_MC[qb]), t2), I("v_mov_b32", V(V_MC[qb]), t2), I("v_exp_f32", V(V_CO[qb]), t3),
                             I("s_or_b32", S_FLAG, S_FLAG, 1 << qb), I("s_branch", Label(l_back))])
            return [I("s_cmp_lg_u64", S_FIRE[qb], 0), I("s_cbranch_scc1", Label(l_fire)), label(l_back)]
        if kind == "f":
            e = payload
            y = V(Sb + e)
            return [I("v_fma_f32", y, y, S_C, -V(V_MC[e >> 5]), tag=f"fma {e}")]
        if kind == "e":
            y = V(Sb + payload)
            return [I("v_exp_f32", y, y, tag=f"exp {payload}")]
        if kind == "cv":
            g, j = payload
            # two scores -> two fp8 in the low (j even) / high half of packed register 4 kb + (j >> 1) of the query block: k slots
            # 16 kb + 2 j, + 1 of the B operand P^T(qb).  In place: the register written holds scores of this block that are packed
            # already (group kb = 1 writes into registers 4..7 of group kb = 0, whose pack ran first: tile_plan's order)
            qb, kb = g >> 1, g & 1
            return [I(self.cvt, V(Sb + 32 * qb + 4 * kb + (j >> 1)), V(Sb + 16 * g + 2 * j), V(Sb + 16 * g + 2 * j + 1),
                      op_sel=(0, 0, j & 1), tag=f"cvt g{g} {j}")]
        raise KeyError(kind)

    # ------------------------------------------------------------------ causal masks

    def mask_lazy(self, Sb, kind, payload, lazy):
        """Diagonal tiles other than a job's first are not masked before the softmax: the row maxima are taken over all 64 keys
        (a masked key can only RAISE a maximum: harmless unless it fires the deferred-maximum rescale, and that path --
        fire_exact -- masks the scores exactly and takes the maxima again), and
          'pm'  the wave on the diagonal clears the masked entries of the PACKED P (24 instructions out of line instead of 80
                on the fp32 scores: 8 AND masks per triangle group from the set-up, 8 zero moves for the hidden group);
          'ms'  waves below the diagonal (the whole tile is hidden from them) swap +inf in for the running maximum of the
                query block, so that every exp2(s c - m) is 0 and nothing fires;  'mr' puts the maximum back.
        Both are in line, wave-uniform selects instead of branches (a taken branch costs ~25 cycles at one wave per SIMD)."""
        jd, cond = lazy
        if self.split:
            # every wave of this body sits on the diagonal of tile jd (tile_fill adds 'pm' only there): the even wave has
            # pattern D0 on query block qa = jd >> 1 (key block 0: triangle, key block 1: hidden), the odd one D1 (key block 0
            # visible, key block 1: triangle).  D0 in line, D1 out of line (a taken branch costs what eight VALU operations do)
            assert kind == "pm"
            qa = jd >> 1
            # (fp8: the packed P of score group (qa, kb) is the four registers Sb + 32 qa + 4 kb .. + 3, four keys each)
            p0, p1 = Sb + 32 * qa, Sb + 32 * qa + 4
            l_d1, l_back, l_skip = self.lab("pmask_d1"), self.lab("pmask_back"), self.lab("pmask_skip")
            self.ool.append([label(l_d1)] + [I("v_and_b32", V(p1 + j), V(p1 + j), V(V_PM[j])) for j in range(4)] +
                            [I("s_branch", Label(l_back))])
            head = [I("s_cmp_eq_u32", cond[0], cond[1]), I("s_cbranch_scc0", Label(l_skip))] if cond is not None else []
            return head + [I("s_bitcmp1_b32", S_WAVE, 0), I("s_cbranch_scc1", Label(l_d1))] + \
                [I("v_and_b32", V(p0 + j), V(p0 + j), V(V_PM[j])) for j in range(4)] + \
                [I("v_mov_b32", V(p1 + j), 0) for j in range(4)] + [label(l_back)] + ([label(l_skip)] if cond is not None else [])
        if kind == "pm":
            l_pm, l_back = self.lab("pmask"), self.lab("pmask_back")
            blk = [label(l_pm)]
            if cond is not None:
                blk += [I("s_cmp_eq_u32", cond[0], cond[1]), I("s_cbranch_scc0", Label(l_back))]
            for g in (0, 3):
                blk += [I("v_and_b32", V(Sb + 16 * g + j), V(Sb + 16 * g + j), V(V_PM[j])) for j in range(8)]
            blk += [I("v_mov_b32", V(Sb + 16 + j), 0) for j in range(8)]
            self.ool.append(blk + [I("s_branch", Label(l_back))])
            return [I("s_cmp_eq_u32", S_WAVE, jd), I("s_cbranch_scc1", Label(l_pm)), label(l_back)]
        if jd == 0:
            return []      # no wave lies below diagonal tile 0
        assert cond is None
        sel = [I("s_cmp_ge_u32", S_WAVE, jd), I("s_cselect_b64", VCC, -1, 0)]   # VCC: the tile is (partly) visible to this wave
        if kind == "ms":
            qb = payload
            return sel + [I("v_mov_b32", V(V_MSV[qb]), V(V_MC[qb])), I("v_cndmask_b32", V(V_MC[qb]), -NINF, V(V_MC[qb]), VCC)]
        return sel + [I("v_cndmask_b32", V(V_MC[qb]), V(V_MSV[qb]), V(V_MC[qb]), VCC) for qb in range(2)]

    # ------------------------------------------------------------------ the two phases
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
        length = [64.0 if "32x32x64" in m.op else 32.0 for _, m in kept]
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
        """O^T(qb, db) += V^T(db) . P^T(qb): 8 MFMAs of 64 cycles over all 64 keys, and the row sums of the two P operands
        (v_mfma_f32_16x16x128_f8f6f4 against the 0 / 1 operand: register 0 of V_LACC[qb] is the lane's own 64-key sum), in a list of
        a64's 40 phase-B slots with an MFMA in every fourth: four products, the row sum of query block 0, four products, the row sum
        of query block 1 -- emit_phase hands each the fillers of the four slots it stands for"""
        out = [None] * 40
        seq = []
        for db in range(4):
            for qb in range(2):
                if self.scaled:
                    seq.append(I("v_mfma_scale_f32_32x32x64_f8f6f4", A_O(qb, db), V_F(db), P_OP(X, qb), A_O(qb, db), V(V_S127), V(V_SCL[qb]),
                                 op_sel_hi=(0, 0, 0), tag=f"pv db{db} qb{qb}", **self.fmt) if qb in qbs else None)
                    continue
                seq.append(I(self.mfma, A_O(qb, db), V_F(db), P_OP(X, qb), A_O(qb, db), tag=f"pv db{db} qb{qb}", **self.fmt) if qb in qbs else None)
            if db & 1:
                qb = db >> 1
                seq.append(I("v_mfma_f32_16x16x128_f8f6f4", V(V_LACC[qb], 4), V(V_ONES, 8), P_OP(X, qb), V(V_LACC[qb], 4),
                             tag=f"rowsum qb{qb}", **self.fmt) if qb in qbs and "no_rowsum" not in self.abl else None)
        for k, m in enumerate(seq):
            out[4 * k] = m
        return out

    def rescale(self, qb, tmp, co):
        if not self.scaled:
            return super().rescale(qb, tmp, co)
        # the row sums take 2^(m_old - m), the new scale byte takes over; O only on the guard path (bit 2 + qb)
        l_skip, l_noo = self.lab("rescale_skip"), self.lab("rescale_no_o")
        blk = [I("s_bitcmp1_b32", S_FLAG, qb), I("s_cbranch_scc0", Label(l_skip)),
               I("v_mov_b32", co.sub(0), V(V_CO[qb])), I("v_mov_b32", V(V_SCL[qb]), V(V_SCP[qb]))]
        blk += [I("v_pk_mul_f32", V(V_LACC[qb] + k, 2), V(V_LACC[qb] + k, 2), co, op_sel_hi=(1, 0)) for k in (0, 2)]
        blk += [I("v_mov_b32", V(V_CO[qb]), 1.0), I("s_bitcmp1_b32", S_FLAG, 2 + qb), I("s_cbranch_scc0", Label(l_noo)),
                I("v_mov_b32", co.sub(0), V(V_CO2[qb]))]
        for base in range(0, 64, 8):
            regs = [A(qb * 64 + base + k) for k in range(8)]
            blk += [I("v_accvgpr_read_b32", tmp[k], regs[k]) for k in range(8)]
            blk += [I("v_pk_mul_f32", V(tmp[k].idx, 2), V(tmp[k].idx, 2), co, op_sel_hi=(1, 0)) for k in range(0, 8, 2)]
            blk += [I("v_accvgpr_write_b32", regs[k], tmp[k]) for k in range(8)]
        return blk + [label(l_noo), label(l_skip)]

    # ------------------------------------------------------------------ epilogue of the current job

    def k_epilogue(self):
        """1 / l (one Newton step), L = m + log2 l, O^T -> fp8 rows through the wave's LDS slice -> 16-byte row stores, O^T := 0.
        A query block's 32 rows of 128 bytes leave in four stores of eight rows; the stores of the first block are sprinkled through
        the arithmetic of the second, those of the second run under the MFMAs that zero O."""
        e = self.e
        t = [V(x) for x in V_T]
        e(comment("epilogue: l, 1/l, L; O^T -> rows through the wave's LDS slice -> global; O^T := 0"))
        # (the O and L descriptors of this job were formed in the seam's last phase B: epilogue_descs)
        e(I("s_nop", 15), I("s_nop", 7))  # last P.V MFMAs (16 passes) -> accumulator reads
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
            e(I("v_fma_f32", inv[qb], l[qb], inv[qb], inv[qb]), I(self.cvt, m2[qb], m2[qb], m2[qb]))     # (the low byte: L in fp8)
        if self.scaled:   # O is relative to m_O, l to m: O / (l 2^(m - m_O)); the next job starts at scale 2^0
            for qb in range(2):
                e(I("v_sub_u32", V(V_SCP[qb]), 127, V(V_SCL[qb])))
            for qb in range(2):
                e(I("v_ldexp_f32", inv[qb], inv[qb], V(V_SCP[qb])), I("v_mov_b32", V(V_SCL[qb]), 127))
        e(self.stamp_async(0))
        # O: 4 accumulators (four consecutive columns of one query) -> one register of four fp8 -> ds_write_b32 at (row i, byte
        # 32 db + 8 g4 + 4 h); one query block at a time.  (S[0] already holds the next job's first scores and v[128:159] its K(1):
        # rows and temporaries are score buffer 1, whose P was consumed by the job's last P.V.)  A batch = one 32-column block.
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
            for db in range(4):
                tm = tset[db & 1]
                src = A_O(qb, db)
                rd = [I("v_accvgpr_read_b32", tm[k], src.sub(k)) for k in range(16)]
                mu = [I("v_pk_mul_f32", V(tm[k].idx, 2), V(tm[k].idx, 2), V(inv[qb].idx, 2), op_sel_hi=(1, 0)) for k in range(0, 16, 2)]
                cv = []
                for g4 in range(4):
                    cv += [I(self.cvt, tm[4 * g4], tm[4 * g4], tm[4 * g4 + 1]),
                           I(self.cvt, tm[4 * g4], tm[4 * g4 + 2], tm[4 * g4 + 3], op_sel=(0, 0, 1))]
                wr = [I("ds_write_b32", V(V_EW), tm[4 * g4], offset=32 * db + 8 * g4) for g4 in range(4)]
                stages.append((rd, mu, cv, wr))
            # software pipeline over the four batches (two register sets): batch b + 1 is read while batch b is scaled, ...
            head = stages[0][0] + weave(stages[0][1], stages[1][0]) + stages[0][2] + stages[0][3]
            tail = weave(stages[1][1], stages[2][0]) + stages[1][2] + stages[1][3] + weave(stages[2][1], stages[3][0]) + \
                stages[2][2] + stages[2][3] + stages[3][1] + stages[3][2] + stages[3][3]
            e(head)
            if qb == 1:
                e(self.stamp_async(2))
                # the first block's rows have been on their way back from LDS since before this block started (four of this
                # block's writes are younger): wait for them once, then one row store every ~50 instructions
                e(waitcnt(lgkmcnt=4))
                e(sprinkle(tail, row_stores(0)))
            else:
                e(tail)
            e(read_back())
            e(self.stamp_async(1 if qb == 0 else 3))
        # O^T := 0 and row sums := 0 for the next job; O on the matrix pipe: eight bf16 32x32x16 MFMAs on zero operands clear 16
        # accumulators each (instead of 128 v_accvgpr_write)
        z = V(V_Z, 4)
        e([I("v_mov_b32", V(V_LACC[qb] + k), 0) for qb in range(2) for k in range(4)])
        e([I("v_mov_b32", z.sub(k), 0) for k in range(4)], I("s_nop", 1))
        zero = [I("v_mfma_f32_32x32x16_bf16", A_O(qb, db), z, z, 0) for qb in range(2) for db in range(4)]
        # (offset / stride registers the job bookkeeping below leaves alone: k_promote and k_advance use S_T[0..4], [6], [7])
        st1 = row_stores(1, off=S_T[5], stride=S_T[6], restride=True)
        e(zero[0], zero[1])
        e(self.stamp_async(4))
        e(waitcnt(lgkmcnt=0))
        e(self.stamp_async_flush((13, 14, 15, 20, 21)))   # (before the scalar code below: it uses the stamp registers)
        # L store (lanes 0..31), one byte per row: in front of the job bookkeeping (it needs this job's row numbers and S_T)
        e(I("s_lshr_b64", EXEC, EXEC, 32))
        for qb in range(2):
            pre, st = self.buf_op("buffer_store_byte", m2[qb], V(V_L2), S_NVRS, S_QROW[qb])
            e(pre, st)
        e(I("s_mov_b64", EXEC, -1))
        for k in range(4):
            e(st1[k])
            e(zero[2 + k])
            if k == 0:
                # Job bookkeeping in the shadow of the row stores: the next job becomes the current one and the job after it is
                # decoded.  S_FINAL still says "this job is the workgroup's last" for the branch behind the epilogue: it is put
                # aside in S_FLAG (idle between steps)
                l_last = self.lab("epi_last")
                e(I("s_mov_b32", S_FLAG, S_FINAL), I("s_cmp_lg_u32", S_FINAL, 0), I("s_cbranch_scc1", Label(l_last)))
                self.k_promote()
                self.k_advance(vt=(tset[0][4], tset[0][5]))
                e(label(l_last))
        e(zero[6], zero[7])


def product_gens():
    """the kernels of this generator that ship in libfa2_hip.so's code object (built by fa2_a64_gen.main)"""
    out = []
    for dtype in ("e4m3", "e5m2"):
        for causal in (False, True):
            for ragged in (False, True):
                g = Gen(dtype, causal, ragged=ragged)
                g.build()
                out.append(g)
    return out


def variant_gens():
    """experiments build: the kernel without the block scale (a rescale of O whenever the running maximum moves), and ring depths,
    for A/B runs"""
    out = [Gen("e4m3", False, scaled=False), Gen("e4m3", False, name="fa2_fwd_a8_e4m3_n_ring4", ring=(4, 4, 3)),
           Gen("e4m3", False, name="fa2_fwd_a8_e4m3_n_ring2", ring=(2, 3, 2))]
    for g in out:
        g.build()
    return out
