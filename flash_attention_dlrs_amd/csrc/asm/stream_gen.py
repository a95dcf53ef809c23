"""The job-stream machinery shared by the four generated kernel families: fa2_a64_gen (f16 / bf16, d = 128), fa2_a16_gen (the
same on v_mfma_f32_16x16x32), fa2_a64d_gen (d = 64) and fa2_a8_gen (fp8).

All four have one structure (fa2_a64_gen's docstring): a persistent grid of 4-wave workgroups, 64-key K / V tiles in LDS rings
filled by LDS-DMA, two phases per tile with the softmax spread over the MFMA gaps, a continuous tile stream across jobs.  What
they share lives here: the SGPR map and the kernel-argument block, the score buffers, the job decode, the DMA bookkeeping, the
softmax plan of a tile, the phases, the seam and the whole-kernel driver, the stamps, the text and the metadata.

A family module keeps its own VGPR / AGPR map and LDS geometry as module globals, and the values differ between families.  A
method here must therefore never read a family's register or size as a global of this module: it reads it through the instance
(StreamGen's docstring lists them), and where the families' streams differ in a constant the constant is a named class
attribute.  Where they differ in structure the family overrides the method.  No method here tests which family it serves.
"""
from __future__ import annotations

from .isa import A, I, Inst, Label, Reg, S, V, VCC, comment, label, waitcnt

SBUF = (0, 64)            # two score buffers of 64 registers: group g = 2*qb + kb at +16 g

# SGPRs.  s4..s47 hold the kernel arguments (loaded once).
S_KARG = S(0, 2)
S_WGID = S(2)
S_FINAL = S(75)
S_Q, S_K, S_V, S_O, S_L = S(4, 2), S(6, 2), S(8, 2), S(10, 2), S(12, 2)
S_QSB, S_QSH, S_KSB, S_KSH, S_VSB, S_VSH, S_OSB, S_OSH, S_LSB, S_LSH = (S(14 + 2 * k, 2) for k in range(10))
S_QSN, S_KSN, S_VSN, S_OSN = S(34), S(35), S(36), S(37)
S_N, S_H, S_NQ, S_TOTAL = S(38), S(39), S(40), S(41)
S_C, S_THR, S_NUNIT, S_G = S(42), S(43), S(44), S(45)
S_NBH, S_NWG = S(46), S(47)
S_KRS, S_VRS, S_NVRS, S_SQ = S(48, 4), S(52, 4), S(56, 4), S(60, 4)   # K / V descriptors, the next job's V, a scratch one
S_NB, S_NHH, S_NQI, S_NNT = S(64), S(65), S(66), S(67)                # the next job
S_JOB, S_WAVE = S(68), S(69)
S_KDMA, S_VDMA = S(70), S(71)    # source offset of the next K / V tile to stream (the wave's row base included)
S_K32, S_V32 = S(72), S(74)      # 32 rows of K / V in bytes
S_K64, S_V64 = S(76), S(77)
S_LDSW = S(78)                   # 2048 * wave: the wave's piece offset inside a ring buffer
S_LOOP, S_FLAG = S(79), S(80)
S_QI, S_B, S_HH, S_UNIT, S_PASS, S_NT = S(81), S(83), S(84), S(85), S(86), S(87)   # the current job
S_T = tuple(S(88 + k) for k in range(8))  # temporaries s88..s95 (S_T[0] even: usable as a 64-bit pair)
S_QROW = (S(96), S(97))          # first row of the wave's query block qb (current job)
S_DBG = S(98, 2)
S_KW, S_VW = S(100), S(101)      # 8 * wave * row stride: the wave's row base inside a tile
S_KT0 = S(86)                    # (= S_PASS, causal only) non-causal ragged: real keys in the job's last 256 = N - 256 (nq - 1)
S_LG = S(73)                     # decode shifts: lgH | lgG << 8 | lg(G * nunit) << 16 | pow2-mode << 24
S_FIRE = (S(0, 2), S(2, 2))      # per query block: lanes whose row maximum passed the deferral threshold (s0..s3 are free after the set-up)
S_X2 = S(82)

KARG_SIZE = 192
NSLOT = 24


def module_text(gens):
    head = ['.amdgcn_target "amdgcn-amd-amdhsa--gfx950"', ".amdhsa_code_object_version 6", ".text", ""]
    body = "\n".join(head) + "\n".join(g.text() for g in gens)
    md = ["", ".amdgpu_metadata", "---", "amdhsa.kernels:"] + [g.metadata() for g in gens] + [
        "amdhsa.target: amdgcn-amd-amdhsa--gfx950", "amdhsa.version:", "  - 1", "  - 2", "...", ".end_amdgpu_metadata", ""]
    return body + "\n".join(md)


class StreamGen:
    """Base of every family's Gen.  The subclass supplies, as class attributes:

    its registers and LDS size (its module's values): V_T (temporaries), V_ST_LAST / V_ST_ACC (stamps), V_MC / V_MX / V_CO /
    V_MSV (running maxima, max chains, rescale factors, the finished job's maxima), V_LACC (row sums), V_LANE, V_IMH / V_PM /
    NINF (causal masks), S_NDESC / S_DESC (the downward walk; not for a family that does not walk down), LDS_TOTAL;

    the constants in which the streams differ:
      FAMILY        kernel-name stem: fa2_fwd_<FAMILY>_<dtype>_<c|n>[r]
      MFMA, CVT     the matrix instruction ("{dtype}" filled in); the P pack per I/O dtype (its keys: the dtypes taken)
      DMA_PIECES    LDS-DMA pieces per K (or V) tile and wave
      K_READS       K row reads per phase B;  V_READS: V transposed reads per phase A
      DMA_GAPS      phase-B gaps of a step's own DMA pieces (V pieces, then K)
      QS_GAPS       the seam's Q staging: (step 0's own-piece gaps, its late Q pieces' gaps, step 1's in-phase and late Q
                    pieces' gaps, the further pieces step 1's barrier wait leaves in flight)
      O_AGPRS       O^T accumulators of both query blocks (a[0:O_AGPRS])
      ROW_BYTES     bytes of a K / V row: ragged descriptors cover (N - 1) * stride + ROW_BYTES
      L_SN          make_desc's int row size of the L descriptor
      BRANCH_NEED   check.check_branch_targets' need (None: its default)
      WALK_DOWN     causal light jobs may walk their tiles downwards (stream_start)

    and overrides what differs in structure: the MFMA emitters (qk_mfmas, pv_mfmas, emit_phase), the operand reads (q_reads,
    k_reads, v_reads), q_stage, dma_piece, k_setup, k_epilogue, tile_op, and where a family's masking or stamps differ, those."""

    def __init__(self, dtype="bf16", causal=False, name=None, stamps=False, abl=(), ring=(2, 3, 2), vread_double=4, ragged=False,
                 caps=(5, 24), split=True):
        assert dtype in self.CVT, f"{self.FAMILY}: {' / '.join(self.CVT)}"
        self.dtype = dtype
        self.causal = causal
        self.name = name or f"fa2_fwd_{self.FAMILY}_{dtype}_{'c' if causal else 'n'}{'r' if ragged else ''}"
        self.atmp = 0          # (ragged) which of the two address temporaries the next buffer operation takes
        self.atmp_regs = (self.V_T[8], self.V_T[9])
        self.prog: list[Inst] = []
        self.uid = 0
        self.mfma = self.MFMA.format(dtype=dtype)
        self.cvt = self.CVT[dtype]
        self.ool: list[list[Inst]] = []  # out-of-line blocks (rare paths), appended after the main body
        self.caps = caps       # fillers / issue cycles a gap behind a 32x32x16 MFMA may carry in the softmax plan
        # causal row map "split": wave w owns the 32-row blocks w (qb 0) and w + 4 (qb 1) of the job's 256 rows instead of
        # 2 w and 2 w + 1.  Diagonal tile j (key blocks 2 j, 2 j + 1) is then hidden from query block 0 of EVERY wave for
        # j >= 2 and fully visible to query block 1 for j < 2: the job's last steps run on one query block (half the MFMAs)
        # for all four waves instead of on both for a shrinking set of waves -- see build()
        self.split = bool(split) and causal
        self.cls = None        # split seam bodies: "low" (waves 0, 1) / "high" (waves 2, 3) while their code is generated
        self.ragged = ragged   # N is not a multiple of 256: range-checked descriptors, every offset in the VGPR operand, masked key tail
        assert not (ragged and stamps), "the ragged kernels use the stamps' temporaries as address registers"
        self.vread_double = vread_double   # phase-A gaps that carry two V transposed reads (the last read sits in gap 31 - this)
        self.abl = set(abl)    # timing-only ablations of the steady loop (diagnostic builds; results wrong by construction)
        self.R, self.dk, self.dv = ring   # ring depth; K(t + dk) and V(t + dv) are streamed in phase B(t): dk <= R + 1, dv <= R
        assert 3 <= self.dk <= min(self.R + 1, 4) and 2 <= self.dv <= self.R and 4 % self.R == 0
        self.vm = 2 * self.DMA_PIECES * min(self.dk - 3, self.dv - 2)  # DMA pieces that may stay in flight across the mid-step barrier
        self._cache = {}
        self.stamps = stamps   # diagnostic build: s_memtime stamps of the job timeline go to the debug buffer
        # Causal, the LIGHT job of a unit walks DOWNWARDS (the host sets bit 25 of the decode word): a unit is the heavy job
        # (query block nq - 1 - u, key tiles upwards) followed by the light job (query block u) of the same head.  All units of a head
        # start their heavy job at tile 0 together and leave it behind their diagonal, after 4 (nq - u) steps; a light job that walks
        # its non-diagonal tiles 4 u - 1 .. 0 downwards is at tile 4 nq - 1 - s at step s WHATEVER its u: the light jobs of a head
        # form one stream in lockstep (each tile fetched once for all of them) that meets the tiles in the reverse of the order
        # the heavy jobs left them in the XCD's L2 -- instead of every light job starting again at tile 0 at a time of its own
        # (K / V came from beyond L2 2.0 times; profiles/r02/c3_a64_rocprof.json).  The diagonal tiles stay a job's last four,
        # and the order is a function of (query block, nq) alone: a head's result does not depend on the launch it is part of.
        self.down = self.WALK_DOWN and causal and not stamps and not ragged

    def e(self, *insts):
        for x in insts:
            if isinstance(x, (list, tuple)):
                self.e(*x)
            else:
                self.prog.append(x)

    def lab(self, stem):
        self.uid += 1
        return f".L{self.name}_{stem}_{self.uid}"

    def stamp(self, slot, real=False):
        """diagnostic builds only: dbg[(wg * 4 + wave) * NSLOT + slot] = s_memtime (or s_memrealtime)"""
        if not self.stamps:
            return []
        t = S(S_T[0].idx, 2)
        v = V(self.V_T[8], 2)
        return [I("s_memrealtime" if real else "s_memtime", t), waitcnt(lgkmcnt=0),
                I("v_mov_b32", v.sub(0), t.sub(0)), I("v_mov_b32", v.sub(1), t.sub(1)),
                I("v_mov_b32", V(self.V_T[7]), 0), I("global_store_dwordx2", V(self.V_T[7]), v, S_DBG, offset=8 * slot)]

    ASYNC_PAIRS = (S(90, 2), S(92, 2), S(94, 2), S(0, 2), S(2, 2))   # S_T[2..7], S_FIRE: idle in the epilogue

    def stamp_async(self, k):
        """diagnostic builds only: s_memtime into spare pair k WITHOUT a wait (the epilogue's LDS queue is not drained; its
        counted lgkmcnt waits may be satisfied early by the returning s_memtime: timing-only)"""
        return [I("s_memtime", self.ASYNC_PAIRS[k])] if self.stamps else []

    def stamp_async_flush(self, slots):
        if not self.stamps:
            return []
        out = [waitcnt(lgkmcnt=0), I("v_mov_b32", V(self.V_T[7]), 0)]
        v = V(self.V_T[8], 2)
        for k, slot in enumerate(slots):
            t = self.ASYNC_PAIRS[k]
            out += [I("v_mov_b32", v.sub(0), t.sub(0)), I("v_mov_b32", v.sub(1), t.sub(1)),
                    I("global_store_dwordx2", V(self.V_T[7]), v, S_DBG, offset=8 * slot), I("s_nop", 7)]
        return out

    def stamp_acc(self, k):
        """diagnostic builds only: acc[k] += cycles since the previous stamp_acc (its s_waitcnt drains the LDS queue as well: the
        per-phase shares cost cycles of their own -- the "lite" kernels carry the job-level stamps only)"""
        if not self.stamps or "lite" in self.abl:
            return []
        t = S(S_T[0].idx, 2)
        tmp = V(self.V_T[9])
        acc = [I("v_sub_u32", tmp, t.sub(0), V(self.V_ST_LAST)), I("v_add_u32", V(self.V_ST_ACC + k), V(self.V_ST_ACC + k), tmp)] if k < 3 else []
        return [I("s_memtime", t), waitcnt(lgkmcnt=0)] + acc + [I("v_mov_b32", V(self.V_ST_LAST), t.sub(0))]

    def stamp_job(self, k):
        """lite diagnostic builds: acc[k] += cycles since the previous stamp_job, summed over ALL jobs of the workgroup
        (0 steady loops, 1 seam bodies, 2 epilogues + job bookkeeping, 3 the pipeline fill of the first job)"""
        if not self.stamps or "lite" not in self.abl:
            return []
        t = S(S_T[0].idx, 2)
        tmp = V(self.V_T[9])
        acc = [I("v_sub_u32", tmp, t.sub(0), V(self.V_ST_LAST)), I("v_add_u32", V(self.V_ST_ACC + k), V(self.V_ST_ACC + k), tmp)] if k < 3 else []
        return [I("s_memtime", t), waitcnt(lgkmcnt=0)] + acc + [I("v_mov_b32", V(self.V_ST_LAST), t.sub(0))]

    def stamp_job_flush(self):
        if not self.stamps or "lite" not in self.abl:
            return []
        out = [I("v_mov_b32", V(self.V_T[7]), 0)]
        for k, slot in enumerate((10, 11, 12)):
            out += [I("global_store_dword", V(self.V_T[7]), V(self.V_ST_ACC + k), S_DBG, offset=8 * slot)]
        return out

    def stamp_flush(self):
        if not self.stamps or "lite" in self.abl:
            return []
        out = [I("v_mov_b32", V(self.V_T[7]), 0)]
        for k in range(3):
            out += [I("global_store_dword", V(self.V_T[7]), V(self.V_ST_ACC + k), S_DBG, offset=8 * (10 + k)),
                    I("v_mov_b32", V(self.V_ST_ACC + k), 0)]
        return out

    def udiv(self, q: Reg, r: Reg | None, n: Reg, d: Reg, vt=None):
        """q = n / d, r = n % d for wave-uniform 32-bit values < 2^22 (float reciprocal + one correction each way)"""
        t0, t1 = vt if vt is not None else (V(self.V_T[0]), V(self.V_T[1]))
        st, sr = S_T[6], S_T[7]
        self.e(I("v_cvt_f32_u32", t0, n), I("v_cvt_f32_u32", t1, d), I("s_nop", 0), I("v_rcp_f32", t1, t1), I("s_nop", 1),
               I("v_mul_f32", t0, t0, t1), I("v_cvt_u32_f32", t0, t0), I("s_nop", 1), I("v_readfirstlane_b32", q, t0), I("s_nop", 4),
               I("s_mul_i32", st, q, d), I("s_sub_i32", sr, n, st),
               # r < 0 -> q--, r += d
               I("s_cmp_lt_i32", sr, 0), I("s_cselect_b32", st, 1, 0), I("s_sub_u32", q, q, st),
               I("s_cmp_lt_i32", sr, 0), I("s_cselect_b32", st, d, 0), I("s_add_i32", sr, sr, st),
               # r >= d -> q++, r -= d
               I("s_cmp_ge_i32", sr, d), I("s_cselect_b32", st, 1, 0), I("s_add_u32", q, q, st),
               I("s_cmp_ge_i32", sr, d), I("s_cselect_b32", st, d, 0), I("s_sub_i32", sr, sr, st))
        if r is not None:
            self.e(I("s_mov_b32", r, sr))

    def mad64(self, dst: Reg, idx: Reg, stride: Reg):
        """dst(64) += idx(32, unsigned) * stride(64)"""
        lo, hi = S_T[6], S_T[7]
        return [I("s_mul_i32", lo, idx, stride.sub(0)), I("s_mul_hi_u32", hi, idx, stride.sub(0)),
                I("s_add_u32", dst.sub(0), dst.sub(0), lo), I("s_addc_u32", dst.sub(1), dst.sub(1), hi),
                I("s_mul_i32", lo, idx, stride.sub(1)), I("s_add_u32", dst.sub(1), dst.sub(1), lo)]

    def make_desc(self, rs: Reg, base: Reg, sb: Reg, sh: Reg, b: Reg, hh: Reg, sn=None):
        """raw buffer descriptor of the (b, hh) slice of a tensor: base + b * sb + hh * sh.  N a multiple of 256: the range check
        is not used (soffset is unchecked anyway; every address the kernel forms lies inside the tensor).  Ragged kernels:
        num_records = (N - 1) * sn + ROW_BYTES bytes of rows (sn: the row stride register; an int: bytes per row of L) -- loads of
        rows past N come back as zeros, stores to them are dropped; those kernels keep every offset in the VGPR operand"""
        tmp = S(S_T[0].idx, 2)
        out = ([I("s_mov_b64", tmp, base)] + self.mad64(tmp, b, sb) + self.mad64(tmp, hh, sh) +
               [I("s_mov_b32", rs.sub(0), tmp.sub(0)), I("s_and_b32", rs.sub(1), tmp.sub(1), 0xFFFF), I("s_mov_b32", rs.sub(3), 0x00020000)])
        if not self.ragged:
            return out + [I("s_mov_b32", rs.sub(2), 0x7FFFFFF0)]
        assert sn is not None
        if isinstance(sn, int):
            return out + [I("s_mul_i32", rs.sub(2), S_N, sn)]
        return out + [I("s_sub_u32", S_T[6], S_N, 1), I("s_mul_i32", S_T[6], S_T[6], sn), I("s_add_u32", rs.sub(2), S_T[6], self.ROW_BYTES)]

    def buf_op(self, op, data, voff: Reg, rsrc: Reg, soff, **mods):
        """a buffer operation at byte offset voff (per lane) + soff (scalar).  The scalar operand of the instruction is not
        range-checked: the ragged kernels add it into an address temporary first (two, taken alternately: a set-up may run
        ahead of the previous piece's load by one gap).  Returns (set-up instructions, the memory instruction)"""
        ops = (lambda v, so: (data, v, rsrc, so) if data is not None else (v, rsrc, so))
        if not self.ragged:
            return [], I(op, *ops(voff, soff), offen=1, **mods)
        tmp = V(self.atmp_regs[self.atmp])
        self.atmp ^= 1
        return [I("v_add_u32", tmp, soff, voff)], I(op, *ops(tmp, 0), offen=1, **mods)

    def k_decode_next(self, vt=None):
        e = self.e
        l_else, l_done = self.lab("dec_else"), self.lab("dec_done")
        t = S_T
        bh = S_X2
        l_gen = self.lab("dec_generic")
        e(comment("job index -> (b, h), work unit, query block, tile count of the NEXT job"),
          I("s_bitcmp1_b32", S_LG, 24), I("s_cbranch_scc0", Label(l_gen)))
        # H, G, G * nunit powers of two and B * H a multiple of 8 (the host says so): shifts and masks only
        e(I("s_lshr_b32", t[0], S_JOB, 3),                                   # slot
          I("s_lshr_b32", t[1], S_LG, 16), I("s_and_b32", t[1], t[1], 255),   # lg(G nunit)
          I("s_lshr_b32", t[2], t[0], t[1]),                                  # batch
          I("s_lshl_b32", t[3], 1, t[1]), I("s_sub_u32", t[3], t[3], 1), I("s_and_b32", t[3], t[0], t[3]),   # r
          I("s_lshr_b32", t[1], S_LG, 8), I("s_and_b32", t[1], t[1], 255),    # lg G
          I("s_lshr_b32", S_UNIT, t[3], t[1]),                                # unit = r >> lgG
          I("s_lshl_b32", t[4], 1, t[1]), I("s_sub_u32", t[4], t[4], 1), I("s_and_b32", t[4], t[3], t[4]),   # r % G
          I("s_lshl_b32", t[2], t[2], t[1]), I("s_add_u32", t[2], t[2], t[4]), I("s_lshl_b32", t[2], t[2], 3),
          I("s_and_b32", t[0], S_JOB, 7), I("s_add_u32", bh, t[2], t[0]),
          I("s_and_b32", t[1], S_LG, 255),                                    # lg H
          I("s_lshr_b32", S_NB, bh, t[1]),
          I("s_lshl_b32", t[4], 1, t[1]), I("s_sub_u32", t[4], t[4], 1), I("s_and_b32", S_NHH, bh, t[4]))
        l_qi = self.lab("dec_qi")
        e(I("s_branch", Label(l_qi)), label(l_gen),
          I("s_and_b32", t[0], S_NBH, 7), I("s_cmp_lg_u32", t[0], 0), I("s_cbranch_scc1", Label(l_else)))
        # slot = id >> 3; GN = G * nunit; batch = slot / GN; r = slot % GN; bh = (batch * G + r % G) * 8 + (id & 7); unit = r / G
        e(I("s_lshr_b32", t[0], S_JOB, 3), I("s_mul_i32", t[1], S_G, S_NUNIT))
        self.udiv(t[2], t[3], t[0], t[1], vt)       # batch, r
        self.udiv(S_UNIT, t[4], t[3], S_G, vt)      # unit = r / G, r % G
        e(I("s_mul_i32", t[2], t[2], S_G), I("s_add_u32", t[2], t[2], t[4]), I("s_lshl_b32", t[2], t[2], 3),
          I("s_and_b32", t[0], S_JOB, 7), I("s_add_u32", bh, t[2], t[0]), I("s_branch", Label(l_done)))
        e(label(l_else))
        self.udiv(bh, S_UNIT, S_JOB, S_NUNIT, vt)
        e(label(l_done))
        self.udiv(S_NB, S_NHH, bh, S_H, vt)
        e(label(l_qi))
        if self.causal:
            # unit u, pass 0: qi = nq - 1 - u (heavy), pass 1: qi = u;  tiles = 4 (qi + 1)
            l_p1, l_pd = self.lab("pass1"), self.lab("passd")
            e(I("s_cmp_lg_u32", S_PASS, 0), I("s_cbranch_scc1", Label(l_p1)),
              I("s_sub_u32", S_NQI, S_NQ, 1), I("s_sub_u32", S_NQI, S_NQI, S_UNIT), I("s_branch", Label(l_pd)),
              label(l_p1), I("s_mov_b32", S_NQI, S_UNIT), label(l_pd),
              I("s_add_u32", t[0], S_NQI, 1), I("s_lshl_b32", S_NNT, t[0], 2))
            if self.down:   # the light job of a unit walks downwards (unless it is nothing but its diagonal)
                e(I("s_lshr_b32", t[0], S_LG, 25), I("s_and_b32", t[0], t[0], S_PASS), I("s_and_b32", t[0], t[0], 1),
                  I("s_cmp_lg_u32", S_NQI, 0), I("s_cselect_b32", self.S_NDESC, t[0], 0))
        else:
            e(I("s_mov_b32", S_NQI, S_UNIT), I("s_lshl_b32", S_NNT, S_NQ, 2))      # (4 tiles per 256 rows, N rounded up)

    def k_advance(self, vt=None):
        """S_JOB / S_PASS -> the job after the most recently decoded one, decoded into the next-job registers;
        S_FINAL = 1 if there is none (the next-job registers then repeat the current job).  vt: two VGPR temporaries for the
        divisions of the generic decode (default V_T[0], V_T[1])"""
        e = self.e
        l_fin, l_ok = self.lab("adv_final"), self.lab("adv_ok")
        if self.causal:
            l_adv = self.lab("adv")
            # pass 0 -> pass 1 of the same unit unless the pair is a single tile (nq odd, middle)
            e(I("s_cmp_lg_u32", S_PASS, 0), I("s_cbranch_scc1", Label(l_adv)),
              I("s_sub_u32", S_T[0], S_NQ, 1), I("s_sub_u32", S_T[0], S_T[0], S_UNIT), I("s_cmp_eq_u32", S_T[0], S_UNIT),
              I("s_cbranch_scc1", Label(l_adv)),
              I("s_mov_b32", S_PASS, 1), I("s_branch", Label(l_ok)),
              label(l_adv), I("s_mov_b32", S_PASS, 0), I("s_add_u32", S_JOB, S_JOB, S_NWG))
        else:
            e(I("s_add_u32", S_JOB, S_JOB, S_NWG))
        e(I("s_cmp_ge_u32", S_JOB, S_TOTAL), I("s_cbranch_scc1", Label(l_fin)), label(l_ok))
        self.k_decode_next(vt)
        l_done = self.lab("adv_done")
        e(I("s_branch", Label(l_done)), label(l_fin),
          comment("no further job: the seam streams the current job's first tiles again (results discarded)"),
          I("s_mov_b32", S_FINAL, 1), I("s_mov_b32", S_NB, S_B), I("s_mov_b32", S_NHH, S_HH), I("s_mov_b32", S_NQI, S_QI),
          I("s_mov_b32", S_NNT, S_NT), ([I("s_mov_b32", self.S_NDESC, self.S_DESC)] if self.down else []), label(l_done))

    def k_promote(self):
        """next job -> current job"""
        self.e(([I("s_mov_b32", self.S_DESC, self.S_NDESC)] if self.down else []),
               I("s_mov_b32", S_B, S_NB), I("s_mov_b32", S_HH, S_NHH), I("s_mov_b32", S_QI, S_NQI), I("s_mov_b32", S_NT, S_NNT),
               # query rows of this wave: qrow[qb] = 256 qi + 64 wave + 32 qb  (split row map: 256 qi + 32 wave + 128 qb)
               I("s_lshl_b32", S_T[0], S_QI, 8), I("s_lshl_b32", S_T[1], S_WAVE, 5 if self.split else 6),
               I("s_add_u32", S_QROW[0], S_T[0], S_T[1]),
               I("s_add_u32", S_QROW[1], S_QROW[0], 128 if self.split else 32))

    def stream_start(self, which):
        """causal: start offset and step of the NEXT job's K / V tile stream -- upwards from tile 0, or (S_NDESC) downwards from
        the tile under the diagonal span, 4 qi - 1.  S_K64 / S_V64 hold the signed step of the running stream"""
        dma, w0, s32, step = (S_KDMA, S_KW, S_K32, S_K64) if which == "k" else (S_VDMA, S_VW, S_V32, S_V64)
        if not self.down:
            return [I("s_mov_b32", dma, w0)]
        t0, t1 = S_T[6], S_T[7]     # (the 64-bit multiply's scratch: free between scalar units; S_T[2..4] belong to the Q staging)
        return [I("s_lshl_b32", t0, s32, 1), I("s_lshl_b32", t1, S_NQI, 2), I("s_sub_u32", t1, t1, 1), I("s_mul_i32", t1, t1, t0),
                I("s_cmp_lg_u32", self.S_NDESC, 0), I("s_cselect_b32", t1, t1, 0), I("s_add_u32", dma, w0, t1),
                I("s_sub_u32", t1, 0, t0), I("s_cmp_lg_u32", self.S_NDESC, 0), I("s_cselect_b32", step, t1, t0)]

    def stream_to_diagonal(self, which):
        """causal, the steady loop's last trip: the stream has reached the job's diagonal span -- tiles 4 qi .. 4 qi + 3, upwards
        (for a job that walks upwards this is where it stood anyway)"""
        if not self.down:
            return []
        dma, w0, s32, step = (S_KDMA, S_KW, S_K32, S_K64) if which == "k" else (S_VDMA, S_VW, S_V32, S_V64)
        t0, t1 = S_T[6], S_T[7]
        return [I("s_lshl_b32", t0, s32, 1), I("s_lshl_b32", t1, S_QI, 2), I("s_mul_i32", t1, t1, t0), I("s_add_u32", t1, t1, w0),
                I("s_cmp_eq_u32", S_LOOP, 1), I("s_cselect_b32", dma, t1, dma),
                I("s_cmp_eq_u32", S_LOOP, 1), I("s_cselect_b32", step, t0, step)]

    def dma_tile(self, which, buf):
        out = []
        for j in range(self.DMA_PIECES):
            out += self.dma_piece(which, j, buf)
        out.append(I("s_add_u32", S_KDMA, S_KDMA, S_K64) if which == "k" else I("s_add_u32", S_VDMA, S_VDMA, S_V64))
        return out

    # Time line of a tile, in MFMA gaps (tau): [0, 32) = the phase A that computes its scores (QK^T chains g = 0..3, eight
    # MFMAs each), [32, 32 + NB) = the following phase B (NB = 40 MFMAs: P.V of the previous tile plus its row sums),
    # [32 + NB, 64 + NB) = the next phase A, at whose end P must be packed (its own P.V follows).  In steady state the
    # physical gap (tau mod PERIOD) therefore carries operations of two tiles: a modulo reservation table keeps every gap
    # within what hides beside an MFMA (measured, scripts/probes/mb_run + asm/microbench.py: at most five fillers per gap,
    # issue costs v_exp 8 / three-operand VALU 5 / two-operand 4 summing to <= 24; LDS reads first in their gap).
    NB = 40

    PERIOD = 72

    T_END = 104

    LAZY_TAU = {"ms0": 28, "ms1": 29, "mr": 99, "pm": 100}   # tau of the lazy-masking operations of a diagonal tile (mask_lazy)

    def lazy_tau(self):
        """(the split row map has no 'ms' / 'mr'; its packed-P masking sits behind the last pack of the plan, which ends two gaps
        later there: tile_plan, gap2)"""
        return dict(self.LAZY_TAU, pm=103) if self.split else self.LAZY_TAU

    def tile_plan(self, init=False, lean=False):
        """placement of the per-tile softmax operations: returns [(tau, kind, payload)] sorted by tau.
        kinds: 'mx' (g, j)  'dec' (qb, part)  'f' e  'e' e  'cv' (g, j)"""
        key = "plan"
        if key in self._cache:
            return self._cache[key]
        P = self.PERIOD
        slots = [0.0] * P
        cost = [0.0] * P
        nexp = [0] * P
        cap_s = [float(self.caps[0])] * P
        cap_c = [float(self.caps[1])] * P
        # phase B: the gap behind a 16x16x32 row-sum MFMA is half as long
        for b in self.b_short_gaps():
            cap_s[32 + b], cap_c[32 + b] = 2.0, 8.0
        # pre-reserved: the V transposed reads of phase A; K reads, DMA pieces and their scalar set-up in phase B
        for k in range(self.V_READS):
            slots[self.a_vread_gap(k)] += 1
            cost[self.a_vread_gap(k)] += 2
        for b, n in self.b_reserved().items():
            slots[32 + b] += n
            cost[32 + b] += 3 * n
        placed = []

        def place(earliest, c, kind, payload, is_exp=False):
            t = int(earliest)
            while True:
                assert t < self.T_END + 40, (kind, payload)
                g = t % P
                if slots[g] + 1 <= cap_s[g] and cost[g] + c <= cap_c[g] and (not is_exp or nexp[g] < 2):
                    slots[g] += 1
                    cost[g] += c
                    nexp[g] += int(is_exp)
                    placed.append((t, kind, payload))
                    return t
                t += 1
        # row maxima: chain g may start 3 gaps after its last QK^T MFMA (12 wait states), one operation per gap and chain
        t_mx = {}
        for g in range(4):
            # (chain g's last MFMA is number 8 g + 7, or 16 qb + 14 + kb with the chains of a query block interleaved)
            t = 8 * g + 11 if "qk_chain_order" in self.abl else 16 * (g >> 1) + 18 + (g & 1)
            for j in range(8):
                t = place(t, 5, "mx", (g, j)) + 1
            t_mx[g] = t
        t_dec = {}
        for qb in range(2):
            t = max(t_mx[2 * qb], t_mx[2 * qb + 1])
            # (the compare and the branch on it sit in different gaps: back to back the branch waits ~30 cycles for the mask.
            # A job's first tile has no decision to take but keeps the slots: the loop body that finishes it is the one that
            # finishes every other tile, so both placements must agree)
            for part in range(5):
                # (the branch two gaps behind its compare: with one MFMA between them the scalar compare waits ~10 cycles for the
                # mask -- microbenchmark mb_cmps_a_scmp_brs against mb_cmps_aaa_scmp_brs -- and query block 0's pair sat in the last
                # gaps in front of the mid-step barrier; now its branch is the first thing behind the barrier)
                # (not where the lazy masking of the contiguous row map / the ragged key tail pins 'mr' in front of the last packs)
                gap2 = part == 4 and "fire_adjacent" not in self.abl and (self.split or not (self.causal or self.ragged))
                t = place(t + (1 if gap2 else 0), (9, 5, 9, 4, 2)[part], "dec", (qb, part)) + 1
            t_dec[qb] = t
        # (causal diagonal tiles handled lazily -- mask_lazy -- add four small operations at LAZY_TAU: gaps of phase A that are
        # nearly empty in every tile, so the plan itself does not reserve anything for them)
        t_d2 = {qb: next(t for t, k, p_ in placed if k == "dec" and p_ == (qb, 2)) for qb in range(2)}
        lz = self.lazy_tau()
        assert self.split or (lz["mr"] - P < lz["ms0"] < t_d2[0] and lz["mr"] - P < lz["ms1"] < t_d2[1])
        assert lz["pm"] < self.T_END
        # s' = s * c - m, exp2, pack -- element order inside a group is the packing order
        for qb in range(2):
            t_f = t_dec[qb]
            last_cv = {}
            for g in (2 * qb, 2 * qb + 1):
                t_e_prev = None
                for r in range(16):
                    e = 16 * g + r
                    tf = place(t_f, 5, "f", e)
                    t_f = tf  # keep the fma stream in order (several per gap allowed)
                    te = place(tf + 1, 8, "e", e, is_exp=True)
                    if r & 1:
                        j = r >> 1
                        tc = max(te, t_e_prev) + 1
                        if j - 1 in last_cv.get(g, {}):
                            tc = max(tc, last_cv[g][j - 1] + 0)
                        tc = place(tc, 5, "cv", (g, j))
                        last_cv.setdefault(g, {})[j] = tc
                    t_e_prev = te
        if self.causal or self.ragged:     # (the kernels that mask lazily)
            assert max(t for t, k, _ in placed if k == "cv") < (lz["pm"] if self.split else min(lz["mr"], lz["pm"])), \
                "a pack operation behind the packed-P masking"
        placed.sort(key=lambda x: x[0])
        assert max(t for t, _, _ in placed) < self.T_END, max(t for t, _, _ in placed)
        self._cache[key] = placed
        return placed

    def a_vread_gap(self, k):
        """phase-A gap of V transposed read k: two per gap at the start, none in the last four -- the wait in front of the barrier
        then finds the youngest read ~130 cycles old instead of just issued"""
        nd = self.vread_double
        return k // 2 if k < 2 * nd else k - nd

    def b_short_gaps(self):
        """indices (0..39) of the phase-B gaps that follow a 16x16x32 row-sum MFMA"""
        return [10 * k + 8 for k in range(4)] + [10 * k + 9 for k in range(4)]

    def b_reserved(self):
        """phase-B gap -> number of pre-reserved fillers (K reads, DMA loads, DMA scalar set-up)"""
        r = {}
        for k in range(self.K_READS):
            r[self.b_kread_gap(k)] = r.get(self.b_kread_gap(k), 0) + 1
        for k in range(2 * self.DMA_PIECES):
            g = self.b_dma_gap(k)
            r[g] = r.get(g, 0) + 1
            r[g - 1] = r.get(g - 1, 0) + 1
        return r

    def b_kread_gap(self, k):
        if "kfront" in self.abl:     # (experiment) two K reads per gap from the start of the phase
            g = k // 2
            while g in self.b_short_gaps():
                g += 1
            return g
        g = 2 * k
        while g in self.b_short_gaps():
            g += 1
        return g

    def b_dma_gap(self, k):
        """phase-B gap whose FIRST filler is DMA piece k's load; its scalar set-up (soffset, M0) ends the gap before, so the MFMA
        between them is the wait state the M0 write needs.  Distinct, two apart, clear of the short row-sum gaps."""
        return self.DMA_GAPS[k]

    def tile_op(self, Sb, kind, payload, init, lazy=None):
        """the instructions of one placed operation, for the tile whose scores live in score buffer Sb.
        lazy = (jd, cond): the tile is diagonal tile jd of its job (if cond holds) and masked lazily (mask_lazy)"""
        if kind in ("ms", "mr", "pm"):
            return self.mask_lazy(Sb, kind, payload, lazy)
        if kind == "mx":
            g, j = payload
            qb, kb = g >> 1, g & 1
            mx = V(self.V_MX[qb][kb])
            y = lambda r: V(Sb + 16 * g + r)
            if j == 0:
                return [I("v_max3_f32", mx, y(0), y(1), y(2), tag=f"max g{g}")]
            if j == 7:
                return [I("v_max_f32", mx, mx, y(15), tag=f"max g{g}")]
            return [I("v_max3_f32", mx, mx, y(2 * j + 1), y(2 * j + 2), tag=f"max g{g}")]
        if kind == "dec":
            qb, part = payload
            a, b = V(self.V_MX[qb][0]), V(self.V_MX[qb][1])
            d = V(self.V_T[qb])
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
                if init:
                    return [I("v_max_f32", a, a, b), I("v_mul_f32", V(self.V_MC[qb]), S_C, a)]
                return ([I("v_max_f32", a, a, b)] if full else []) + [I("v_fma_f32", d, a, S_C, -V(self.V_MC[qb]))]
            if init:
                return []
            if part == 3:
                return [I("v_cmp_gt_f32", S_FIRE[qb], d, S_THR)]
            if "fire_nobranch" in self.abl:       # (timing-only: the compare without its branch)
                return []
            l_fire, l_back = self.lab("fire"), self.lab("fire_back")
            # rare: raise this query block's running maximum now (every s' = s * c - m of the PREVIOUS tile has been formed:
            # plan order), remember the factor; O and the row sums are scaled at the end of the coming phase B
            t2, t3 = V(self.V_T[2 + 2 * qb]), V(self.V_T[3 + 2 * qb])
            exact = self.fire_exact(Sb, qb, lazy) if lazy is not None else []
            swap = [] if "full_max" in self.abl else [I("v_mov_b32", b, a), I("v_permlane32_swap_b32", a, b), I("v_max_f32", a, a, b)]
            if exact and "full_max" not in self.abl and "fire_noexact" not in self.abl:
                # a lazily masked diagonal tile: the partial maxima ran over hidden keys too.  With the exact maximum in hand, leave
                # again unless a row really passes the threshold -- the decision of the oracle's deferred mode (f16, threshold
                # 15.875: a hidden key beats it every few diagonal tiles, and a rescale costs ~2 000 cycles with three waves waiting)
                swap = swap + [I("v_fma_f32", t3, a, S_C, -V(self.V_MC[qb])), I("v_cmp_lt_f32", VCC, S_THR, t3), I("s_nop", 3),
                               I("s_cbranch_vccz", Label(l_back))]
            self.ool.append([label(l_fire)] + exact + swap + [I("v_mul_f32", t2, S_C, a), I("v_max_f32", t2, t2, V(self.V_MC[qb])),
                             I("v_sub_f32", t3, V(self.V_MC[qb]), t2), I("v_mov_b32", V(self.V_MC[qb]), t2), I("v_exp_f32", V(self.V_CO[qb]), t3),
                             I("s_or_b32", S_FLAG, S_FLAG, 1 << qb), I("s_branch", Label(l_back))])
            return [I("s_cmp_lg_u64", S_FIRE[qb], 0), I("s_cbranch_scc1", Label(l_fire)), label(l_back)]
        if kind == "f":
            e = payload
            y = V(Sb + e)
            return [I("v_fma_f32", y, y, S_C, -V(self.V_MC[e >> 5]), tag=f"fma {e}")]
        if kind == "e":
            y = V(Sb + payload)
            return [I("v_exp_f32", y, y, tag=f"exp {payload}")]
        if kind == "cv":
            g, j = payload
            return [I(self.cvt, V(Sb + 16 * g + j), V(Sb + 16 * g + 2 * j), V(Sb + 16 * g + 2 * j + 1), tag=f"cvt g{g} {j}")]
        raise KeyError(kind)

    @staticmethod
    def op_qb(kind, payload):
        """query block a placed softmax operation belongs to (None: not tied to one)"""
        if kind in ("mx", "cv"):
            return payload[0] >> 1
        if kind == "dec":
            return payload[0]
        if kind in ("f", "e"):
            return payload >> 5
        if kind == "ms":
            return payload
        return None

    def tile_fill(self, Sb, lo, hi, init, masks=None, abl=(), qbs=(0, 1)):
        """[(gap - lo, [insts], is_exp)] of the tile's operations with lo <= tau < hi.  masks: causal (jd, cond): the tile is
        diagonal tile jd of its job (when cond = (sgpr, value) holds, if given).  A job's first tile (init) gets its scores
        masked up front -- the tests of score group g go in front of its first row-maximum operation; every other diagonal
        tile is masked lazily (mask_lazy)"""
        out = []
        seen_mask = set()
        tail = masks is not None and masks[0] == "tail"     # non-causal ragged: ("tail", j[, cond]) -- seam tile j may hold keys >= N
        if tail:
            masks = masks[1:]
        jd, cond = (masks + (None,))[:2] if masks is not None else (None, None)
        lazy = (jd, cond) if masks is not None and not init else None
        plan = self.tile_plan(init)
        if lazy is not None:
            lz = self.lazy_tau()
            if self.split and not tail:
                # split row map: a hidden (tile, query block) is not computed at all -- no running-maximum swap ('ms' / 'mr');
                # the packed-P masking only where this body's waves sit on the tile's diagonal and the block is computed
                pm = self.cls is not None and (jd >> 1) in qbs and self.cls == ("low", "high")[jd & 1]
                plan = sorted(plan + ([(lz["pm"], "pm", None)] if pm else []), key=lambda x: x[0])
            else:
                plan = sorted(plan + [(lz["ms0"], "ms", 0), (lz["ms1"], "ms", 1), (lz["mr"], "mr", None)] +
                              ([] if tail else [(lz["pm"], "pm", None)]), key=lambda x: x[0])
        for t, kind, payload in plan:
            if not (lo <= t < hi):
                continue
            if self.op_qb(kind, payload) is not None and self.op_qb(kind, payload) not in qbs:
                continue
            if ("no_" + kind) in abl or (kind == "dec" and payload[1] >= 3 and "no_fire" in abl):
                continue   # timing-only ablations (diagnostic build)
            if tail:
                assert not init
                ins = self.mask_tail(Sb, kind, payload, jd, cond) if kind in ("ms", "mr") else self.tile_op(Sb, kind, payload, init, None)
            else:
                ins = self.tile_op(Sb, kind, payload, init, lazy)
            if not ins:
                continue
            if masks is not None and (init or tail) and kind == "mx" and payload[1] == 0 and payload[0] not in seen_mask:
                seen_mask.add(payload[0])
                ins = (self.mask_tail_tests(Sb, payload[0], jd, cond) if tail else self.mask_tests(Sb, payload[0], jd, cond)) + ins
            out.append((t - lo, ins, kind == "e"))
        return out

    def score_mask_ops(self, Y, g):
        """the wave ON the diagonal (w == jd): -inf into the scores of group g = 2 qb + kb whose key lies behind the query.
        (qb0, kb0) and (qb1, kb1) get the triangle, (qb0, kb1) is masked entirely, (qb1, kb0) not at all.  Register r of a
        group <-> key (r & 3) + 8 (r >> 2) + 4 h, lane <-> query i"""
        if g in (0, 3):
            out = []
            for r in range(16):
                key = (r & 3) + 8 * (r >> 2)
                out += [I("v_cmp_ge_i32", VCC, V(self.V_IMH), key), I("v_cndmask_b32", V(Y + 16 * g + r), self.NINF, V(Y + 16 * g + r), VCC)]
            return out
        if g == 1:
            return [I("v_mov_b32", V(Y + 16 + r), self.NINF) for r in range(16)]
        return []

    def group_mask_ops(self, Y, g, what):
        """-inf into the scores of group g: what = "tri" (key block == query block: keys behind the query) or "all".
        Register r of a group <-> key (r & 3) + 8 (r >> 2) + 4 h, lane <-> query i"""
        if what == "all":
            return [I("v_mov_b32", V(Y + 16 * g + r), self.NINF) for r in range(16)]
        out = []
        for r in range(16):
            key = (r & 3) + 8 * (r >> 2)
            out += [I("v_cmp_ge_i32", VCC, V(self.V_IMH), key), I("v_cndmask_b32", V(Y + 16 * g + r), self.NINF, V(Y + 16 * g + r), VCC)]
        return out

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
            g0, g1 = 2 * qa, 2 * qa + 1
            l_d1, l_back, l_skip = self.lab("pmask_d1"), self.lab("pmask_back"), self.lab("pmask_skip")
            self.ool.append([label(l_d1)] + [I("v_and_b32", V(Sb + 16 * g1 + j), V(Sb + 16 * g1 + j), V(self.V_PM[j])) for j in range(8)] +
                            [I("s_branch", Label(l_back))])
            head = [I("s_cmp_eq_u32", cond[0], cond[1]), I("s_cbranch_scc0", Label(l_skip))] if cond is not None else []
            return head + [I("s_bitcmp1_b32", S_WAVE, 0), I("s_cbranch_scc1", Label(l_d1))] + \
                [I("v_and_b32", V(Sb + 16 * g0 + j), V(Sb + 16 * g0 + j), V(self.V_PM[j])) for j in range(8)] + \
                [I("v_mov_b32", V(Sb + 16 * g1 + j), 0) for j in range(8)] + [label(l_back)] + ([label(l_skip)] if cond is not None else [])
        if kind == "pm":
            l_pm, l_back = self.lab("pmask"), self.lab("pmask_back")
            blk = [label(l_pm)]
            if cond is not None:
                blk += [I("s_cmp_eq_u32", cond[0], cond[1]), I("s_cbranch_scc0", Label(l_back))]
            for g in (0, 3):
                blk += [I("v_and_b32", V(Sb + 16 * g + j), V(Sb + 16 * g + j), V(self.V_PM[j])) for j in range(8)]
            blk += [I("v_mov_b32", V(Sb + 16 + j), 0) for j in range(8)]
            self.ool.append(blk + [I("s_branch", Label(l_back))])
            return [I("s_cmp_eq_u32", S_WAVE, jd), I("s_cbranch_scc1", Label(l_pm)), label(l_back)]
        if jd == 0:
            return []      # no wave lies below diagonal tile 0
        assert cond is None
        sel = [I("s_cmp_ge_u32", S_WAVE, jd), I("s_cselect_b64", VCC, -1, 0)]   # VCC: the tile is (partly) visible to this wave
        if kind == "ms":
            qb = payload
            return sel + [I("v_mov_b32", V(self.V_MSV[qb]), V(self.V_MC[qb])), I("v_cndmask_b32", V(self.V_MC[qb]), -self.NINF, V(self.V_MC[qb]), VCC)]
        return sel + [I("v_cndmask_b32", V(self.V_MC[qb]), V(self.V_MSV[qb]), V(self.V_MC[qb]), VCC) for qb in range(2)]

    def mask_tail(self, Sb, kind, payload, j, cond):
        """non-causal ragged, seam tile j (keys 64 j .. 64 j + 63 of the job's last 256; S_KT0 of them are real): a tile wholly
        behind N gets +inf for the running maximum like a tile below the causal diagonal (mask_lazy 'ms' / 'mr')"""
        if j == 0:
            return []          # at least one key of tile 0 is real
        assert cond is None
        sel = [I("s_cmp_gt_i32", S_KT0, 64 * j), I("s_cselect_b64", VCC, -1, 0)]     # VCC: the tile holds a real key
        if kind == "ms":
            qb = payload
            return sel + [I("v_mov_b32", V(self.V_MSV[qb]), V(self.V_MC[qb])), I("v_cndmask_b32", V(self.V_MC[qb]), -self.NINF, V(self.V_MC[qb]), VCC)]
        return sel + [I("v_cndmask_b32", V(self.V_MC[qb]), V(self.V_MSV[qb]), V(self.V_MC[qb]), VCC) for qb in range(2)]

    def mask_tail_tests(self, Y, g, j, cond):
        """in front of score group g's first row-maximum operation: if some of its 32 keys lie at or behind N (and some key of
        the tile is real: else mask_tail deals with it), -inf into those scores, out of line.  Register r of a group <-> key
        (r & 3) + 8 (r >> 2) + 4 h of the group's 32"""
        kb = g & 1
        l_m, l_back = self.lab("tail"), self.lab("tail_back")
        t = V(self.V_T[6])
        blk = [label(l_m)]
        if cond is not None:
            blk += [I("s_cmp_eq_u32", cond[0], cond[1]), I("s_cbranch_scc0", Label(l_back))]
        if j > 0:
            blk += [I("s_cmp_gt_i32", S_KT0, 64 * j), I("s_cbranch_scc0", Label(l_back))]
        # T = real keys of this group minus the lane half's offset: register r is kept iff T > (r & 3) + 8 (r >> 2)
        # (S_X2, the job decode's scratch: the S_T temporaries may be in the middle of a descriptor computation spread over gaps)
        blk += [I("s_sub_i32", S_X2, S_KT0, 64 * j + 32 * kb), I("v_lshrrev_b32", t, 5, V(self.V_LANE)), I("v_lshlrev_b32", t, 2, t),
                I("v_sub_u32", t, S_X2, t)]
        for r in range(16):
            blk += [I("v_cmp_gt_i32", VCC, t, (r & 3) + 8 * (r >> 2)), I("v_cndmask_b32", V(Y + 16 * g + r), self.NINF, V(Y + 16 * g + r), VCC)]
        self.ool.append(blk + [I("s_branch", Label(l_back))])
        # in line: one compare and an untaken branch while all 32 keys of the group are real
        return [I("s_cmp_lt_i32", S_KT0, 64 * j + 32 * kb + 32), I("s_cbranch_scc1", Label(l_m)), label(l_back)]

    def fire_exact(self, Sb, qb, lazy):
        """head of the rare rescale path of a lazily masked diagonal tile: on the wave that sits on the diagonal the row maxima
        were taken over masked keys too -- mask this query block's scores now and take the maxima again (then the plain path
        decides with the exact maximum; the packed-P masking later is a no-op on the -inf entries)"""
        jd, cond = lazy
        l_plain = self.lab("fire_plain")
        a, b = V(self.V_MX[qb][0]), V(self.V_MX[qb][1])
        blk = []
        if self.split:
            # only query block jd >> 1 has waves on the diagonal of tile jd: waves 2 p (pattern D0) and 2 p + 1 (D1), p = jd & 1
            if qb != jd >> 1:
                return []
            p2 = 2 * (jd & 1)
            l_d1, l_max = self.lab("fire_d1"), self.lab("fire_max")
            if cond is not None:
                blk += [I("s_cmp_eq_u32", cond[0], cond[1]), I("s_cbranch_scc0", Label(l_plain))]
            blk += [I("s_cmp_eq_u32", S_WAVE, p2 + 1), I("s_cbranch_scc1", Label(l_d1)),
                    I("s_cmp_eq_u32", S_WAVE, p2), I("s_cbranch_scc0", Label(l_plain))]
            blk += self.group_mask_ops(Sb, 2 * qb, "tri") + self.group_mask_ops(Sb, 2 * qb + 1, "all") + [I("s_branch", Label(l_max))]
            blk += [label(l_d1)] + self.group_mask_ops(Sb, 2 * qb + 1, "tri") + [label(l_max)]
            for g, mx in ((2 * qb, a), (2 * qb + 1, b)):
                y = lambda r: V(Sb + 16 * g + r)
                blk += [I("v_max3_f32", mx, y(0), y(1), y(2))] + [I("v_max3_f32", mx, mx, y(2 * j + 1), y(2 * j + 2)) for j in range(1, 7)] + \
                    [I("v_max_f32", mx, mx, y(15))]
            blk += [I("v_max_f32", a, a, b), I("v_mov_b32", b, a), I("v_permlane32_swap_b32", a, b), I("v_max_f32", a, a, b), label(l_plain)]
            return blk
        if cond is not None:
            blk += [I("s_cmp_eq_u32", cond[0], cond[1]), I("s_cbranch_scc0", Label(l_plain))]
        blk += [I("s_cmp_eq_u32", S_WAVE, jd), I("s_cbranch_scc0", Label(l_plain))]
        for g, mx in ((2 * qb, a), (2 * qb + 1, b)):
            blk += self.score_mask_ops(Sb, g)
            y = lambda r: V(Sb + 16 * g + r)
            blk += [I("v_max3_f32", mx, y(0), y(1), y(2))] + [I("v_max3_f32", mx, mx, y(2 * j + 1), y(2 * j + 2)) for j in range(1, 7)] + \
                [I("v_max_f32", mx, mx, y(15))]
        blk += [I("v_max_f32", a, a, b), I("v_mov_b32", b, a), I("v_permlane32_swap_b32", a, b), I("v_max_f32", a, a, b), label(l_plain)]
        return blk

    def mask_tests(self, Y, g, jd, cond=None):
        """causal: the tile whose softmax starts is diagonal tile jd (0..3) of its job: keys 64 jd .. 64 jd + 63 of the 256-key
        diagonal span against this wave's rows 64 w .. 64 w + 63.  w > jd: nothing; w == jd: score groups (qb0, kb0) and
        (qb1, kb1) get the triangle (key > query -> -inf), (qb0, kb1) is all -inf; w < jd: all -inf.  Register r of a
        group <-> key (r & 3) + 8 (r >> 2) + 4 h, lane <-> query i.  cond: (sgpr, value): the tile is diagonal at all.
        Returns the in-line tests for score group g (in front of its first row-maximum operation); the masking itself runs
        out of line.  The branch sits where that row-maximum operation is legal, i.e. the MFMA -> VALU wait states have passed
        (check.check_branch_targets verifies it on the built program)."""
        if self.split:
            # waves 2 p / 2 p + 1 (p = jd & 1) carry patterns D0 / D1 on query block jd >> 1 (see mask_lazy); a block wholly
            # hidden from a wave is not computed at all by the split bodies
            l_back = self.lab("mask_back")
            qb, kb = g >> 1, g & 1
            if qb != jd >> 1:
                return []
            p2 = 2 * (jd & 1)
            tests = []
            l_d0 = self.lab("mask_d0")
            self.ool.append([label(l_d0)] + self.group_mask_ops(Y, g, "tri" if kb == 0 else "all") + [I("s_branch", Label(l_back))])
            tests += [I("s_cmp_eq_u32", S_WAVE, p2), I("s_cbranch_scc1", Label(l_d0))]
            if kb == 1:
                l_d1 = self.lab("mask_d1")
                self.ool.append([label(l_d1)] + self.group_mask_ops(Y, g, "tri") + [I("s_branch", Label(l_back))])
                tests += [I("s_cmp_eq_u32", S_WAVE, p2 + 1), I("s_cbranch_scc1", Label(l_d1))]
            if cond is None:
                return tests + [label(l_back)]
            l_tests = self.lab("mask_tests")
            self.ool.append([label(l_tests)] + tests + [I("s_branch", Label(l_back))])
            return [I("s_cmp_eq_u32", cond[0], cond[1]), I("s_cbranch_scc1", Label(l_tests)), label(l_back)]
        l_eq, l_lt, l_back = self.lab("mask_eq"), self.lab("mask_lt"), self.lab("mask_back")
        tests = []
        eq_ops = self.score_mask_ops(Y, g)
        if eq_ops:
            tests += [I("s_cmp_eq_u32", S_WAVE, jd), I("s_cbranch_scc1", Label(l_eq))]
            self.ool.append([label(l_eq)] + eq_ops + [I("s_branch", Label(l_back))])
        if jd > 0:
            tests += [I("s_cmp_lt_u32", S_WAVE, jd), I("s_cbranch_scc1", Label(l_lt))]
            self.ool.append([label(l_lt)] + [I("v_mov_b32", V(Y + 16 * g + r), self.NINF) for r in range(16)] +
                            [I("s_branch", Label(l_back))])
        if cond is None:
            return tests + [label(l_back)]
        if not tests:
            return []
        # the tile is diagonal only in the loop's last trip (or for a one-tile-row job): the common path falls through one
        # compare and one untaken branch -- a TAKEN branch over the tests cost ~25 cycles per step in the steady loop
        l_tests = self.lab("mask_tests")
        self.ool.append([label(l_tests)] + tests + [I("s_branch", Label(l_back))])
        return [I("s_cmp_eq_u32", cond[0], cond[1]), I("s_cbranch_scc1", Label(l_tests)), label(l_back)]

    def phase_a(self, t4, with_qk=True, cur=True, nxt=True, nxt_init=False, masks=None, steady=False, dma=(), cur_masks=None, extra=(),
                cur_qbs=(0, 1), nxt_qbs=(0, 1)):
        """A(t), t4 = t & 3: QK^T(t+1) -> S[1-p]  ||  V(t) reads from VB[t % R]  ||  the late softmax operations of tile t (on S[p])
        ||  the early ones of tile t+1 (on S[1-p])"""
        p = t4 & 1
        X, Y = SBUF[p], SBUF[1 - p]
        abl = self.abl if steady else set()
        mf = self.qk_mfmas(Y, qbs=nxt_qbs) if with_qk else []
        gaps = {}
        add = lambda k, order, ins: gaps.setdefault(min(max(int(k), 0), 31), []).append((order, ins))
        if cur:
            if "novread" not in abl:
                for k, ins in enumerate(self.v_reads(t4 % self.R)):
                    add(self.a_vread_gap(k), 0, [ins])
            if "nofinish" not in abl:
                for k, ins, is_exp in self.tile_fill(X, 32 + self.NB, self.T_END, False, cur_masks, abl=abl, qbs=cur_qbs):
                    add(k, 1 if is_exp else 2, ins)
        if nxt and "nostart" not in abl:
            for k, ins, is_exp in self.tile_fill(Y, 0, 32, nxt_init, masks, abl=abl, qbs=nxt_qbs):
                add(k, 1 if is_exp else 2, ins)
        for g, ins in extra:
            add(g, 2, ins)
        for g, setup, load in dma:   # LDS-DMA pieces riding in this phase (the seam's Q rows): set-up ends gap g - 1, load opens gap g
            add(g - 1, 3, setup)
            add(g, 0, [load])
        if not mf:
            return [x for k in sorted(gaps) for _, ins in sorted(gaps[k], key=lambda x: x[0]) for x in ins]
        return self.emit_phase(mf, gaps)

    def phase_b(self, t4, with_pv=True, nxt=True, nxt_init=False, with_kread=True, with_dma=True, steady=False,
                pre=(), early=(), late=(), masks=None, own_gaps=None, post=(), cur_qbs=(0, 1), nxt_qbs=(0, 1)):
        """B(t), t4 = t & 3: P.V(t) and the row sums of P(t) from S[p]  ||  the middle softmax operations of tile t+1 (on S[1-p])
        ||  K(t+2) reads from KB[(t+2) % R]  ||  LDS-DMA V(t+dv) -> VB[(t+dv) % R], K(t+dk) -> KB[(t+dk) % R].
        pre: instructions ahead of the phase;  early: scalar work / register loads spread over the first gaps;
        late: further DMA pieces (the next job's Q rows) as (gap, set-up, load);  own_gaps: the gaps of this step's own pieces"""
        p = t4 & 1
        X, Y = SBUF[p], SBUF[1 - p]
        abl = self.abl if steady else set()
        mf = self.pv_mfmas(X, qbs=cur_qbs) if with_pv else []
        NB = self.NB
        gaps = {}
        add = lambda k, order, ins: gaps.setdefault(min(max(int(k), 0), NB - 1), []).append((order, ins))
        head = list(pre)
        post, post_arg = [], list(post)
        if with_kread and "nokread" not in abl:
            for k, ins in enumerate(self.k_reads((t4 + 2) % self.R)):
                add(self.b_kread_gap(k), 0, [ins])
        if with_dma:
            pieces = [self.dma_piece("v", j, (t4 + self.dv) % self.R) for j in range(self.DMA_PIECES)] + \
                [self.dma_piece("k", j, (t4 + self.dk) % self.R) for j in range(self.DMA_PIECES)]
            for k, pc in enumerate(pieces):
                if "nodma" in abl:
                    continue
                # (with further pieces behind them -- the seam's Q rows -- this step's own go first: the counted waits
                # assume all eight are older than the sixteen)
                g = own_gaps[k] if own_gaps else self.b_dma_gap(k)
                # scalar set-up (soffset, M0) at the end of the previous gap, the load first in its own: the MFMA between
                # them is the wait state the M0 write needs
                setup, load = [x for x in pc if not x.op.startswith("buffer_load") and x.op != "s_nop"], [x for x in pc if x.op.startswith("buffer_load")]
                add(g - 1, 3, setup)
                add(g, 0, load if mf else [I("s_nop", 0)] + load)
            post += [I("s_add_u32", S_VDMA, S_VDMA, S_V64), I("s_add_u32", S_KDMA, S_KDMA, S_K64)]
        # scalar work rides in the first gaps one UNIT at a time: an instruction that consumes SCC (the s_addc of a 64-bit
        # add, a select or branch on a compare) stays glued to the instructions since its producer -- other fillers write
        # SCC too (the DMA set-up's s_add_u32), and a descriptor base once lost its carry that way (check.py R9)
        units = []
        for ins in early:
            d_, u_ = ins.defs_uses()
            if ("scc", 0) in u_ and units:
                units[-1].append(ins)
            else:
                units.append([ins])
        ne = len(units)
        for k, unit in enumerate(units):
            add(1 + 12 * k // max(ne, 1), 2, unit)   # done before this phase's own DMA pieces (gap 15 on) and the late ones
        for g, setup, load in late:   # (gap pairs disjoint from the own pieces': both use M0 and the scratch offset register)
            add(g - 1, 3, setup)
            add(g, 0, [load])
        if nxt and "nostart" not in abl:
            for k, ins, is_exp in self.tile_fill(Y, 32, 32 + NB, nxt_init, masks, abl=abl, qbs=nxt_qbs):
                add(k, 1 if is_exp else 2, ins)
        if not mf:
            body = [x for k in sorted(gaps) for _, ins in sorted(gaps[k], key=lambda x: x[0]) for x in ins]
        else:
            body = self.emit_phase(mf, gaps)
        body = head + body + post + post_arg
        # deferred rescale of O and the row sums by the factors the decisions of this step left (rare)
        l_rs, l_back = self.lab("rescale"), self.lab("rescale_back")
        body += [I("s_cmp_lg_u32", S_FLAG, 0), I("s_cbranch_scc1", Label(l_rs)), label(l_back)]
        # (bit qb of S_FLAG: query block qb fired in this step -- only its accumulators are touched; packed multiplies: the
        # matrix pipe is idle here.  f16 inputs fire a few times per job: P must stay below 65 504)
        blk = [label(l_rs), I("s_nop", 15)]
        tmp = [V(self.V_T[k]) for k in range(8)]
        co = V(self.V_T[8], 2)      # (an even register: the factor is read as the low word of an aligned 64-bit operand)
        for qb in range(2):
            blk += self.rescale(qb, tmp, co)
        blk += [I("s_mov_b32", S_FLAG, 0), I("s_nop", 3), I("s_branch", Label(l_back))]
        self.ool.append(blk)
        return body

    def rescale(self, qb, tmp, co):
        """the out-of-line rescale of query block qb (bit qb of S_FLAG): its O^T accumulators and row sums times V_CO[qb]"""
        l_skip = self.lab("rescale_skip")
        n = self.O_AGPRS // 2
        blk = [I("s_bitcmp1_b32", S_FLAG, qb), I("s_cbranch_scc0", Label(l_skip)), I("v_mov_b32", co.sub(0), V(self.V_CO[qb]))]
        for base in range(0, n, 8):
            regs = [A(qb * n + base + k) for k in range(8)]
            blk += [I("v_accvgpr_read_b32", tmp[k], regs[k]) for k in range(8)]
            blk += [I("v_pk_mul_f32", V(tmp[k].idx, 2), V(tmp[k].idx, 2), co, op_sel_hi=(1, 0)) for k in range(0, 8, 2)]
            blk += [I("v_accvgpr_write_b32", regs[k], tmp[k]) for k in range(8)]
        blk += [I("v_pk_mul_f32", V(self.V_LACC[qb] + k, 2), V(self.V_LACC[qb] + k, 2), co, op_sel_hi=(1, 0)) for k in (0, 2)]
        return blk + [I("v_mov_b32", V(self.V_CO[qb]), 1.0), label(l_skip)]

    def sync_mid(self, steady=False, vm=None):
        if vm is not None:
            return [waitcnt(vmcnt=vm, lgkmcnt=0), I("s_barrier")]
        if steady and "novmwait" in self.abl:
            return [waitcnt(lgkmcnt=0), I("s_barrier")]
        if steady and "nobarrier" in self.abl:
            return [waitcnt(vmcnt=self.vm, lgkmcnt=0)]
        out = [waitcnt(vmcnt=self.vm, lgkmcnt=0, comment="the DMA pieces the next reads need have landed; V fragments in"), I("s_barrier")]
        if steady and "skew" in self.abl:   # experiment: wave w leaves the barrier 8 w cycles late
            l1, l2 = self.lab("skew1"), self.lab("skew2")
            out += [I("s_bitcmp1_b32", S_WAVE, 0), I("s_cbranch_scc0", Label(l1)), I("s_nop", 7), label(l1),
                    I("s_bitcmp1_b32", S_WAVE, 1), I("s_cbranch_scc0", Label(l2)), I("s_nop", 15), label(l2)]
        return out

    def step(self, t4, a_pre=(), **kw):
        """one tile step, t4 = t & 3"""
        ka = {k: v for k, v in kw.items() if k in ("with_qk", "cur", "nxt", "nxt_init", "steady", "dma", "cur_masks", "extra",
                                                   "cur_qbs", "nxt_qbs")}
        kb = {k: v for k, v in kw.items() if k in ("with_pv", "nxt", "nxt_init", "with_kread", "with_dma", "steady", "pre", "early", "late",
                                                   "own_gaps", "post", "cur_qbs", "nxt_qbs")}
        if kw.get("masks") is not None:   # the masking tests of a score group sit in front of its first row-maximum operation
            ka["masks"] = kw["masks"]
            kb["masks"] = kw["masks"]
        out = [comment(f"---- step {t4}: phase A")]
        out += self.stamp_acc(2)
        out += list(a_pre)
        out += [waitcnt(lgkmcnt=0, comment="K fragments in")]
        out += self.phase_a(t4, **ka)
        out += self.stamp_acc(0)
        out += self.sync_mid(kw.get("steady", False), kw.get("vm"))
        out += self.stamp_acc(1)
        if kw.get("mid_stamp") is not None:      # (diagnostic builds: the seam's steps 2 and 3 split at their barrier)
            out += self.stamp(kw["mid_stamp"])
        out += [comment(f"---- step {t4}: phase B")]
        out += self.phase_b(t4, **kb)
        return out

    def epilogue_descs(self):
        """descriptors of the current job's O rows (S_SQ: the next job's Q rows are through by then) and L (S_NVRS: the next job's V
        descriptor has moved to S_VRS): scalar work that rides in the gaps of the seam's last phase B instead of standing in
        front of the epilogue"""
        return self.make_desc(S_SQ, S_O, S_OSB, S_OSH, S_B, S_HH, S_OSN) + self.make_desc(S_NVRS, S_L, S_LSB, S_LSH, S_B, S_HH, self.L_SN)

    def build(self):
        e = self.e
        name = self.name
        l_job, l_loop, l_seam, l_end = (f".L{name}_{s}" for s in ("job", "loop", "seam", "end"))
        self.k_setup()
        e(I("s_cmp_ge_u32", S_JOB, S_TOTAL), I("s_cbranch_scc1", Label(l_end)))
        # ---- first job of this workgroup: decode, descriptors, first loads, pipeline fill
        self.k_decode_next()
        self.k_promote()
        self.k_advance()      # (every later job is decoded in its predecessor's epilogue, under the row stores)
        e(comment("first job: K / V descriptors, K(0..2), V(0..1) by LDS-DMA, Q rows"))
        e(self.make_desc(S_KRS, S_K, S_KSB, S_KSH, S_B, S_HH, S_KSN), self.make_desc(S_VRS, S_V, S_VSB, S_VSH, S_B, S_HH, S_VSN))
        e(I("s_mov_b32", S_KDMA, S_KW), I("s_mov_b32", S_VDMA, S_VW))
        e(self.stamp(0))
        # (the first QK^T needs the Q rows and K(0) only: they go first, and the wait in front of the first barrier leaves the other
        # tiles in flight -- all 256 workgroups start at once and the burst is bandwidth-bound, ~7 us for everything)
        qs_setup, qs_pieces = self.q_stage(S_B, S_HH, S_QI)
        e(qs_setup, [pc + [I("s_nop", 0), ld] for pc, ld in qs_pieces])
        late = []
        for j in range(self.dk - 1):
            (e if j == 0 and "prologue_old" not in self.abl else late.append)(self.dma_tile("k", j % self.R))
            if j < self.dv - 1:
                late.append(self.dma_tile("v", j % self.R))
        e(late)
        n_late = sum(1 for t in late for x in t if x.op.startswith("buffer_load")) if "prologue_old" not in self.abl else 0   # (A/B variant: wait for everything)
        e([I("v_accvgpr_write_b32", A(k), 0) for k in range(self.O_AGPRS)])   # O^T := 0
        e(waitcnt(vmcnt=n_late), I("s_barrier"))
        e(self.stamp(1))
        e(self.q_reads(), self.k_reads(0))
        # step -1 (buffers as t4 = 3): A = QK^T(0) only; B = start(0) as init, K(1) reads, DMA V(2), K(3)
        e(self.step(3, with_qk=True, cur=False, with_pv=False, nxt_init=True, masks=(0, (S_NT, 4)) if self.causal else None))
        e(self.stamp(2), self.stamp_flush(), self.stamp_acc(3), self.stamp_job(3))
        # ---- job loop
        e(label(l_job))
        e(I("s_lshr_b32", S_LOOP, S_NT, 2), I("s_sub_u32", S_LOOP, S_LOOP, 1),
          I("s_cmp_eq_u32", S_LOOP, 0), I("s_cbranch_scc1", Label(l_seam)))
        e(label(l_loop))
        for t4 in range(4):
            # causal: the last steady body starts the job's first diagonal tile in its last phase B
            tailm = ("tail", 0, (S_LOOP, 1)) if self.ragged and not self.causal else None
            # (the K tile streamed in step 1 of the last trip and the V tile of its step 2 are the first of the diagonal span)
            jump = self.stream_to_diagonal("k") if t4 == 4 - self.dk else self.stream_to_diagonal("v") if t4 == 4 - self.dv else []
            e(self.step(t4, steady=True, masks=((0, (S_LOOP, 1)) if self.causal else tailm) if t4 == 3 else None, early=jump))
        e(I("s_sub_u32", S_LOOP, S_LOOP, 1), I("s_cmp_lg_u32", S_LOOP, 0), I("s_cbranch_scc1", Label(l_loop)))
        e(label(l_seam))
        e(self.stamp(3), self.stamp_acc(2), self.stamp_flush(), self.stamp_job(0))
        # ---- the job's last four tiles: the next job's K / V / Q stream in, its first QK^T and softmax start run here
        cm = self.causal
        kpre = self.make_desc(S_KRS, S_K, S_KSB, S_KSH, S_NB, S_NHH, S_KSN) + self.stream_start("k") + \
            self.make_desc(S_NVRS, S_V, S_VSB, S_VSH, S_NB, S_NHH, S_VSN)
        vpre = [I("s_mov_b32", S_VRS.sub(k), S_NVRS.sub(k)) for k in range(4)] + self.stream_start("v")
        sk, sv = 4 - self.dk, 4 - self.dv      # seam step whose phase B streams the next job's first K / V tile
        assert sk <= 2 and sv <= 2             # (step 3 re-uses S_SQ and S_NVRS for the epilogue's descriptors)
        qs_setup, qs_pieces = self.q_stage(S_NB, S_NHH, S_NQI)
        own, late0, dma1, late1, vm1 = self.QS_GAPS
        n0, n1 = len(late0), len(late0) + len(dma1)
        for st in range(4):
            kw = dict(masks=((st + 1,) if st < 3 else (0, (S_NNT, 4))) if cm else None, cur_masks=(st,) if cm else None)
            if self.ragged and not cm:   # keys at or behind N in the job's last four tiles (a ragged N has at least eight)
                kw = dict(masks=("tail", st + 1) if st < 3 else None, cur_masks=("tail", st))
            early, pre = [], []
            if st == 0:
                # the next job's Q rows start their way into the wave's LDS slice, never more than one DMA piece per two
                # gaps (that rate is free beside the MFMAs): behind this step's own K / V pieces, in the quiet end of the
                # next phase A, in front of the next step's own (QS_GAPS).  The barrier waits in between leave them in
                # flight; the one of step 2 retires them
                early += qs_setup
                kw.update(own_gaps=own, late=[(g, *qs_pieces[k]) for k, g in enumerate(late0)])
            if st == 1:
                kw.update(vm=self.vm + vm1,
                          dma=[(g, *qs_pieces[n0 + k]) for k, g in enumerate(dma1)],
                          late=[(g, *qs_pieces[n1 + k]) for k, g in enumerate(late1)])
            if st == sk:
                early += kpre
            if st == sv:
                pre += vpre
            if st == 2 and "noqreads" not in self.abl:   # (timing-only ablation: what the AGPR-destination reads cost)
                early += self.q_reads()      # slice -> a[128:191] (Q was last read by this step's phase A)
            if st == 3:
                early += self.epilogue_descs()
                # the job's last tile: its running maxima are put aside for the epilogue before the next job's first
                # tile re-initialises them (its row sums stay in V_LACC until the epilogue has read them)
                save = [I("v_mov_b32", V(msv), V(mc)) for msv, mc in zip(self.V_MSV, self.V_MC)]
                if (cm and not self.split) or (self.ragged and not cm):   # (behind the tile's 'mr': until then V_MSV holds what 'ms' put aside, mask_lazy)
                    kw.update(nxt_init=True, extra=list(kw.get("extra", ())) + [(self.LAZY_TAU["mr"] - self.PERIOD + 1, save)])
                else:
                    kw.update(nxt_init=True, a_pre=save)
            e(self.stamp(16 + st))
            if self.split:
                # split row map (wave w: 32-row blocks w and w + 4).  Diagonal tile j -- key blocks 2 j, 2 j + 1 -- against
                # query block 0 (row block w): hidden for w < 2 j, on the diagonal for w = 2 j (D0) / 2 j + 1 (D1), visible
                # above; against query block 1 (row block w + 4): the same with w + 4.  So tile 0: everything runs (waves
                # 0 / 1 mask block 0), tile 1: block 0 only on waves 2, 3 (which mask it), tile 2: block 1 only (waves 0 / 1
                # mask), tile 3: block 1 on waves 2, 3 only (which mask).  Step st finishes tile st and starts tile st + 1:
                # two bodies per step, waves 0-1 ("low") out of line, waves 2-3 ("high") in line, each with only the MFMAs
                # and softmax operations of the blocks it needs -- 216 MFMA slots on the critical path instead of 288.
                cur_q = (((0, 1), (0, 1)), ((1,), (0, 1)), ((1,), (1,)), ((), (1,)))[st]
                nxt_q = (((1,), (0, 1)), ((1,), (1,)), ((), (1,)), ((0, 1), (0, 1)))[st]
                l_low, l_join = self.lab("low"), self.lab("low_join")
                e(I("s_cmp_lt_u32", S_WAVE, 2), I("s_cbranch_scc1", Label(l_low)))
                for ci, cls in ((1, "high"), (0, "low")):
                    ckw = dict(kw)
                    cq, nq_ = cur_q[ci], nxt_q[ci]
                    ckw.update(cur_qbs=cq or (0, 1), nxt_qbs=nq_ or (0, 1))
                    if not cq:
                        ckw.update(cur=False, with_pv=False)
                    if not nq_:
                        ckw.update(with_qk=False, nxt=False)
                    self.cls = cls
                    if cls == "high":
                        e(self.step(st, early=early, pre=pre, mid_stamp=20 + st if st >= 2 else None, **ckw), label(l_join))
                    else:
                        body, self.prog = self.prog, []
                        e(label(l_low), self.step(st, early=early, pre=pre, **ckw), I("s_branch", Label(l_join)))
                        self.ool.append(self.prog)
                        self.prog = body
                    self.cls = None
                continue
            lean = cm and st >= 1 and "nolean" not in self.abl
            half = cm and st < 3 and "nolean" not in self.abl
            if lean:
                # waves below this step's diagonal tile (w < st): the tile whose softmax finishes and whose P.V runs here is
                # hidden from them, and so is the one that starts (steps 1, 2; step 3 starts the next job's first tile).
                # They take a body with the same loads, DMA pieces, waits and barriers but without those MFMAs and softmax
                # operations, and idle at the barriers: at the package power limit what one wave does not execute, the
                # others run faster (+1.2 % on c3 causal, A/B in one process).  Such a wave's running maximum was swapped for
                # +inf when the hidden tile started ('ms'): the lean body puts it back.
                l_lean, l_join = self.lab("lean"), self.lab("lean_join")
                e(I("s_cmp_lt_u32", S_WAVE, st), I("s_cbranch_scc1", Label(l_lean)))
            if half:
                # the wave ON this step's diagonal (w == st): the tile that starts here is hidden from it -- no QK^T, no start
                # of its softmax (+0.2 % at c3, +1 % at N = 2048 on top of the lean bodies)
                l_half = self.lab("half")
                l_join2 = l_join if lean else self.lab("half_join")
                e(I("s_cmp_eq_u32", S_WAVE, st), I("s_cbranch_scc1", Label(l_half)))
            e(self.step(st, early=early, pre=pre, **kw))
            if lean or half:
                e(label(l_join if lean else l_join2))
                body, self.prog = self.prog, []
                if lean:
                    lkw = dict(kw)
                    lkw["a_pre"] = [I("v_mov_b32", V(self.V_MC[qb]), V(self.V_MSV[qb])) for qb in range(2)] + list(kw.get("a_pre", ()))
                    lkw.update(dict(with_qk=False, cur=False, nxt=False, with_pv=False) if st < 3 else dict(cur=False, with_pv=False))
                    e(label(l_lean), self.step(st, early=early, pre=pre, **lkw), I("s_branch", Label(l_join)))
                if half:
                    hkw = dict(kw)
                    # (no 'ms' runs for the hidden tile: the lean body of the next step restores from V_MSV all the same)
                    hkw["a_pre"] = list(kw.get("a_pre", ())) + [I("v_mov_b32", V(self.V_MSV[qb]), V(self.V_MC[qb])) for qb in range(2)]
                    hkw.update(with_qk=False, nxt=False)
                    e(label(l_half), self.step(st, early=early, pre=pre, **hkw), I("s_branch", Label(l_join2)))
                self.ool.append(self.prog)
                self.prog = body
        e(self.stamp(4), self.stamp_job(1))
        self.k_epilogue()
        e(self.stamp(5))
        # (S_FLAG: S_FINAL as it stood in front of the epilogue's job bookkeeping; back to 0 for the next step's rescale flag)
        e(I("s_cmp_lg_u32", S_FLAG, 0), I("s_mov_b32", S_FLAG, 0), I("s_cbranch_scc1", Label(l_end)))
        e(self.stamp(0), self.stamp_acc(3), self.stamp_job(2))
        e(I("s_branch", Label(l_job)))
        e(label(l_end), self.stamp_job(2), self.stamp_job_flush(), waitcnt(vmcnt=0), self.stamp(7, real=True), self.stamp(9), I("s_endpgm"))
        for blk in self.ool:
            e(blk)
        from .check import check_branch_targets, fix
        self.prog, self.pads = fix(self.prog)
        bad = check_branch_targets(self.prog, need=self.BRANCH_NEED)
        assert not bad, ("a branch enters a block that touches fresh MFMA results", bad[:4])
        return self.prog

    def lds_total(self):
        return self.LDS_TOTAL

    def text(self):
        lines = [f".protected {self.name}", f".globl {self.name}", ".p2align 8", f".type {self.name},@function", f"{self.name}:"]
        lines += [x.text() for x in self.prog]
        lines += [f".L{self.name}_fend:", f".size {self.name}, .L{self.name}_fend-{self.name}", "",
                  '.section .rodata,"a",@progbits', ".p2align 6, 0x0", f".amdhsa_kernel {self.name}",
                  f"  .amdhsa_group_segment_fixed_size {self.lds_total()}", "  .amdhsa_private_segment_fixed_size 0",
                  f"  .amdhsa_kernarg_size {KARG_SIZE}", "  .amdhsa_user_sgpr_count 2", "  .amdhsa_user_sgpr_kernarg_segment_ptr 1",
                  "  .amdhsa_system_sgpr_workgroup_id_x 1", "  .amdhsa_system_vgpr_workitem_id 0",
                  "  .amdhsa_next_free_vgpr 512", "  .amdhsa_next_free_sgpr 102", "  .amdhsa_accum_offset 256",
                  "  .amdhsa_reserve_vcc 1", "  .amdhsa_ieee_mode 1", "  .amdhsa_dx10_clamp 1",
                  "  .amdhsa_float_round_mode_32 0", "  .amdhsa_float_round_mode_16_64 0",
                  "  .amdhsa_float_denorm_mode_32 3", "  .amdhsa_float_denorm_mode_16_64 3", ".end_amdhsa_kernel", ".text", ""]
        return "\n".join(lines)

    def metadata(self):
        return "\n".join([
            f"  - .args:", f"      - .offset: 0", f"        .size: {KARG_SIZE}", f"        .value_kind: by_value",
            f"    .group_segment_fixed_size: {self.lds_total()}", f"    .kernarg_segment_align: 8", f"    .kernarg_segment_size: {KARG_SIZE}",
            f"    .max_flat_workgroup_size: 256", f"    .name: {self.name}", f"    .private_segment_fixed_size: 0",
            f"    .sgpr_count: 108", f"    .symbol: {self.name}.kd", f"    .vgpr_count: 512", f"    .agpr_count: 256",
            f"    .wavefront_size: 64"])
