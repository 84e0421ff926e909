// vit_pk_tb.h -- the block-parallel speculative traceback of the packed kernels, both forms (see the file comment of vit_pk.hip),
// and the VIT_DIAG_SPEC counters of what it did.
#pragma once
#include "vit_pk_acs.h"

namespace {

// ---- traceback -------------------------------------------------------------------------------
// The path is followed in PHYSICAL coordinates: (l, n) = lane (within the pair) and register
// (N0/N1) that held the survivor decision of the state on the path after step t.  With
// j = 4 - ((t-1) mod 5), the lane bit exchanged before step t, one step back is
//     n' = bit j of l,   l' = l with bit j replaced by the decision k read at step t
// (this is ChainBack's E = (E>>1)|(k<<7), deconvolve.cpp:424-433, seen through the rotating
// lane<->state map).  The history words hold NOT k, so the code tracks the complement
// P = (31-l)<<3 | (1-n)<<2 - the stored bit is inserted unchanged - and the decision blocks are laid
// out in LDS in those same complemented coordinates (dec_slot() below), so that P IS the byte offset
// of the history word inside its block.  State 0 is P = 252.
constexpr u32 P_ZERO = 252u;
constexpr u32 TB_WARM = 30;  // warm-up steps (multiple of 5) a speculative block starts above its own range; the fast form is written for 30
// Input without signal (uniform random bytes, hard decisions from a dead channel) merges late: after 30 steps back from
// state 0 half of the blocks are still off the survivor path (3 % at Eb/N0 = 3 dB), after 90 steps 12 %
// (profiles/r03_merge_depth.txt).  A wave that sees at least TB_HARD_MISSES of its 64 blocks miss in the first pass of a
// part traces the parts that follow with the longer warm-up: one long pass instead of a chain of re-trace passes
// (profiles/r03_inputs.txt: 73.8 -> 75.4 Gbit/s on uniform random bytes, 3 dB input unchanged).
constexpr u32 TB_WARM_HARD = 90, TB_HARD_MISSES = 8;

#ifdef VIT_DIAG_SPEC  /* test build: what the traceback did.  The long-frame kernel's fast groups - [0] groups, [1] parts traced in flight,
                        [2] groups that gave up tracing in flight (input without signal), [3] parts traced after the forward pass beyond
                        part 0, [4] of those: parts that had been traced in flight and failed their check.  Every packed kernel - [5] blocks
                        of the fast form (parts traced from a known top) that missed in the first pass, [6] re-trace passes the fast form
                        ran, [7] general-form parts whose first pass switched the wave to the long warm-up.
                        tests/test_gpu_tb_paths.py compares all eight with tests/tbdirect.py's models. */
__device__ unsigned long long g_diag_spec[8];
#define SPEC_COUNT(i) do { if (lane == 0) atomicAdd(&g_diag_spec[i], 1ull); } while (0)
#define SPEC_COUNT_N(i, n) do { if (lane == 0) atomicAdd(&g_diag_spec[i], (unsigned long long)(n)); } while (0)
#else
#define SPEC_COUNT(i) do { } while (0)
#endif

// LDS byte offset, inside a 512-byte decision block, of the (acc1, acc0) pair of ACS lane `lane`:
// [pair][31 - l][1 - n] - the register with n = 1 first.  Every store of a block uses it.
DEV u32 dec_slot(u32 lane) { return acs_pair(lane) * 256u + (31u - acs_l5(lane)) * 8u; }

// One step back for every active lane.  JJ = 3 + j is the position of lane bit j inside P.
//   x     = (t - 16*slot0) << 5: bits 9.. select the block, bits 5..8 are t & 15
//   PC    = P | pair << 8 | half << 1: with the mirrored block layout the 16 history bits of (frame, l, n)
//           for block t >> 4 are the halfword at (x & ~511) | PC
//   kb    = bit t & 15 of it (= NOT decision);   P: bit JJ := kb, bit 2 := old bit JJ
template <int JJ>
DEV void tb_step(u32& PC, u32& kb, u32 x) {
    // x already carries the LDS address of dec (a multiple of 512, checked in traceback_part): no add left here
    const u32 w = *reinterpret_cast<const __attribute__((address_space(3))) unsigned short*>((x & ~511u) | PC);
    kb = __builtin_amdgcn_ubfe(w, (x >> 5) & 15u, 1u);
    const u32 t = ((PC >> (JJ - 2)) & 4u) | (kb << JJ);
    PC = bfi((1u << JJ) | 4u, t, PC);
}

// Runs block-relative indices i = i_from .. i_to (downwards; i_from + 1 and i_to are multiples of 5
// so that the phase of every unrolled position is static: j(i) = (j0 - i) mod 5, JA = j(i_from)).
// Lanes take part while `on` and i <= i_start.  RECORD: collect kb bits of index i into words
// (bit i&31 of word i>>5), flushed to scratch when a word is complete.  xbase = x of index 0.
template <bool RECORD, int JA>
DEV void tb_loop(u32& PC, u32* scratch, int i_from, int i_to, bool on, u32 i_start, u32 xbase) {
    u32 cur = 0;
    for (int i = i_from; i >= i_to; i -= 5) {
#define TB_ONE(K)                                                                  \
    {                                                                              \
        const int ii = i - (K);                                                    \
        u32 kb = 0;                                                                \
        if (on && (u32)ii <= i_start) tb_step<3 + (JA + (K)) % 5>(PC, kb, xbase + ((u32)ii << 5)); \
        if (RECORD) {                                                              \
            cur |= kb << (ii & 31);                                                \
            if ((ii & 31) == 0) {                                                  \
                if (on) scratch[ii >> 5] = cur;                                    \
                cur = 0;                                                           \
            }                                                                      \
        }                                                                          \
    }
        TB_ONE(0) TB_ONE(1) TB_ONE(2) TB_ONE(3) TB_ONE(4)
#undef TB_ONE
    }
}
template <bool RECORD>
DEV void tb_run(u32& PC, u32* scratch, int i_from, int i_to, bool on, u32 i_start, u32 xbase, u32 j0) {
    // i_from % 5 == 4  ->  j(i_from) = (j0 - 4) mod 5 = (j0 + 1) % 5
    switch ((j0 + 1u) % 5u) {
        case 0: tb_loop<RECORD, 0>(PC, scratch, i_from, i_to, on, i_start, xbase); break;
        case 1: tb_loop<RECORD, 1>(PC, scratch, i_from, i_to, on, i_start, xbase); break;
        case 2: tb_loop<RECORD, 2>(PC, scratch, i_from, i_to, on, i_start, xbase); break;
        case 3: tb_loop<RECORD, 3>(PC, scratch, i_from, i_to, on, i_start, xbase); break;
        default: tb_loop<RECORD, 4>(PC, scratch, i_from, i_to, on, i_start, xbase); break;
    }
}

// One traceback part over steps [ts, te) of every frame (te per lane's frame, te_max uniform),
// decisions of block b at dec + (b - slot0)*512.  Lane = (frame fi = lane>>4, block q = lane&15)
// takes the BL steps from ts + q*BL.  A block whose warm-up reaches the frame's last step of the
// part starts from the true position P_top; the others start TB_WARM steps early from state 0,
// which merges with the true path with high probability.  Afterwards every speculative block is
// checked against the block above it and re-traced until nothing changes, so the result is
// exactly the serial chainback.  ORs the decoded bits into img; returns P after step ts.
DEV u32 traceback_part(const char* dec, u32* scratch, u32* img, u32 fstride, u32 lane, u32 ts, u32 te, u32 te_max, u32 slot0,
                       u32 P_top, u32& warm, u32 dmask = 0xFFFFFFFFu) {
    const u32 fi = lane >> 4, q = lane & 15u;
    const u32 span = te_max > ts ? te_max - ts : 0u;
    if (span == 0) return P_top;
    const u32 BL = 5u * ((span + 79u) / 80u);  // 16*BL >= span, multiple of the phase period 5
    const u32 tbase = ts + q * BL;
    const bool has_work = tbase < te;
    const u32 i_last = has_work ? te - 1u - tbase : 0u;  // block-relative index of the frame's last step here
    const u32 q_top = te > ts ? (te - 1u - ts) / BL : 0u;
    const u32 i_warm = BL - 1u + warm;
    const u32 i_start = i_last < i_warm ? i_last : i_warm;
    const bool fixed = has_work && i_last <= i_warm;  // starts from the true position: never re-traced
    // PC = P | C: the lane's constant address bits (pair, half) ride along in the tracked position
    const u32 C = (fi >> 1) * 256u + (fi & 1u) * 2u;
    // x of block-relative index 0 (every t traced is >= 16*slot0), with the LDS address of `dec` folded in: the
    // block select is (x & ~511), so that address must be a multiple of 512 (it is 0: dynamic LDS, no static LDS)
    const u32 dbase = (u32)(uintptr_t)(const __attribute__((address_space(3))) char*)dec;
    if (dbase & 511u) __builtin_trap();
    const u32 xbase = ((tbase - slot0 * 16u) << 5) + dbase;
    const u32 j0 = (4u + 5u - ((ts + 5u - 1u) % 5u)) % 5u;  // j of block-relative index 0: 4 - ((ts-1) mod 5)
    const u32 PC_top = P_top | C;

    u32 P = fixed ? PC_top : (P_ZERO | C), P_out = PC_top;
    // pass 0: warm-up (no bits kept) then the block itself
    tb_run<false>(P, scratch, (int)i_warm, (int)BL, has_work, i_start, xbase, j0);
    u32 P_in = P;  // position the trace passed through at the block's top (meaningless for short top blocks)
    tb_run<true>(P, scratch, (int)BL - 1, 0, has_work, i_start, xbase, j0);
    if (has_work) P_out = P;
    for (int pass = 0; pass < 17; pass++) {
        const u32 nxt = __shfl_down(P_out, 1);  // the block above belongs to the same frame: same C
        const u32 new_in = (q < q_top) ? nxt : PC_top;
        const bool changed = has_work && !fixed && new_in != P_in;
        const unsigned long long miss = __ballot(changed);
        if (miss == 0) break;
#ifdef VIT_DIAG_SPEC
        if (pass == 0 && warm == TB_WARM && (u32)__popcll(miss) >= TB_HARD_MISSES) SPEC_COUNT(7);
#endif
        if (pass == 0 && warm == TB_WARM && (u32)__popcll(miss) >= TB_HARD_MISSES) warm = TB_WARM_HARD;  // for the parts that follow
        if (changed) P_in = new_in;
        P = new_in;
        tb_run<true>(P, scratch, (int)BL - 1, 0, changed, BL - 1u, xbase, j0);
        if (changed) P_out = P;
    }
    // decoded bit index of step t is t - 6 (chainback skips the 6 tail decisions); decoded bit = NOT stored bit
    if (has_work) {
        const u32 nvalid = i_last + 1u < BL ? i_last + 1u : BL;
        const u32 nw = (BL + 31u) >> 5;
        for (u32 w = 0; w < nw; w++) {
            const u32 lo = 32u * w;
            const u32 cnt = nvalid > lo ? nvalid - lo : 0u;
            const u32 mask = cnt >= 32u ? 0xFFFFFFFFu : ((1u << cnt) - 1u);
            const u32 val = ~scratch[w] & mask;
            const u32 b0 = tbase - VIT_TAIL + lo;
            const u32 d = b0 >> 5, sft = b0 & 31u;
            if (val) {
                atomicOr(&img[fi * fstride + (d & dmask)], val << sft);  // dmask: the long-frame kernel's image is a ring
                if (sft) atomicOr(&img[fi * fstride + ((d + 1u) & dmask)], val >> (32u - sft));
            }
        }
    }
    return __shfl(P_out, (int)(fi * 16u)) & 0xFCu;  // block 0 of the frame ends at step ts; C stripped
}

// ---- traceback, fast form: blocks of 16 steps, straight-line code (round 3) ---------------------------------------------
// For a wave whose four frames have the SAME length, a multiple of 16 bits (every DAB size: the FIC's 768, 96*m), the parts
// are cut top-down, 256 steps each (the lowest one may be shorter, a multiple of 16): part = [lo, lo + 16*nl), lo = 6 mod
// 16, lane (frame, q) takes the 16 steps from lo + 16q.  Then
//   * every lane's block-relative index ii has the same bit position (6 + ii) & 15 in its history word and crosses a
//     16-step history block at the same ii: the bit position is an immediate of v_bfe, the block an immediate offset of
//     the ds_read, and there is no address arithmetic left but ONE v_or;
//   * which lanes take part changes at two fixed points only (the two top lanes of a part start late, from the true
//     position): three straight-line segments under one exec mask each instead of a compare + exec save/restore per step;
//   * a lane's 16 decoded bits are one halfword of the image: a plain ds_write_b16, no scratch words, no atomics.
// What is NOT uniform any more is the phase of the lane <-> state map (16 is not a multiple of its period 5): the shift,
// the bit number and the v_bfi mask of a step come from five per-lane register triples indexed by ii mod 5 (static).
// A step back is 5 VALU instructions and 18.9 issue cycles (v_bfe, v_lshrrev, v_and, v_lshl_or, v_bfi; the tracked value is
// the LDS address itself) instead of 9 and 37, and a part is 16 + 30 steps instead of 20 + 30.  Same fixed point, same re-trace rule: exactly ChainBack.
struct Tb16 {
    u32 sh[5], jj[5], mk[5];  // by ii mod 5: JJ - 2, JJ, (1 << JJ) | 4 with JJ = 7 - ((t - 1) mod 5), t = tbase + ii
};
DEV Tb16 tb16_lane(u32 tbase) {  // tbase = the first step of the lane's block
    Tb16 L;
    const u32 c = (tbase + 4u) % 5u;  // (tbase - 1) mod 5
#pragma unroll
    for (int r = 0; r < 5; r++) {
        const u32 e = (c + r) % 5u, JJ = 7u - e;
        L.sh[r] = JJ - 2u;
        L.jj[r] = JJ;
        L.mk[r] = (1u << JJ) | 4u;
    }
    return L;
}
// the triples of a block that starts s steps (mod 5) lower: (tbase - s - 1 + r) mod 5 = (tbase - 1 + (r - s)) mod 5
template <u32 S>
DEV Tb16 tb16_rotate(const Tb16& a) {
    Tb16 L;
#pragma unroll
    for (int r = 0; r < 5; r++) {
        const int k = (r + 5 - (int)(S % 5u)) % 5;
        L.sh[r] = a.sh[k];
        L.jj[r] = a.jj[k];
        L.mk[r] = a.mk[k];
    }
    return L;
}
DEV u32 bfi_v(u32 mask, u32 a, u32 b) {
    u32 d;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(d) : "v"(mask), "v"(a), "v"(b));
    return d;
}
// PC carries the lane's block base (a multiple of 512, bits 9 and up, which the v_bfi never touches): it IS the LDS address.
template <int II, bool REC>
DEV void tb16_step(u32& PC, u32& cur, const Tb16& L) {
    constexpr int r = II % 5, blk = (6 + II) >> 4, idx = (6 + II) & 15;
    const u32 w = *reinterpret_cast<const __attribute__((address_space(3))) unsigned short*>(PC + (u32)(blk * DEC_BLOCK));
    // asm: left to itself hipcc narrows the extract of a zero-extended halfword to v_lshrrev_b16 + v_and 1 + v_and 0xffff
    u32 kb;
    asm("v_bfe_u32 %0, %1, %2, 1" : "=v"(kb) : "v"(w), "n"(idx));
    const u32 m = (PC >> L.sh[r]) & 4u;
    const u32 t = (kb << L.jj[r]) | m;
    PC = bfi_v(L.mk[r], t, PC);
    if constexpr (REC) cur |= kb << II;
}
template <int IFROM, int ITO, bool REC>
struct Tb16Run {
    static DEV void run(u32& PC, u32& cur, const Tb16& L) {
        tb16_step<IFROM, REC>(PC, cur, L);
        if constexpr (IFROM > ITO) Tb16Run<IFROM - 1, ITO, REC>::run(PC, cur, L);
    }
};
// One part [lo, lo + 16*nl) of four equally long frames; decisions of block b at dec + (b - slot0)*512.  Returns P after step lo.
// SPEC (round 4, the long-frame kernel's in-flight parts): the position at the part's top is not known yet.  Every lane - the
// two top ones too - then starts 30 steps above its block from state 0 (the three history blocks above the part must be in LDS),
// the top lane is trusted, and *p_spec receives the position it passed through at the part's top: the part's output is final iff
// that equals what the part above ends in, which the caller checks once the frame's last part has been traced from the true end
// state.  *misses = speculative blocks of the wave that missed in the first pass.  TOMEM (gout = per lane: its frame's output):
// the lane's 16 decoded bits go straight to memory as two MSB-first bytes (deconvolve.cpp:432-433) instead of into the LDS image.
// GEO (the fixed-geometry kernel, vit_pk_fixed_kernel): lo, nl and slot0 are compile-time constants of the caller, which also
// hands in the five per-lane triples (*geo: they only rotate from part to part) and has checked the LDS layout statically.
template <bool SPEC = false, bool TOMEM = false, bool GEO = false>
DEV u32 traceback_part16(const char* dec, u32* img, u32 fstride, u32 lane, u32 lo, u32 nl, u32 slot0, u32 P_top, u32 dmask,
                         uint8_t* gout = nullptr, u32* p_spec = nullptr, u32* misses = nullptr, const Tb16* geo = nullptr) {
    constexpr int W = 30;  // warm-up; with 16-step blocks the chain of a speculative lane starts at ii = 45
    const u32 fi = lane >> 4, q = lane & 15u;
    const u32 tbase = lo + q * 16u;
    const bool has_work = q < nl;
    const u32 above = SPEC ? 3u : nl - q;  // blocks from this one up to the top of the part (has_work: >= 1)
    const bool fixed = has_work && above <= 2u;  // its warm-up would cross the part's top: it starts there, from the true position
    const u32 C = (fi >> 1) * 256u + (fi & 1u) * 2u;
    const u32 dbase = (u32)(uintptr_t)(const __attribute__((address_space(3))) char*)dec;
    if constexpr (!GEO) {
        if (dbase & 511u) __builtin_trap();
    }
    const u32 bbq = dbase + ((lo >> 4) - slot0 + q) * DEC_BLOCK;
    Tb16 L;
    if constexpr (GEO) {
        L = *geo;
    } else {  // (= tb16_lane(tbase), written out: through the helper the general kernels' set-up code comes out in another order)
        const u32 c = (tbase + 4u) % 5u;  // (tbase - 1) mod 5
#pragma unroll
        for (int r = 0; r < 5; r++) {
            const u32 e = (c + r) % 5u, JJ = 7u - e;
            L.sh[r] = JJ - 2u;
            L.jj[r] = JJ;
            L.mk[r] = (1u << JJ) | 4u;
        }
    }
    // positions travel between lanes without the block base (P & 0x1FF); a lane adds its own
    const u32 PC_top = P_top | C;
    u32 P = (fixed ? PC_top : (P_ZERO | C)) | bbq, P_out = PC_top, cur = 0;
    if (has_work && above >= 3u) Tb16Run<15 + W, 32, false>::run(P, cur, L);
    if (has_work && above >= 2u) Tb16Run<31, 16, false>::run(P, cur, L);
    u32 P_in = P & 0x1FFu;
    if (has_work) {
        Tb16Run<15, 0, true>::run(P, cur, L);
        P_out = P & 0x1FFu;
    }
    for (int pass = 0; pass < 17; pass++) {
        // the block above = the next lane of the same 16-lane row: one DPP move (row_shl:1), no LDS round trip in the pass loop
        const u32 nxt = (u32)__builtin_amdgcn_update_dpp(0, (int)P_out, 0x101, 0xF, 0xF, true);
        const u32 new_in = (q + 1u < nl) ? nxt : (SPEC ? P_in : PC_top);
        const bool changed = has_work && !fixed && new_in != P_in;
        if constexpr (SPEC) {
            const unsigned long long miss = __ballot(changed);
            if (pass == 0) *misses = (u32)__popcll(miss);
            if (miss == 0) break;
        } else {
#ifdef VIT_DIAG_SPEC
            {
                const unsigned long long miss = __ballot(changed);
                if (pass == 0) SPEC_COUNT_N(5, __popcll(miss));
                if (miss) SPEC_COUNT(6);
            }
#endif
            if (!__any(changed)) break;
        }
        if (changed) {
            P_in = new_in;
            P = new_in | bbq;
            cur = 0;
            Tb16Run<15, 0, true>::run(P, cur, L);
            P_out = P & 0x1FFu;
        }
    }
    // decoded bit index of step t is t - 6 (a multiple of 16 here); decoded bit = NOT stored bit
    if (has_work) {
        const u32 h = (tbase - VIT_TAIL) >> 4;  // halfword index in the frame's bit image
        if constexpr (TOMEM) {
            const u32 v = __builtin_bitreverse32(~cur & 0xFFFFu);  // byte 3 = bits 0..7 reversed, byte 2 = bits 8..15 reversed
            gout[2u * h] = (uint8_t)(v >> 24);
            gout[2u * h + 1u] = (uint8_t)(v >> 16);
        } else {
            reinterpret_cast<unsigned short*>(img + fi * fstride)[((h >> 1) & dmask) * 2u + (h & 1u)] = (unsigned short)~cur;
        }
    }
    if constexpr (SPEC) *p_spec = __shfl(P_in, (int)(fi * 16u + nl - 1u)) & 0xFCu;  // the top lane's position at the part's top
    return __shfl(P_out, (int)(fi * 16u)) & 0xFCu;
}

}  // namespace
