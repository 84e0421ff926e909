// vit_pk_acs.h -- what the forward pass of the packed kernels (vit_pk.hip, 4 frames per wavefront) shares: sizes, the per-lane table
// addresses, the lane exchange and the ACS step, the block bodies, the LDS layout of a segment, the issue-priority helpers.
#pragma once
#include "vit_internal.h"
#include "vit_pk_dev.h"

namespace {

constexpr int TAB_BYTES = 2048;  // 32 steps x 2 pairs x 8 triples x M (4 B); 63-M is one v_sub in the ACS
constexpr int DEC_BLOCK = 512;   // 16 steps of decisions: 64 lanes x 8 B
constexpr unsigned PK_SPLIT_DEN = 8;  // a sorted table is split between the kernels when < 1/8 of its frames are long

// One set of table ADDRESSES per table half (even / odd block), the half chosen by a uniform branch: no address add in front of
// the table reads (5 per block; 0.4363 -> 0.4306 ms, profiles/r03_ab_tabs.txt).
struct Lanes {
    u32 toff[5];  // LDS address of this lane's M entry for phase rho, in the table half the block reads
};

// ACS lane roles: lane bits 0..4 carry the butterfly index (l5), lane bit 5 the pair.
DEV u32 acs_l5(u32 lane) { return lane & 31u; }
DEV u32 acs_pair(u32 lane) { return lane >> 5; }
// toff by lane, tabulated at compile time (80 VALU instructions per wave as arithmetic; two loads that are back long before the
// first table read).  Butterfly index of ACS lane l5 at phase rho = rol5(l5, rho); its class = parity((2i) & poly_j), const.asm:27-63.
struct alignas(32) ToffTable {  // load_toff reads a row with one 16-byte load
    u32 v[64][8];  // [lane][rho], rows padded to 32 bytes
};
constexpr ToffTable make_toff_table() {
    ToffTable t{};
    for (u32 lane = 0; lane < 64; lane++) {
        const u32 l5 = lane & 31u, pair = lane >> 5;
        for (u32 rho = 0; rho < 5; rho++) {
            const u32 i = ((l5 << rho) | (l5 >> (5 - rho))) & 31u;
            const u32 i0 = i & 1u, i1 = (i >> 1) & 1u, i2 = (i >> 2) & 1u, i3 = (i >> 3) & 1u, i4 = (i >> 4) & 1u;
            const u32 c = (i1 ^ i2 ^ i4) | ((i0 ^ i1 ^ i2) << 1) | ((i0 ^ i3) << 2);
            t.v[lane][rho] = pair * 32u + c * 4u;
        }
    }
    return t;
}
__constant__ ToffTable g_toff = make_toff_table();
DEV void load_toff(Lanes& L, u32 lane) {
    const uint4 a = *reinterpret_cast<const uint4*>(&g_toff.v[lane][0]);
    L.toff[0] = a.x;
    L.toff[1] = a.y;
    L.toff[2] = a.z;
    L.toff[3] = a.w;
    L.toff[4] = g_toff.v[lane][4];
}
// lane-bit <-> register-bit transpose on lane bit J: afterwards A holds the s5=0
// member and B the s5=1 member of the next butterfly.
//   A = bit_J(lane) ? N1[lane ^ 2^J] : N0        B = bit_J(lane) ? N1 : N0[lane ^ 2^J]
// J = 4: v_permlane16_swap.  J < 4: two v_cndmask_b32_dpp (DPP on src0, select by VCC);
// `s_nop 1` covers the VALU-write -> DPP-read hazard of N0/N1, which hipcc cannot see
// inside an asm statement.
// Issue cost on gfx950 (profiles/r01_valu_issue_rates_ubench.txt): every v_pk_*, VOP3 three-operand,
// DPP and v_cmp instruction holds the SIMD for 4 cycles per wave, v_permlane*_swap for 8, and
// v_cndmask_b32 through VCC for ~22.  So for J < 4 the partner values travel through the LDS
// crossbar (ds_swizzle: no VALU slot, no LDS memory) and two v_cndmask_b32_e64 pick them up.
// Lane bit 3 goes through ds_swizzle too and lane bit 2 through masked DPP moves: since the round-2 traceback the kernel sits
// between the VALU and the LDS limit - none of the two swizzled 0.467 ms, bit 3 only 0.458, bit 2 only 0.459, both 0.462
// (profiles/r02_ab_k3_swz.txt).
template <int J>  // J = lane bit (bit J of l5)
DEV void exchange(u32& A, u32& B, u32 N0, u32 N1, u32 lane) {
    if constexpr (J == 4) {
        // swap N0's odd rows with N1's even rows (rows = 16 lanes)
        auto r = __builtin_amdgcn_permlane16_swap(N0, N1, false, false);
        A = r[0];
        B = r[1];
    } else if constexpr (J == 2) {
        // masked DPP moves stay in the VALU (10 cycles incl. one copy) and keep LDS latency off this step
        A = __builtin_amdgcn_update_dpp(N0, N1, 0x114 /*row_shr:4*/, 0xF, 0xA, false);
        B = __builtin_amdgcn_update_dpp(N1, N0, 0x104 /*row_shl:4*/, 0xF, 0x5, false);
    } else {
        // lane bits 0/1 cannot be masked by DPP bank masks (and DPP needs the source lane active)
        const bool hi = (lane >> J) & 1u;
        // partner values through ds_swizzle (LDS crossbar, no VALU slot): 8 VALU cycles for the selects
        constexpr int pat = 0x1F | ((1 << J) << 10);  // BitMode: src lane = lane ^ 2^J within 32
        const u32 p1 = (u32)__builtin_amdgcn_ds_swizzle((int)N1, pat);
        const u32 p0 = (u32)__builtin_amdgcn_ds_swizzle((int)N0, pat);
        A = hi ? p1 : N0;
        B = hi ? N1 : p0;
    }
}

// One trellis step for 4 frames (deconvolve.cpp:352-374 in packed u16 form).
template <int RHO, int J, bool HIST>
DEV void acs_step(u32& A, u32& B, u32& acc0, u32& acc1, u32 mt, u32 lane, const Consts& C) {
    constexpr bool ODD = (J & 1) != 0;
    // 63 - M per half as ONE 32-bit subtract.  Odd steps: M <= 63, no borrow.  Even steps carry the
    // +0xFF00 bias: (0xFE3F - M') mod 2^16 per half; the low half always borrows, hence 0xFE40 on top.
    const us2 a = U(A), b = U(B), M = U(mt), MM = U((ODD ? 0x003F003Fu : 0xFE40FE3Fu) - mt);
    const us2 m0 = __builtin_elementwise_add_sat(a, M), m1 = __builtin_elementwise_add_sat(b, MM);
    const us2 m2 = __builtin_elementwise_add_sat(a, MM), m3 = __builtin_elementwise_add_sat(b, M);
    us2 n0 = __builtin_elementwise_min(m0, m1), n1 = __builtin_elementwise_min(m2, m3);
    // sign(m0-m1) = 1  <=>  m0 < m1  <=>  decision bit 0 (tie -> decision 1)
    if constexpr (HIST) {
        const us2 x01 = m0 - m1, x23 = m2 - m3;
        // history: both metrics carry the same bias and lie in one 256-wide range, so m0 - m1 is in
        // [-255, 255] (0xFF01 .. 0x00FF) and bits 8..15 of each half of the difference are EIGHT
        // copies of its sign: one v_bfi can drop the decision at any of those positions.
        // Step j of the block ends up at bit j of its half with ONE 32-bit shift per 16 steps:
        //   steps 0..7 -> bits 8..15 | >>8 | steps 8..15 -> bits 8..15
        // (what the shift carries from the upper half into bits 8..15 of the lower one is overwritten
        // by the eight inserts that follow it; the stale bits of the previous block are overwritten by
        // the first eight inserts or shifted out).
        constexpr int pos = 8 + (J & 7);
        constexpr u32 mask = 0x00010001u << pos;
        if constexpr (J == 8) {
            acc0 >>= 8;
            acc1 >>= 8;
        }
        acc0 = bfi(mask, W(x01), acc0);
        acc1 = bfi(mask, W(x23), acc1);
    }
    if constexpr (ODD) {
        // Renormalize256: state 0 (lane 0 of the pair, register N0) > 150 (or >= 150, the MASM decoders' test) ->
        // psubusb 63.  z = m + 0xFF00 per half.  z + 0x8069 has bit 15 set iff m >= 151; done as ONE 32-bit add:
        // the low half always carries out (0xFF00 + 0x8069 >= 2^16), so the high constant is 0x8068 (C.rc).
        // The subtrahend is per frame, i.e. the same for every lane and both registers of a pair, so it
        // commutes with the lane exchange: the broadcast and the exchange are issued together and
        // the subtraction lands on the exchanged registers (one LDS latency instead of two in a row).
        const u32 z = (u32)__builtin_amdgcn_ds_swizzle((int)W(n0), 0);  // lane 0 of each 32-lane group
        exchange<4 - RHO>(A, B, W(n0), W(n1), lane);
        // The subtrahend 0xFF00 + {0,63} per half in three instructions: v_add_u32 (2.7 cycles; bit 15 of each half := m >= 151),
        // v_pk_ashrrev_i16 15, v_and_or_b32 - 0.8 % on the headline batch and 1-2 % on config 3 against add, shift, and,
        // multiply-add (profiles/r03_ab_swz_k3.txt)
        u32 K;
        {
            const u32 w = z + C.rc;
            asm("v_pk_ashrrev_i16 %0, 15, %1 op_sel_hi:[0,1]\n\t"
                "v_and_or_b32 %0, %0, %2, %3"
                : "=&v"(K)
                : "v"(w), "s"(0x003F003Fu), "v"(C.hi));
        }
        A = W(__builtin_elementwise_sub_sat(U(A), U(K)));  // -> 0-based representation
        B = W(__builtin_elementwise_sub_sat(U(B), U(K)));
    } else {
        exchange<4 - RHO>(A, B, W(n0), W(n1), lane);
    }
}

template <int V, int J, int JEND, bool HIST>
struct Steps {
    static DEV void run(u32& A, u32& B, u32& acc0, u32& acc1, const char* tab, const Lanes& L, u32 lane,
                        const Consts& C) {
        constexpr int RHO = (V + J) % 5;
        // L.toff holds LDS addresses of the table half this block reads: no address arithmetic left in the loop
        const u32 mt = *reinterpret_cast<const __attribute__((address_space(3))) u32*>(L.toff[RHO] + (u32)(J * 64));
        acs_step<RHO, J, HIST>(A, B, acc0, acc1, mt, lane, C);
        Steps<V, J + 1, JEND, HIST>::run(A, B, acc0, acc1, tab, L, lane, C);
    }
};
template <int V, int JEND, bool HIST>
struct Steps<V, JEND, JEND, HIST> {
    static DEV void run(u32&, u32&, u32&, u32&, const char*, const Lanes&, u32, const Consts&) {}
};
template <bool HIST, int N = 16>
DEV void steps16(u32 v, u32& A, u32& B, u32& acc0, u32& acc1, const char* th, const Lanes& L, u32 lane, const Consts& C) {
    switch (v) {
        case 0: Steps<0, 0, N, HIST>::run(A, B, acc0, acc1, th, L, lane, C); break;
        case 1: Steps<1, 0, N, HIST>::run(A, B, acc0, acc1, th, L, lane, C); break;
        case 2: Steps<2, 0, N, HIST>::run(A, B, acc0, acc1, th, L, lane, C); break;
        case 3: Steps<3, 0, N, HIST>::run(A, B, acc0, acc1, th, L, lane, C); break;
        default: Steps<4, 0, N, HIST>::run(A, B, acc0, acc1, th, L, lane, C); break;
    }
}
// Last block of a frame whose step count is 6 mod 16 - every DAB size (framebits = 96*m, and the FIC's
// 768): the ten padding steps are not computed.  After six steps the history sits at bits 8..13 of
// each half (see acs_step); one more shift puts step j at bit j like in a full block.
DEV void steps6(u32 v, u32& A, u32& B, u32& acc0, u32& acc1, const char* th, const Lanes& L, u32 lane, const Consts& C) {
    steps16<true, 6>(v, A, B, acc0, acc1, th, L, lane, C);
    acc0 >>= 8;
    acc1 >>= 8;
}

typedef u32 v32u __attribute__((ext_vector_type(32)));
constexpr u32 VREG_BLOCKS = 32;  // decision blocks that can stay in VGPRs (2 x 32 dwords)

constexpr u32 DUMP_GROUP = 16;   // register blocks are dumped to LDS 16 at a time
constexpr u32 SEG_BLOCKS = VREG_BLOCKS + DUMP_GROUP + 1u;  // 49 blocks = 784 steps: one FIC frame

// Decision history of ONE SEGMENT (<= 49 blocks).  Blocks [0,R) of the segment stay in VGPRs, the
// other nb - R in LDS: Ld of them in the `dec` region, the LAST one where the (by then dead)
// branch-metric table starts, right behind dec - so a FIC frame needs 16 x 512 + 2048 = 10 KB of
// LDS and 16 waves fit a CU.
//   nb <= 17 : R = 0,                Ld = nb - 1
//   else     : R = min(32, nb - 17), Ld = nb - R - 1  (>= 16 = one dump group)
// Frames longer than a segment take vit_pk_long_kernel below (blocks beyond the last 17 go through HBM).
__host__ __device__ constexpr inline u32 pk_reg_blocks(u32 nb) {
    if (nb <= DUMP_GROUP + 1u) return 0;
    const u32 r = nb - (DUMP_GROUP + 1u);
    return r < VREG_BLOCKS ? r : VREG_BLOCKS;
}
__host__ __device__ constexpr inline u32 pk_img_stride(u32 maxfb) { return ((maxfb + 31u) >> 5) + 2u; }  // dwords per frame
__host__ __device__ constexpr inline u32 pk_scratch_words(u32 maxfb) {
    // words per lane of traceback bit scratch: the longest part is a segment's LDS tail (<= 17 blocks)
    // or a 256-step register group -> BL <= 20 for full segments; short frames are all "tail"
    u32 nblk = (maxfb + VIT_TAIL + 15u) >> 4;
    if (nblk > SEG_BLOCKS) nblk = SEG_BLOCKS;
    const u32 tail = (nblk - pk_reg_blocks(nblk)) * 16u;
    const u32 span = tail > 256u ? tail : 256u;
    const u32 bl = 5u * ((span + 79u) / 80u);
    return (bl + 31u) >> 5;
}
struct PkLayout {
    u32 dec_bytes;  // tab starts here
    u32 img_off;    // output bit image
    u32 total;
    u32 maxfb;      // the framebits this layout was sized for
};
__host__ __device__ constexpr inline PkLayout pk_layout(u32 maxfb) {  // single-segment kernel (nblk <= 49)
    const u32 nb = (maxfb + VIT_TAIL + 15u) >> 4;
    PkLayout l{};
    l.maxfb = maxfb;
    l.dec_bytes = (nb - pk_reg_blocks(nb) - 1u) * DEC_BLOCK;
    const u32 scratch = 64u * 4u * pk_scratch_words(maxfb), img = 16u * pk_img_stride(maxfb);
    u32 tabregion = DEC_BLOCK + scratch + img;  // the image lives in the dead table region too
    tabregion = tabregion > (u32)TAB_BYTES ? ((tabregion + 15u) & ~15u) : (u32)TAB_BYTES;
    l.img_off = l.dec_bytes + DEC_BLOCK + scratch;
    l.total = l.dec_bytes + tabregion;
    return l;
}

// ---- issue priority, hardware slot, timeline diagnostic ---------------------------------------------------------------------------
// s_setprio takes an immediate: a wave-uniform level is a scalar branch over the four instructions
DEV void set_prio(u32 level) {
    switch (level) {
        case 0: __builtin_amdgcn_s_setprio(0); break;
        case 1: __builtin_amdgcn_s_setprio(1); break;
        case 2: __builtin_amdgcn_s_setprio(2); break;
        default: __builtin_amdgcn_s_setprio(3); break;
    }
}
// Static issue priority by wave slot within the SIMD.  ONE wave of the four at low priority, three equal: four distinct levels starve
// the lowest (a wave then takes 63 ... 248 us) and the launch drains for ~50 us; this map is 1.3 % faster at 3 dB and 4 % on input
// without signal (profiles/r03_ab_priomap.txt).  Static priorities as such: ~1 % on the 65536-frame batch.
constexpr u32 prio_map(u32 slot) { return slot == 0u ? 0u : 1u; }
DEV u32 hw_id() {
    u32 hwid;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
    return hwid;
}
#ifdef VIT_DIAG_TIMES
// Timeline diagnostic (tools/exp/timeline.py, long_phases.py), one record per group of four frames: start, start of the traceback,
// end (= now) and the hardware slot (the long-frame kernel writes its own fourth word: the time spent in in-flight parts).
__device__ unsigned long long g_diag_times[16384 * 4];
DEV void diag_times_put(u32 lane, u32 group, unsigned long long t0, unsigned long long t1) {
    if (lane == 0 && group < 16384u) {
        const u32 hwid = hw_id();
        g_diag_times[group * 4u + 0u] = t0;
        g_diag_times[group * 4u + 1u] = t1;
        g_diag_times[group * 4u + 2u] = __builtin_amdgcn_s_memrealtime();
        g_diag_times[group * 4u + 3u] = hwid;
    }
}
#endif

}  // namespace
