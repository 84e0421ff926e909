// vit_pk_fixed.h -- the fixed-geometry instantiation of the packed kernel (a uniform batch of FIC frames).
#pragma once
#include "vit_pk_acs.h"
#include "vit_pk_tb.h"

namespace {

// ---- fixed geometry: a uniform batch of frames of ONE length known at compile time (the FIC's 768 bits) ------------------------
// vit_pk_kernel pays for what such a launch never uses: four possibly different frames per wave (descriptor or uniform branch,
// 64-bit offsets, validity checks, per-lane selects), run-time block geometry (register or LDS history per block, a predicate
// on every symbol prefetch), the set-up of every traceback part (tbase mod 5, fifteen per-lane values, three times), a window
// move with run-time bounds, and the general traceback form, whose 25 spilled VGPRs make every wave a scratch-using wave.  Here
// the frame length FB is a template parameter: frame addresses are scalar arithmetic on blockIdx.x, the block loop is cut where
// the history moves from registers to LDS, the traceback parts and the window moves have constant bounds, and only the fast
// traceback form is compiled in (no private segment).  Same arithmetic, same traceback fixed point: the same bytes.
// Another uniform length (FB = 32*m <= 768) is one more instantiation plus its line in vit_launch_pk.
#ifndef VIT_FIC_FIXED
#define VIT_FIC_FIXED 1  /* 0: the library without the fixed-geometry instantiation (A/B runs; the general path at 768 bits) */
#endif
template <u32 FB>
struct PkFixed {
    static constexpr u32 T = FB + VIT_TAIL;            // trellis steps
    static constexpr u32 NB = (T + 15u) >> 4;          // blocks; the last one has six steps
    static constexpr u32 R = pk_reg_blocks(NB);        // blocks [0,R) keep their history in VGPRs
    static constexpr u32 LD = NB - R - 1u;             // blocks [R, NB-1) go to dec, the last one onto the dead table
    static constexpr u32 TAB_OFF = LD * DEC_BLOCK;
    static constexpr u32 IMG_OFF = TAB_OFF + DEC_BLOCK;  // the image follows the last block (no traceback scratch words here)
    static constexpr u32 FSTRIDE = FB / 32u;           // image dwords per frame: every halfword is written by exactly one lane
    static constexpr u32 LDS_BYTES = TAB_OFF + (u32)TAB_BYTES;
    static constexpr u32 SYM_STEPS = T;                // symbols per frame in memory: 4 per step
    static constexpr u32 OUT_BYTES = FB / 8u;
    static_assert(FB % 32u == 0 && FB >= 32u, "whole image dwords, an even number of 16-step blocks below the last one");
    static_assert((T & 15u) == 6u, "the last block has six steps");
    static_assert(NB <= SEG_BLOCKS && (R & 1u) == 0 && (LD & 1u) == 0 && R + 3u <= NB, "one segment, cut into pairs of blocks");
    static_assert(LD <= DUMP_GROUP, "the traceback window is dec + one block");
    static_assert(IMG_OFF + 16u * FSTRIDE <= LDS_BYTES, "the image fits the dead table region");
    static_assert(TAB_OFF % 512u == 0, "tb16_step selects the block with the address bits above 511");
    static_assert(LDS_BYTES == pk_layout(FB).total, "as many waves per CU as the general kernel");
};

// the parts of the fast traceback, top down: [LO, HI) with the window's slot 0 = block SLOT0; then the window moves down
template <class G, u32 HI, u32 SLOT0>
DEV void fixed_traceback(char* dec, u32* img, u32 lane, u32 dslot, const v32u r0, const v32u r1, u32 P, const Tb16 L) {
    constexpr u32 LO = HI > 256u + VIT_TAIL ? HI - 256u : VIT_TAIL;
    static_assert(LO % 16u == VIT_TAIL && (LO >> 4) >= SLOT0 && (HI >> 4) - SLOT0 <= DUMP_GROUP, "the part lies in the window");
    P = traceback_part16<false, false, true>(dec, img, G::FSTRIDE, lane, LO, (HI - LO) >> 4, SLOT0, P, 0xFFFFFFFFu, nullptr,
                                             nullptr, nullptr, &L);
    if constexpr (LO != VIT_TAIL) {
        // what stays goes D slots up (every lane moves its own 8 bytes of a block), the D register blocks below come in
        constexpr u32 D = SLOT0 < DUMP_GROUP ? SLOT0 : DUMP_GROUP, G0 = SLOT0 - D;
        static_assert(D >= 1u, "there are blocks below this part");
        constexpr u32 LO2 = LO > 256u + VIT_TAIL ? LO - 256u : VIT_TAIL;
        __syncthreads();
#pragma unroll
        for (u32 sl = DUMP_GROUP; sl >= D; sl--)
            *reinterpret_cast<uint2*>(dec + sl * DEC_BLOCK + dslot) = *reinterpret_cast<const uint2*>(dec + (sl - D) * DEC_BLOCK + dslot);
#pragma unroll
        for (u32 b = G0; b < SLOT0; b++)
            *reinterpret_cast<uint2*>(dec + (b - G0) * DEC_BLOCK + dslot) = make_uint2(r1[b], r0[b]);
        __syncthreads();
        fixed_traceback<G, LO, G0>(dec, img, lane, dslot, r0, r1, P, tb16_rotate<LO - LO2>(L));
    }
}

template <u32 FB, bool SYM32, bool ROT>
__global__ __launch_bounds__(64, 4) void vit_pk_fixed_kernel(const uint8_t* __restrict__ sym, uint8_t* __restrict__ out,
                                                              long long nframes, u32 renorm_c) {
    typedef PkFixed<FB> G;
#ifdef VIT_DIAG_TIMES
    const unsigned long long diag_t0 = __builtin_amdgcn_s_memrealtime();
#endif
    __shared__ __attribute__((aligned(512))) char lds[G::LDS_BYTES];
    char* dec = lds;               // [block - R][lane] -> (acc1, acc0); the last block spills into tab
    char* tab = lds + G::TAB_OFF;  // [tau][pair][c] -> M; after the ACS: last block, image
    u32* img = reinterpret_cast<u32*>(lds + G::IMG_OFF);
    const u32 lane = threadIdx.x;
    u32 prio_slot = 0;
    // Static priorities (one wave of a SIMD low, see vit_pk_kernel) only where they rotate.  In a launch of several rounds this
    // kernel runs without any: with them the low-priority wave of a SIMD outlives its neighbours and what is left of it when the
    // dispatcher runs dry finishes alone - a drain of 29 to 48 us whose length swings with a 1 % change of a wave's instruction
    // count, and which cost the no-signal inputs 3-5 % (profiles/r10_fic_isa_ab.txt).
    if constexpr (ROT) {
        prio_slot = hw_id() & 3u;
        set_prio(prio_map(prio_slot));
    }
    // ---- frames: group g = frames 4g .. 4g + 3, each SYM_STEPS x 4 symbols in and OUT_BYTES out.  The launch's last group may
    // have fewer: its missing frames alias the group's first frame (no symbol byte read that belongs to no frame) and their
    // output stores are predicated off (nvalid, wave-uniform)
    constexpr u32 SB = SYM32 ? 4u : 1u, STEP_BYTES = 4u * SB, FRAME_BYTES = G::SYM_STEPS * STEP_BYTES;
    const long long f0 = (long long)blockIdx.x * 4;
    const long long left = nframes - f0;
    const u32 nvalid = left >= 4 ? 4u : (u32)left;
    const uint8_t* gsym = sym + (size_t)f0 * FRAME_BYTES;
    uint8_t* gout = out + (size_t)f0 * G::OUT_BYTES;

    // ---- ACS lane constants ----
    const u32 l5 = acs_l5(lane);
    const u32 dslot = dec_slot(lane);
    Lanes L;
    load_toff(L, lane);
    Lanes L1;
    {
        const u32 tb = (u32)(uintptr_t)(const __attribute__((address_space(3))) char*)tab;
#pragma unroll
        for (int rho = 0; rho < 5; rho++) {
            L.toff[rho] += tb;
            asm volatile("" : "+v"(L.toff[rho]));  // tb is a constant here (static LDS): without this the sum is redone in front of every table read
            L1.toff[rho] = L.toff[rho] + 1024u;
            asm volatile("" : "+v"(L1.toff[rho]));
        }
    }
    Consts C;
    C.hi = HI;
    C.rc = renorm_c;
    asm volatile("" : "+v"(C.hi));
    // ---- pre-pass lane constants: lane = (tau = lane>>1, pair pp = lane&1); frames 2pp (half 0) and 2pp + 1 (half 1) ----
    const u32 tau = lane >> 1, pp = lane & 1u;
    u32 ka = 2u * pp, kb = 2u * pp + 1u;
    if (nvalid < 4u) {
        ka = ka < nvalid ? ka : 0u;
        kb = kb < nvalid ? kb : 0u;
    }
    const u32 a_off = ka * FRAME_BYTES + tau * STEP_BYTES, b_off = kb * FRAME_BYTES + tau * STEP_BYTES;  // from gsym
    typedef typename RawStep<SYM32>::type Raw;
    auto load32 = [&](u32 off, u32 rb) {  // the lane's step of the 32 that start at block rb (rb wave-uniform)
        return *reinterpret_cast<const Raw*>(gsym + (size_t)rb * (16u * STEP_BYTES) + off);
    };
    u32 sel[4];
    {
        const u32 hb = (tau & 1u) ? 0x0C000C00u : 0x0D000D00u;
#pragma unroll
        for (int k = 0; k < 4; k++) sel[k] = hb | (0x00040000u + 0x00010001u * k);
    }
    const PrepassLane PL = prepass_lane(lane);
    u32 A = l5 == 0 ? 0u : 0x003F003Fu, B = 0x003F003Fu;
    u32 acc0 = 0, acc1 = 0;
    v32u r0, r1;

    // ---- ACS over the blocks, two per trip (the pre-pass's 32 steps) ----
    {
        Raw sa = load32(a_off, 0u), sb = load32(b_off, 0u);
        u32 v = 0;
        auto rotate = [&](const u32 rbx) {
            if constexpr (ROT) set_prio((prio_slot + rbx) & 3u);
        };
        auto put_reg = [&](const u32 rbx) {
            u32 i = rbx;
            asm volatile("" : "+s"(i));  // an index of unknown range: with the constant loop bounds in sight the optimiser turns the insert
                                         // into a store through a pointer, and the arrays end up in scratch memory instead of VGPRs
            r0[i] = acc0;  // s_set_gpr_idx_on / v_mov / s_set_gpr_idx_off
            r1[i] = acc1;
        };
        auto put_lds = [&](const u32 rbx) {
            u32 rbs = rbx;
            asm volatile("" : "+s"(rbs));  // the address from the scalar block index (see vit_pk_kernel)
            *reinterpret_cast<uint2*>(dec + (rbs - G::R) * DEC_BLOCK + dslot) = make_uint2(acc1, acc0);
        };
        // one trip: table for blocks rb, rb + 1; the next trip's symbols are in flight meanwhile (all inside the frame)
        auto trip = [&](const u32 rb, auto&& put) {
            u32 rbs = rb;
            asm volatile("" : "+s"(rbs));
            rotate(rb);
            __syncthreads();
            prepass(pack_step(sa), pack_step(sb), tab, PL, sel);
            sa = load32(a_off, rbs + 2u);
            sb = load32(b_off, rbs + 2u);
            __syncthreads();
            steps16<true>(v, A, B, acc0, acc1, tab, L, lane, C);
            put(rb);
            v = v == 4 ? 0 : v + 1;
            rotate(rb + 1u);
            steps16<true>(v, A, B, acc0, acc1, tab, L1, lane, C);
            put(rb + 1u);
            v = v == 4 ? 0 : v + 1;
        };
        // One loop over the register-history pairs and one over the LDS pairs (twenty block bodies, 67 KB of code).  A single loop with the
        // choice per block (ten bodies, 41 KB) is the SLOWER one: 0.4330-0.4343 ms against 0.4122-0.4141 on the benchmark batch, the
        // general kernel 0.4186-0.4205; on input without signal it is the other way round, and the general kernel beats both
        // (profiles/r09_fic_fixed_ab.txt section 3).
        for (u32 rb = 0; rb < G::R; rb += 2u) trip(rb, put_reg);
        for (u32 rb = G::R; rb + 3u < G::NB; rb += 2u) trip(rb, put_lds);
        // the last pair (static phase): of the 32 steps behind it only the last block's six exist
        {
            constexpr u32 rb = G::NB - 3u;
            rotate(rb);
            __syncthreads();
            prepass(pack_step(sa), pack_step(sb), tab, PL, sel);
            sa = sb = Raw{};
            if (tau < G::T - (rb + 2u) * 16u) {  // the lanes beyond the frame's end load nothing
                sa = load32(a_off, rb + 2u);
                sb = load32(b_off, rb + 2u);
            }
            __syncthreads();
            Steps<rb % 5u, 0, 16, true>::run(A, B, acc0, acc1, tab, L, lane, C);
            put_lds(rb);
            rotate(rb + 1u);
            Steps<(rb + 1u) % 5u, 0, 16, true>::run(A, B, acc0, acc1, tab, L1, lane, C);
            put_lds(rb + 1u);
        }
        {
            constexpr u32 rb = G::NB - 1u;
            rotate(rb);
            __syncthreads();
            prepass(pack_step(sa), pack_step(sb), tab, PL, sel);
            __syncthreads();
            Steps<rb % 5u, 0, 6, true>::run(A, B, acc0, acc1, tab, L, lane, C);
            acc0 >>= 8;  // see steps6
            acc1 >>= 8;
            __syncthreads();  // the last block lands on the table: all reads done first
            put_lds(rb);
        }
    }
    __syncthreads();
#ifdef VIT_DIAG_TIMES
    const unsigned long long diag_t1 = __builtin_amdgcn_s_memrealtime();
#endif
    // ---- traceback (fast form only; the image needs no zeroing: every halfword is stored once) ----
    fixed_traceback<G, G::T, G::R>(dec, img, lane, dslot, r0, r1, P_ZERO, tb16_lane((G::T > 256u + VIT_TAIL ? G::T - 256u : VIT_TAIL) + (lane & 15u) * 16u));
    __syncthreads();
#ifdef VIT_DIAG_TIMES
    diag_times_put(threadIdx.x, blockIdx.x, diag_t0, diag_t1);
#endif
    // ---- output: bit b of the image is decoded bit b, bytes are MSB-first; sixteen lanes per frame, dword stores ----
    {
        const u32 k = lane >> 4, j = lane & 15u;
        if (k < nvalid) {
            u32* o = reinterpret_cast<u32*>(gout + k * G::OUT_BYTES);
            const u32* im = img + k * G::FSTRIDE;
#pragma unroll
            for (u32 m0 = 0; m0 < G::FSTRIDE; m0 += 16u)
                if (m0 + 16u <= G::FSTRIDE || j < G::FSTRIDE - m0) o[m0 + j] = __builtin_bswap32(__builtin_bitreverse32(im[m0 + j]));
        }
    }
}

}  // namespace
