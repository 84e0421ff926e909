// vit_pk_long.h -- the packed kernel for frames longer than one segment (persistent workgroups, in-flight traceback, write-only spill).
#pragma once
#include "vit_pk_acs.h"
#include "vit_pk_tb.h"

namespace {

// ---- frames longer than one segment: traced back in flight from a window in LDS; decisions written once to HBM -------------
// (history: round 1 checkpoint + recompute, 1.7x the ACS work; rounds 2-3 one forward pass whose blocks were spilled to HBM and
// read back 16 at a time for a traceback after the forward pass: 8 B per frame-step each way.)
// Round 4: the forward pass writes every block but a frame's last 16 to the workgroup's slice of `spill` (512 B per block,
// coalesced) WITHOUT reading it back, and keeps what a traceback may need next in a window of LDS (see below):
//   * a group of four equally long frames of a multiple of 16 bits (every DAB size) is traced back IN FLIGHT.  Its frames are cut
//     into parts of 256 steps from the top (part 0 = the frame's end); as soon as the ACS is two blocks past the top of part p >= 1,
//     at the next point where the branch-metric table is dead (so that 19 blocks fit the workgroup's 10 KB of LDS), the part is
//     traced speculatively (traceback_part16<SPEC>: every lane 30 steps above its block from state 0, the top lane trusted), its
//     decoded bits go straight to `out`, and the position at its top (spec) and at its bottom (out) are recorded - lane p of two
//     registers holds part p, four frames x 8 bits.
//   * after the forward pass part 0 is traced from the true end state (state 0), and the chain is checked from the top down:
//     part p is final iff spec(p) = out(p - 1).  The first part that fails - 1.1 % of the wave-parts at Eb/N0 = 3 dB, 7 % at 2 dB
//     (profiles/r04_spec_stats.jsonl) - is reloaded from the spill (17 blocks), traced from its true top and checked again:
//     the fixed point is the serial ChainBack (deconvolve.cpp:416-435), as before.
//   * a wave whose first in-flight part shows >= TB_HARD_MISSES missed blocks (input without signal: half of all 30-step
//     speculations fail) stops tracing in flight: its parts stay marked "unchecked" and the top-down loop traces them all from
//     the spill - the behaviour of rounds 2-3.
//   * other groups (mixed lengths in a wave, lengths that are not a multiple of 16) take the general traceback form after the
//     forward pass: the last 17 blocks from the window, the others read back from the spill as before.
// Workgroups are persistent: each takes the next group of 4 frames from an atomic counter, so the spill buffer is sized by the
// resident waves, not by the batch, and a length-sorted descriptor table is consumed longest-first.
constexpr u32 LONG_LDS_BLOCKS = DUMP_GROUP + 1u;  // 17: the blocks of one 256-step part
constexpr u32 LONG_KEEP = DUMP_GROUP;             // the last 16 blocks of a frame are never spilled
constexpr u32 SPEC_BLOCKS = LONG_LDS_BLOCKS + 2u; // an in-flight part and the two blocks above it (30-step warm-up of its top lane)

constexpr u32 IMG_RING = 16;  // output bit image of the general form: a ring of 16 words (512 bits) per frame

__host__ __device__ inline PkLayout pk_layout_long(u32 maxfb) {
    PkLayout l;
    l.maxfb = maxfb;
    l.dec_bytes = DUMP_GROUP * DEC_BLOCK;
    const u32 scratch = 64u * 4u * pk_scratch_words(maxfb), img = 4u * 4u * IMG_RING;
    u32 tabregion = DEC_BLOCK + scratch + img;
    tabregion = tabregion > (u32)TAB_BYTES ? ((tabregion + 15u) & ~15u) : (u32)TAB_BYTES;
    l.img_off = l.dec_bytes + DEC_BLOCK + scratch;
    l.total = l.dec_bytes + tabregion;  // 10 KB for every length: 16 waves per CU
    return l;
}
static_assert(SPEC_BLOCKS * DEC_BLOCK <= DUMP_GROUP * DEC_BLOCK + (u32)TAB_BYTES, "an in-flight part must fit dec + the dead table");

// Where the forward pass keeps the history it may still need (besides the write-only spill): a WINDOW whose slot 0 holds block
// `base` (a signed block number: the short bottom part of a frame starts "below block 0").  Block base + d goes to LDS slot d for
// d < 16 (the dec region); d = 16 .. 19 would land on the branch-metric table, which is live, so those four blocks wait in eight
// VGPRs (the carry) and reach LDS slots 16 .. 19 only when the table is dead: for an in-flight part (slots 0 .. 18 = its 17 blocks and
// the two above), or after the forward pass (slot 16 = the frame's last block).  After an in-flight part the window moves up 16
// blocks and the carried blocks become its slots 0 .. 3.
// The carry is four register pairs, written by ONE inline-asm statement with scalar branches inside: to the compiler a single
// instruction that updates eight registers in place.  Every plainer form cost more than the whole scheme is worth
// (profiles/r04_ab_long_inflight.txt): a switch over the elements of an array or struct - the optimiser merges the four stores into one
// with a computed index and the object lives in scratch memory, i.e. a scratch load behind `s_waitcnt vmcnt(0)` (= behind the
// acknowledgement of the spill stores just issued) at every part, +14 % on a multi-round launch; four separate locals - a web of phi
// copies, eight v_mov_b64 in EVERY block, +3 %; an 8-dword vector with a dynamic index - 16 to 24 v_cndmask per block.
struct Carry {
    u32 a0, b0, a1, b1, a2, b2, a3, b3;  // (acc1, acc0) of window positions 16, 17, 18, 19
};
DEV void carry_put(Carry& c, int d, u32 x, u32 y) {  // d wave-uniform; positions below 16 leave the carry alone
    asm volatile(
        "s_cmp_lt_i32 %[d], 16\n\t"
        "s_cbranch_scc1 .Lcy_end%=\n\t"
        "s_cmp_lg_u32 %[d], 16\n\t"
        "s_cbranch_scc1 .Lcy_1%=\n\t"
        "v_mov_b32 %[a0], %[x]\n\t"
        "v_mov_b32 %[b0], %[y]\n\t"
        "s_branch .Lcy_end%=\n"
        ".Lcy_1%=:\n\t"
        "s_cmp_lg_u32 %[d], 17\n\t"
        "s_cbranch_scc1 .Lcy_2%=\n\t"
        "v_mov_b32 %[a1], %[x]\n\t"
        "v_mov_b32 %[b1], %[y]\n\t"
        "s_branch .Lcy_end%=\n"
        ".Lcy_2%=:\n\t"
        "s_cmp_lg_u32 %[d], 18\n\t"
        "s_cbranch_scc1 .Lcy_3%=\n\t"
        "v_mov_b32 %[a2], %[x]\n\t"
        "v_mov_b32 %[b2], %[y]\n\t"
        "s_branch .Lcy_end%=\n"
        ".Lcy_3%=:\n\t"
        "v_mov_b32 %[a3], %[x]\n\t"
        "v_mov_b32 %[b3], %[y]\n"
        ".Lcy_end%=:"
        : [a0] "+v"(c.a0), [b0] "+v"(c.b0), [a1] "+v"(c.a1), [b1] "+v"(c.b1), [a2] "+v"(c.a2), [b2] "+v"(c.b2), [a3] "+v"(c.a3), [b3] "+v"(c.b3)
        : [d] "s"(d), [x] "v"(x), [y] "v"(y)
        : "scc");
}
// carried blocks 0 .. n - 1 -> LDS slots first .. first + n - 1
DEV void carry_to_lds(const Carry& c, char* dec, u32 dslot, u32 first, u32 n) {
    if (n > 0u) *reinterpret_cast<uint2*>(dec + (first + 0u) * DEC_BLOCK + dslot) = make_uint2(c.a0, c.b0);
    if (n > 1u) *reinterpret_cast<uint2*>(dec + (first + 1u) * DEC_BLOCK + dslot) = make_uint2(c.a1, c.b1);
    if (n > 2u) *reinterpret_cast<uint2*>(dec + (first + 2u) * DEC_BLOCK + dslot) = make_uint2(c.a2, c.b2);
    if (n > 3u) *reinterpret_cast<uint2*>(dec + (first + 3u) * DEC_BLOCK + dslot) = make_uint2(c.a3, c.b3);
}
// four per-frame positions (uniform within each 16-lane row) as one word, frame k in byte k
DEV u32 pack_rows(u32 P) {
    return (u32)__builtin_amdgcn_readlane((int)P, 0) | ((u32)__builtin_amdgcn_readlane((int)P, 16) << 8) |
           ((u32)__builtin_amdgcn_readlane((int)P, 32) << 16) | ((u32)__builtin_amdgcn_readlane((int)P, 48) << 24);
}

#ifndef VIT_LONG_INFLIGHT
#define VIT_LONG_INFLIGHT 1  /* 0: no in-flight parts - every part is traced after the forward pass from the spill (A/B; the rounds 2-3 traffic) */
#endif

// The workgroups of these kernels are ONE wavefront, and a wavefront's LDS instructions execute in issue order: what a
// __syncthreads() has to provide here is only that the compiler keeps LDS accesses on their side of it.  __syncthreads() itself
// is a workgroup-scope fence, i.e. `s_waitcnt vmcnt(0)` as well - in the long-frame kernel that is a wait for the acknowledgement
// of the spill and output stores just issued (1-2 us each time, 4.5 us per in-flight part: profiles/r04_ab_long_inflight.txt).
DEV void wave_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

template <bool SYM32>
__global__ __launch_bounds__(64, 4) void vit_pk_long_kernel(const uint8_t* __restrict__ sym, uint8_t* __restrict__ out,
                                                             const vit_frame_desc* __restrict__ desc,
                                                             u32 framebits_uniform, long long nframes, PkLayout lay,
                                                             uint2* spill, u32 spill_blocks, unsigned* counter,
                                                             u32 ngroups, u32 short_max,
                                                             const unsigned* __restrict__ split_gate, u32 renorm_c, u32 nsimd) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    char* dec = lds;                  // 16 blocks; 17th ... 20th land on the table when it is dead
    char* tab = lds + lay.dec_bytes;  // [tau][pair][c] -> M; after the ACS: last block, scratch, image
    u32* img = reinterpret_cast<u32*>(lds + lay.img_off);
    const u32 lane = threadIdx.x;
    uint2* wspill = spill + (size_t)blockIdx.x * spill_blocks * 64u + lane;
    // few long frames in the table: leave the short groups to the single-segment kernel (no spill for them);
    // many: keep them - they are the small jobs that level the end of this kernel's longest-first schedule
    const bool split = split_gate && (unsigned long long)*split_gate * PK_SPLIT_DEN < (unsigned long long)nframes;

    // ---- lane constants (same roles as in vit_pk_kernel) ----
    const u32 l5 = acs_l5(lane);
    const u32 dslot = dec_slot(lane);  // where this lane's history words go inside a decision block
    Lanes L;
    load_toff(L, lane);
    Lanes L1;
    {
        const u32 tb = (u32)(uintptr_t)(const __attribute__((address_space(3))) char*)tab;
#pragma unroll
        for (int rho = 0; rho < 5; rho++) {
            L.toff[rho] += tb;
            L1.toff[rho] = L.toff[rho] + 1024u;
            asm volatile("" : "+v"(L1.toff[rho]));  // its own register: as "L + 1024" the ds_read2 pairs would need an add again
        }
    }
    Consts C;
    C.hi = HI;
    C.rc = renorm_c;
    asm volatile("" : "+v"(C.hi));
    const u32 tau = lane >> 1, pp = lane & 1u;
    u32 sel[4];
    {
        const u32 hb = (tau & 1u) ? 0x0C000C00u : 0x0D000D00u;
#pragma unroll
        for (int k = 0; k < 4; k++) sel[k] = hb | (0x00040000u + 0x00010001u * k);
    }
    const PrepassLane PL = prepass_lane(lane);

    const u32 prio_slot = hw_id() & 3u;  // wave slot within the SIMD
    // every wave of this kernel at the level of the single-segment kernel's three regular waves: when a split table runs both kernels
    // side by side, the few long groups are the critical path and must not rank below the other kernel's waves
    __builtin_amdgcn_s_setprio(1);
    // A launch with no more groups than workgroups is ONE round of waves: nothing takes the place of a wave that is done, and the
    // hardware's arbitration lets the four waves of a SIMD finish one after the other (profiles/r03_timeline.jsonl: at 320, 385,
    // 450 and 550 us of a 558 us launch), i.e. the SIMD runs on three, two, one wave for the second half.  An issue priority that
    // rotates block by block gives every wave the same share, and they finish together: 16384 x 3072 bits 0.561 -> 0.473 ms,
    // 16384 x 4608 bits 0.812 -> 0.700 (profiles/r03_ab_long_oneround.txt).  Doing the same for the LAST round of a longer launch
    // (the groups from ngroups - gridDim.x on) measured worse than leaving multi-round launches alone.
    bool first_group = true;
    for (;;) {
        u32 grp = 0;
        // a workgroup's first group is its own index; only the later ones come from the counter (4096 workgroups that start
        // with an atomic on one address are served one at a time: the last one waited 46 us, profiles/r03_timeline.jsonl).
        // Worth 3-7 % on most multi-round shapes and on config 3; launches of an exact number of rounds lose 2-3 % (the
        // staggered start had kept their rounds apart): profiles/r03_ab_long_oneround.txt
        if (first_group) {
            grp = blockIdx.x;
        } else {
            if (lane == 0) grp = gridDim.x + atomicAdd(counter, 1u);
            grp = (u32)__builtin_amdgcn_readfirstlane((int)grp);
        }
        first_group = false;
        if (grp >= ngroups) break;
        // The launch's LAST round of fetches (nothing replaces a wave that finishes it): the issue priority grows with the fetch order, one
        // level per quarter of the round, so the waves that start their last group late get the slots first and a SIMD's last waves finish
        // closer together.  Uniform launches of >= 2.25 rounds only: measured over 1 ... 10 rounds x four frame lengths
        // (profiles/r04_ab_long_inflight.txt, section 13) it takes 3-11 % off 2.5 ... 5 rounds (config 5's decode, 5 rounds: -3 %), is within
        // +-2 % from 5.5 rounds up, costs 7 % at exactly two rounds (all waves fetch together: the levels only unbalance them) and 2-3 % on a
        // length-sorted table, whose last fetches are its shortest frames.
        // (a sorted table whose first and last frame are equally long is a uniform launch too)
        const bool uniform_launch = !desc || desc[0].framebits == desc[nframes - 1].framebits;
        if (uniform_launch && (unsigned long long)ngroups * 4ull >= 9ull * gridDim.x && grp + gridDim.x >= ngroups) {
            set_prio(((grp - (ngroups - gridDim.x)) * 4u) / gridDim.x);
        }
#ifdef VIT_DIAG_TIMES
        const unsigned long long diag_t0 = __builtin_amdgcn_s_memrealtime();
        unsigned long long diag_tr = 0;  // time spent in in-flight parts
#endif
        const long long f0 = (long long)grp * 4;
        u32 fbits[4];
        size_t soff[4], ooff[4];
        u32 maxfb = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const long long f = f0 + k;
            fbits[k] = 0;
            soff[k] = ooff[k] = 0;
            if (f < nframes) {
                if (desc) {
                    fbits[k] = desc[f].framebits;
                    soff[k] = desc[f].sym_offset;
                    ooff[k] = desc[f].out_offset;
                    if (fbits[k] > lay.maxfb || (fbits[k] & 1u) || (soff[k] & 3u)) fbits[k] = 0;  // not what the launch was sized for / misaligned
                } else {
                    fbits[k] = framebits_uniform;
                    soff[k] = (size_t)f * 4u * (framebits_uniform + VIT_TAIL);
                    ooff[k] = (size_t)f * ((framebits_uniform + 7u) >> 3);
                }
            }
            maxfb = fbits[k] > maxfb ? fbits[k] : maxfb;
        }
        if (maxfb == 0) continue;
        // length-sorted mixed table: the groups that fit the single-segment kernel are that kernel's (it keeps two
        // thirds of the history in VGPRs instead of spilling it).  The table is ordered by the sort's 8-bit-wide bins
        // only: bin 98 holds 778-bit frames (short) next to 780/782/784-bit ones (long) in no particular order, so a
        // short group inside that bin is skipped, not taken as the end; from the first group of the bins below
        // (maxfb <= 776) on, every later group is short as well.
        if (split && maxfb <= short_max) {
            if (maxfb <= (short_max & ~7u)) break;
            continue;
        }
        const u32 nblk = (maxfb + VIT_TAIL + 15u) >> 4;
        const u32 G = nblk > LONG_KEEP ? nblk - LONG_KEEP : 0u;  // spilled blocks (<= spill_blocks)
        // A descriptor table is consumed longest first, and the launch ends when the workgroup with the longest frames does: in a multi-round
        // table the groups of more than 3/4 (1/2) of the launch's longest frame run at issue priority 3 (2), the rest at 1 - the long groups
        // finish sooner, the dynamic counter levels the short ones behind them.  Config 3 as drawn: 1.125 -> 1.058 ms at 3 dB, the same 6 % at
        // 0 dB and on input without signal; with the 1/2 threshold alone or thresholds of 7/8 and 3/4: nothing
        // (profiles/r04_ab_long_inflight.txt, section 19).  A table of equal lengths runs at one level throughout, as before.
        if (desc && ngroups > gridDim.x && desc[0].framebits != desc[nframes - 1].framebits) {
            // the launch's longest frame: the first descriptor of the (sorted) table; what the caller declared as max_framebits may be generous
            u32 ref = desc[0].framebits;
            if (ref > lay.maxfb || ref < maxfb) ref = lay.maxfb;
            if ((unsigned long long)maxfb * 4ull > (unsigned long long)ref * 3ull) __builtin_amdgcn_s_setprio(3);
            else if ((unsigned long long)maxfb * 2ull > (unsigned long long)ref) __builtin_amdgcn_s_setprio(2);
            else __builtin_amdgcn_s_setprio(1);
        }
        const u32 T_max = maxfb + VIT_TAIL;
        const u32 a_fb = pp ? fbits[2] : fbits[0], b_fb = pp ? fbits[3] : fbits[1];
        const u32 a_T = a_fb ? a_fb + VIT_TAIL : 0u, b_T = b_fb ? b_fb + VIT_TAIL : 0u;
        constexpr size_t SB = SYM32 ? 4 : 1;  // bytes per soft symbol in memory
        const uint8_t* a_sym = sym + SB * (pp ? soff[2] : soff[0]);
        const uint8_t* b_sym = sym + SB * (pp ? soff[3] : soff[1]);
        const u32 fi = lane >> 4;
        const u32 t_fb = fi == 0 ? fbits[0] : fi == 1 ? fbits[1] : fi == 2 ? fbits[2] : fbits[3];
        uint8_t* o_f = out + (fi == 0 ? ooff[0] : fi == 1 ? ooff[1] : fi == 2 ? ooff[2] : ooff[3]);
        const bool fast = fbits[0] == fbits[1] && fbits[1] == fbits[2] && fbits[2] == fbits[3] && (maxfb & 15u) == 0;
        // parts of a fast group: part p = steps [max(hi - 256, 6), hi), hi = T_max - 256 p; its top block is nblk - 1 - 16 p and its
        // window base nblk - 17 - 16 p (part 0 = the frame's last 17 blocks)
        const u32 NP = fast ? (maxfb + 255u) >> 8 : 0u;
        u32 p_next = (VIT_LONG_INFLIGHT && NP > 1u) ? NP - 1u : 0u;  // bottom part first; 0 = nothing (left) to trace in flight
        // the window the ACS is filling: the next in-flight part's, else the frame's last 17 blocks (all of a shorter frame)
        int base = (fast ? (int)nblk - (int)LONG_LDS_BLOCKS : (int)(nblk > LONG_LDS_BLOCKS ? nblk - LONG_LDS_BLOCKS : 0u)) - 16 * (int)p_next;
        u32 rec_spec = 0xFFFFFFFFu, rec_out = 0u;  // lane p: part p, frame k in byte k; 0xFFFFFFFF = not traced (never equals a position)

        // ---- forward pass: ACS with history over all blocks ----
        u32 A = l5 == 0 ? 0u : 0x003F003Fu, B = 0x003F003Fu;
        u32 acc0 = 0, acc1 = 0;
        Carry cy = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        {
            auto sa = load_step<SYM32>(a_sym, tau, tau < a_T), sb = load_step<SYM32>(b_sym, tau, tau < b_T);
            u32 v = 0;
            // Two blocks per trip - the pre-pass's 32 steps: the even block reads table half 0, the odd one half 1 (see vit_pk_kernel:
            // the copies of loop-carried values once per pair).  In-flight parts start behind ODD blocks only: the table is dead there.
            const bool last6 = (T_max & 15u) == 6u;  // the frame's last block has six steps
            // (a launch of at most one wave per SIMD - ngroups <= nsimd - has nothing to rotate between, and the s_setprio per block costs it 4.5 %)
            const bool rot = ngroups <= gridDim.x && ngroups > nsimd;  // one round of waves
            auto rotate = [&](const u32 rbx) {
                if (rot) set_prio((prio_slot + rbx) & 3u);
            };
            // a finished block's history words: the write-only spill, and the window (LDS slot or carry)
            auto put = [&](const u32 rbx) {
                const uint2 hw = make_uint2(acc1, acc0);  // the order of the LDS blocks: a reload is a plain copy
                if (rbx < G) wspill[(size_t)rbx * 64u] = hw;
                const int dx = (int)rbx - base;  // position in the window (< 0: a block no later part of this wave needs in LDS)
                if (dx >= 0 && dx < (int)DUMP_GROUP) *reinterpret_cast<uint2*>(dec + (u32)dx * DEC_BLOCK + dslot) = hw;
                carry_put(cy, dx, acc1, acc0);
            };
            for (u32 rb0 = 0; rb0 < nblk; rb0 += 2u) {
                rotate(rb0);
                wave_sync();
                prepass(pack_step(sa), pack_step(sb), tab, PL, sel);
                const u32 tn = (rb0 + 2u) * 16u + tau;
                sa = load_step<SYM32>(a_sym, tn, tn < a_T);
                sb = load_step<SYM32>(b_sym, tn, tn < b_T);
                wave_sync();
                if (last6 && rb0 + 1u == nblk) steps6(v, A, B, acc0, acc1, tab, L, lane, C);
                else steps16<true>(v, A, B, acc0, acc1, tab, L, lane, C);
                put(rb0);
                v = v == 4 ? 0 : v + 1;
                if (rb0 + 1u >= nblk) break;
                const u32 rb = rb0 + 1u;  // the odd block
                rotate(rb);
                if (last6 && rb + 1u == nblk) steps6(v, A, B, acc0, acc1, tab, L1, lane, C);
                else steps16<true>(v, A, B, acc0, acc1, tab, L1, lane, C);
                put(rb);
                const int d = (int)rb - base;
                // part p_next is traced in flight after the first ODD block (the table is dead then) that is >= two blocks above its top
                if (p_next && d >= (int)LONG_LDS_BLOCKS + 1) {
                    const u32 hi = T_max - 256u * p_next;
                    const u32 lo = hi > 256u + VIT_TAIL ? hi - 256u : VIT_TAIL;
                    const u32 nc = (u32)d - (DUMP_GROUP - 1u);  // carried blocks: 3 or 4
                    // The part runs at the issue priority the wave has.  It is a chain of ~50 dependent LDS reads with five instructions each;
                    // raising its priority (3) so that none of them queues behind the other waves' ACS measured 2-10 % SLOWER on multi-round
                    // launches, lowering it (0) no better: profiles/r04_ab_long_inflight.txt
#ifdef VIT_DIAG_TIMES
                    const unsigned long long diag_ta = __builtin_amdgcn_s_memrealtime();
#endif
                    wave_sync();  // every table read of this block is done
                    carry_to_lds(cy, dec, dslot, DUMP_GROUP, nc);
                    wave_sync();
                    u32 pspec = 0, misses = 0;
                    const u32 pout = traceback_part16<true, true>(dec, nullptr, 0u, lane, lo, (hi - lo) >> 4, (u32)base, 0u, 0u, o_f, &pspec, &misses);
#ifdef VIT_SPEC_SABOTAGE  /* test build: every in-flight part fails its check and comes back from the spill (outputs must not change) */
                    const u32 ks = pack_rows(pspec) ^ ((p_next & 1u) ? 0x04040404u : 0x00000800u), ko = pack_rows(pout);
#else
                    const u32 ks = pack_rows(pspec), ko = pack_rows(pout);
#endif
                    if (lane == p_next) {
                        rec_spec = ks;
                        rec_out = ko;
                    }
                    SPEC_COUNT(1);
                    if (misses >= TB_HARD_MISSES && p_next > 1u) SPEC_COUNT(2);
                    p_next--;
                    wave_sync();  // the part's blocks have been read
                    if (misses >= TB_HARD_MISSES && p_next && (int)rb < (int)nblk - (int)LONG_LDS_BLOCKS) {
                        // input without signal (half of all 30-step speculations fail): no more parts in flight, the top-down loop
                        // below takes them from the spill; the window jumps to the frame's last 17 blocks (always ahead of the ACS
                        // here: a part that is not the last but one ends >= 32 blocks below the top - the test is belt and braces)
                        p_next = 0;
                        base = (int)nblk - (int)LONG_LDS_BLOCKS;
                    } else {
                        base += (int)DUMP_GROUP;  // the next part up (part 0 included): the carried blocks are its first ones
                        carry_to_lds(cy, dec, dslot, 0u, nc);
                    }
#ifdef VIT_DIAG_TIMES
                    diag_tr += __builtin_amdgcn_s_memrealtime() - diag_ta;
#endif
                }
                v = v == 4 ? 0 : v + 1;
            }
        }
        // the frame's last block (window position 16) waited in the carry for the table to die
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // once per group: the spill is complete before anything is read back
        wave_sync();
        if ((int)nblk - 1 - base == (int)DUMP_GROUP) carry_to_lds(cy, dec, dslot, DUMP_GROUP, 1u);
#ifdef VIT_DIAG_TIMES
        const unsigned long long diag_t1 = __builtin_amdgcn_s_memrealtime();
#endif

        if (fast) {
            // ---- part 0 from the window and the true end state, then the chain of parts from the top down: a part whose recorded
            // top position is not what the part above ends in (or that was never traced) comes back from the spill ----
            u32 p = 0;
            SPEC_COUNT(0);
            uint2 d[LONG_LDS_BLOCKS];  // a part's 17 blocks on their way from the spill to LDS
#pragma unroll
            for (u32 k = 0; k < LONG_LDS_BLOCKS; k++) d[k] = make_uint2(0u, 0u);
            auto request = [&](const u32 q) {  // issue the loads of part q's blocks
                const u32 qhi = T_max - 256u * q;
                const u32 qlo = qhi > 256u + VIT_TAIL ? qhi - 256u : VIT_TAIL;
                const u32 qb = qlo >> 4, qn = (qhi - qlo) >> 4;
#pragma unroll
                for (u32 k = 0; k < LONG_LDS_BLOCKS; k++) d[k] = k <= qn ? wspill[(size_t)(qb + k) * 64u] : make_uint2(0u, 0u);
            };
            for (u32 it = 0; it <= NP; it++) {
                if (it) {
                    const u32 up = (u32)__shfl_up((int)rec_out, 1);
                    const unsigned long long bad = __ballot(lane >= 1u && lane < NP && rec_spec != up);
                    if (bad == 0) break;
                    p = (u32)__builtin_ctzll(bad);  // the topmost such part: everything above it is final
                    SPEC_COUNT(3);
                    if ((u32)__builtin_amdgcn_readlane((int)rec_spec, (int)p) != 0xFFFFFFFFu) SPEC_COUNT(4);
                }
                const u32 hi = T_max - 256u * p;
                const u32 lo = hi > 256u + VIT_TAIL ? hi - 256u : VIT_TAIL;
                const u32 nl = (hi - lo) >> 4;
                u32 slot0 = (u32)base;  // part 0 sits in the window the forward pass left behind
                u32 ktop = 0x01010101u * P_ZERO;
                if (p) {
                    slot0 = lo >> 4;
                    wave_sync();
                    ktop = (u32)__builtin_amdgcn_readlane((int)rec_out, (int)(p - 1u));
                    request(p);
#pragma unroll
                    for (u32 k = 0; k < LONG_LDS_BLOCKS; k++)
                        if (k <= nl) *reinterpret_cast<uint2*>(dec + k * DEC_BLOCK + dslot) = d[k];
                }
                // A part's blocks are requested when it is traced, not ahead: requesting a never-traced part below while this one is traced
                // measured config 3 on input without signal 1.37 ms without, 1.39 ms with (profiles/r04_ab_long_inflight.txt §7)
                wave_sync();
                const u32 P_top = (ktop >> (8u * fi)) & 0xFFu;
                const u32 pout = traceback_part16<false, true>(dec, nullptr, 0u, lane, lo, nl, slot0, P_top, 0u, o_f);
                const u32 ko = pack_rows(pout);
                if (lane == p) {
                    rec_spec = ktop;
                    rec_out = ko;
                }
            }
            wave_sync();  // the part's LDS blocks are read before the next group's pre-pass reuses the region
#ifdef VIT_DIAG_TIMES
            if (lane == 0 && grp < 16384u) {
                u32 hwid;
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
                g_diag_times[grp * 4u + 0u] = diag_t0;
                g_diag_times[grp * 4u + 1u] = diag_t1;
                g_diag_times[grp * 4u + 2u] = __builtin_amdgcn_s_memrealtime();
                g_diag_times[grp * 4u + 3u] = diag_tr;
            }
#endif
            continue;
        }
        // ---- general form: LDS tail (the last 17 blocks: the window), then the spilled blocks 16 at a time from the top ----
        const u32 Gg = nblk > LONG_LDS_BLOCKS ? nblk - LONG_LDS_BLOCKS : 0u;  // blocks below the LDS tail (= base: the window never moved)
        img[lane] = 0;  // 4 frames x IMG_RING words (the ring aliases the dead table region behind the 17th block)
        wave_sync();
        const u32 slot = lane & (IMG_RING - 1u);
        const u32 t_T = t_fb ? t_fb + VIT_TAIL : 0u;
        const u32 nbytes_f = (t_fb + 7u) >> 3;  // a partial last byte is padded with zero bits (ChainBack starts from E = 0)
        const bool o_aligned = (reinterpret_cast<uintptr_t>(o_f) & 3u) == 0;
        u32 d_hi = (t_fb + 31u) >> 5;  // image words [d_lo, d_hi) of this lane's frame are not written out yet
        // The image is a ring: after a part has been traced back, every decoded bit from its first step up is
        // final.  Lane (frame, slot) owns the one word of [d_lo, d_hi) that maps to its ring slot: it goes out as
        // 4 MSB-first bytes (deconvolve.cpp:432-433) and the slot is cleared for the words further down.
        auto flush = [&](const u32 ts_done) {
            const u32 d_lo = ts_done <= VIT_TAIL ? 0u : (ts_done - VIT_TAIL + 31u) >> 5;
            wave_sync();  // all atomicOr of the part have landed
            const u32 d = d_lo + ((slot - d_lo) & (IMG_RING - 1u));
            if (d < d_hi) {
                const u32 v = __builtin_bswap32(__builtin_bitreverse32(img[lane]));  // byte k = bit-reversed byte k
                img[lane] = 0;
                const u32 b = 4u * d;
                if (o_aligned && b + 4u <= nbytes_f) {
                    *reinterpret_cast<u32*>(o_f + b) = v;
                } else {
#pragma unroll
                    for (u32 k = 0; k < 4u; k++)
                        if (b + k < nbytes_f) o_f[b + k] = (uint8_t)(v >> (8u * k));
                }
            }
            d_hi = d_hi < d_lo ? d_hi : d_lo;
            wave_sync();
        };
        u32* scratch = reinterpret_cast<u32*>(tab + DEC_BLOCK) + lane * pk_scratch_words(lay.maxfb);
        const u32 t_lo = Gg * 16u;
        const u32 ts_top = t_lo > VIT_TAIL ? t_lo : VIT_TAIL;
        // the spilled blocks come back 16 at a time; a group is fetched into registers while the part above it
        // is being traced back, so its HBM latency is off the wave's critical path
        uint2 d[DUMP_GROUP];
#pragma unroll
        for (u32 k = 0; k < DUMP_GROUP; k++) d[k] = make_uint2(0u, 0u);  // defined on EVERY path: left undefined on the path without a fetch, the array counted as live
                                                                          // across the whole group loop - 29 more VGPRs (128 instead of 99) and 2-6 % of the 3 dB rate (r04_ab_long_inflight.txt §7)
        auto fetch = [&](const u32 g0, const u32 g1) {
#pragma unroll
            for (u32 k = 0; k < DUMP_GROUP; k++)
                d[k] = (g0 + k < g1) ? wspill[(size_t)(g0 + k) * 64u] : make_uint2(0u, 0u);
        };
        if (Gg) fetch(Gg > DUMP_GROUP ? Gg - DUMP_GROUP : 0u, Gg);
        u32 warm = TB_WARM;
        u32 P_part = traceback_part(dec, scratch, img, IMG_RING, lane, ts_top, t_T, T_max, Gg, P_ZERO, warm, IMG_RING - 1u);
        flush(ts_top);
        for (u32 g1 = Gg; g1 > 0;) {
            const u32 g0 = g1 > DUMP_GROUP ? g1 - DUMP_GROUP : 0u;
            wave_sync();
#pragma unroll
            for (u32 k = 0; k < DUMP_GROUP; k++)
                *reinterpret_cast<uint2*>(dec + k * DEC_BLOCK + dslot) = d[k];
            wave_sync();
            if (g0) fetch(g0 > DUMP_GROUP ? g0 - DUMP_GROUP : 0u, g0);  // next group down, in flight during this part
            const u32 tsg = g0 ? g0 * 16u : VIT_TAIL, tend = g1 * 16u;
            const u32 te = t_T < tend ? t_T : tend, te_max = T_max < tend ? T_max : tend;
            const u32 P_top = t_T > tend ? P_part : P_ZERO;
            P_part = traceback_part(dec, scratch, img, IMG_RING, lane, tsg, te, te_max, g0, P_top, warm, IMG_RING - 1u);
            flush(tsg);
            g1 = g0;
        }
        wave_sync();  // the image is read before the next group's pre-pass reuses the region
    }
}

}  // namespace
