// vit_pk.hip -- packed K=7 r=1/4 Viterbi decoder for gfx950: FOUR frames per
// wavefront, no cross-lane traffic through LDS memory in the add-compare-select loop.
//
// Layout.  A wave owns frames F(p,h), p = lane>>5 ("pair"), h = 16-bit half of a
// VGPR.  Within a pair, the 64 path metrics of a frame live in two registers x 32
// lanes: register A holds the state with s5 = 0, register B the one with s5 = 1,
// of the butterfly i = rol5(lane&31, t mod 5).  A butterfly therefore reads both
// of its predecessors (i, i+32) from its own lane, and both survivors
// (2i, 2i+1) stay in the lane.  After each step ONE register bit and ONE lane
// bit swap roles (lane bit 4,3,2,1,0,4,... = 4 - t mod 5): v_permlane16_swap for
// bit 4, masked DPP moves for bits 3/2, ds_swizzle + select for bits 1/0.  The
// state <-> lane map rotates with period 5, so the step body is unrolled
// 5-periodically (16 steps x 5 variants).
//
// Arithmetic.  Metrics are u16 lanes of v_pk_* instructions holding m + 0xFF00,
// so `v_pk_add_u16 clamp` IS paddusb (saturation at 255).  The renormalisation
// (`psubusb 63` when state 0 > 150, every second step) is `v_pk_sub_u16 clamp`
// against 0xFF00 + {0,63}, which lands in a 0-based representation; the branch
// metric table of the following (even) step carries the +0xFF00 back.  Decisions
// are the sign bits of m0-m1 / m2-m3, shifted into two per-lane history registers,
// one 32-bit word pair (8 B/lane) per 16 steps.
//
// Branch metrics.  Only 8 distinct (b0,b1,b2) mask triples exist, so a 32-step
// pre-pass (lane = pair x step) computes the 8 pavgb-tree metrics of both frames of
// its pair with byte-wide v_perm_b32 / v_lerp_u8 and writes a table of M to LDS; an
// ACS lane reads its 4 bytes per step and forms 63-M with one v_sub.
//
// Decision storage.  LDS (160 KB/CU) is what limits resident waves.  Per segment of
// 49 blocks (784 steps) the first 32 blocks of history stay in VGPRs (two 32-dword
// register arrays indexed with s_set_gpr_idx), 16 go to LDS and the last one to the
// start of the then-dead metric table: 10 KB of LDS per wave, 16 waves per CU.
// Longer frames (vit_pk_long_kernel): same forward pass; the frame is traced back 256 steps at a time WHILE
// the pass runs, from a 16-block window in LDS, and every block is also written - once, 8 B per frame-step -
// to a per-workgroup slice of HBM from which only a part that fails its check is read back.
//
// Traceback.  Per segment three parts (LDS tail, then the register blocks 16 at a
// time through the same LDS region), each blocked and speculative: lane = (frame,
// block of BL steps); a block is traced from state 0 after a 30-step warm-up (or
// from the true position when that reaches the frame end), checked against the
// block above and re-traced until nothing changes.  The last block really starts
// in state 0 (tail-terminated), so the fixed point is exactly the serial chainback.
// Two forms: the general one (any mix of lengths in a wave, 20-step blocks, a loop
// with a predicate per step) and, since round 3, a fast one for waves of four equally
// long frames of a multiple of 16 bits - every DAB size -: 16-step blocks in
// straight-line code, 5 instead of 9 instructions per step back (traceback_part16).
//
// Scheduling (round 3, from a per-workgroup timeline of the launch, tools/exp/timeline.py): the hardware's arbitration lets the
// waves of a SIMD advance one after the other.  In a launch of many rounds of waves that is welcome - the latency-bound traceback
// of one wave runs under the ACS of the others - and ONE wave per SIMD at a lower static issue priority is the best of eight
// maps measured (four distinct levels starve the lowest: 63 ... 248 us per wave and a 50 us drain).  In a launch of ONE round
// nothing replaces a finished wave, so the priority rotates block by block and the four waves finish together (a separate
// instantiation of the single-segment kernel; a run-time branch in the persistent long-frame kernel, whose workgroups also take
// their first group statically instead of queueing at one atomic counter).  Round 4 (profiles/r04_ab_long_inflight.txt, sections 13-21): the
// persistent kernel's multi-round launches follow "more work left -> more issue slots" - in a uniform launch the last round of
// fetches runs at a priority that grows with the fetch order, in a length-sorted table the long groups run above the short ones -;
// an s_setprio per block is not free, so launches of at most one wave per SIMD do not rotate.
//
// Instruction costs that shaped this (profiles/r01_valu_issue_rates_ubench.txt): v_pk_*,
// VOP3 three-operand, DPP, SDWA, v_cmp = 4 cycles per wave; plain VOP2 = 2;
// v_permlane*_swap = 8; v_cndmask_b32 via VCC ~22; SALU 1 instr/cycle/CU.
//
// Files (ONE translation unit on purpose: g_toff and the diagnostic counters are device globals, and this build has no
// relocatable device code): vit_pk_dev.h branch metrics, pre-pass and symbol loads (shared with vit_pk8.hip); vit_pk_acs.h sizes, lane
// exchange, ACS step, block bodies, segment layout, issue-priority helpers; vit_pk_tb.h both traceback forms; vit_pk_fixed.h the
// fixed-geometry FIC kernel; vit_pk_long.h the long-frame kernel; this file the single-segment kernel and the launcher.  The build
// switches left are VIT_DIAG_SPEC, VIT_DIAG_TIMES, VIT_SPEC_SABOTAGE (test / diagnostic builds), VIT_LONG_INFLIGHT and VIT_FIC_FIXED.
// The set-up the three kernels repeat (table addresses L / L1, sel[], the per-frame fbits / soff / ooff block) stays written out:
// every helper form tried re-ordered the kernels' compiled code (tools/isa_same.py, profiles/r18_pk_isa_same.txt).
//
// Replaces, from scratch: decon_avx2 / Butterfly256 (deconvolve.cpp:334-387,
// 514-526), Load8Syms256 (:219-228), Renormalize256 (:407-412), ChainBack
// (:416-435), chainback.inc:18-41 and const.asm:19-63.
#include <cstdlib>
#include <mutex>

#include "vit_internal.h"
#include "vit_pk_acs.h"
#include "vit_pk_tb.h"
#include "vit_pk_fixed.h"
#include "vit_pk_long.h"

namespace {

// Single-segment kernel: every frame of the launch fits 49 blocks (framebits <= 778; the FIC fast path).
// One workgroup (= one wave) per group of 4 frames, dispatched by the hardware.  A persistent form of this kernel
// (workgroups looping over groups, static stride or atomic counter, with and without a start-up stagger) was
// measured 7-12 % SLOWER on the benchmark batch and is not kept: profiles/r02_ab_persist.txt, r02_ab_stagger.txt,
// r02_ab_noprio.txt.  Even the loop scaffolding alone (grid = groups, one trip) cost 12 % through the register
// allocation it led to (128 VGPRs / 104 SGPRs instead of 113 / 63): profiles/r02_ab_r1kernel_vs_loop.txt.
// ROT: a launch of ONE round of waves (no more workgroups than the device holds at once): nothing takes the place of a wave that
// is done, so the static per-slot priorities - under which a wave takes between 63 and 248 us - would leave the second half of the
// launch to ever fewer waves; the priority rotates block by block instead and the four waves of a SIMD finish together
// (16384 FIC frames: 0.130 -> 0.117 ms).  A separate instantiation: the rotation's test inside the block loop cost launches that
// do not use it up to 6 % (profiles/r03_ab_long_oneround.txt).
template <bool SYM32, bool ROT>
__global__ __launch_bounds__(64, 4) void vit_pk_kernel(const uint8_t* __restrict__ sym, uint8_t* __restrict__ out,
                                                        const vit_frame_desc* __restrict__ desc, u32 framebits_uniform,
                                                        long long nframes, PkLayout lay, u32 vmax,
                                                        const unsigned* __restrict__ split_gate, u32 renorm_c) {
    // second launch behind the long-frame kernel on a length-sorted table: runs only if that kernel left the short
    // groups to it (same test there, see vit_launch_pk)
    if (split_gate && (unsigned long long)*split_gate * PK_SPLIT_DEN >= (unsigned long long)nframes) return;
#ifdef VIT_DIAG_TIMES
    const unsigned long long diag_t0 = __builtin_amdgcn_s_memrealtime();  // s_memtime
#endif
    extern __shared__ __attribute__((aligned(16))) char lds[];
    char* dec = lds;                  // [block - R][lane] -> (acc0, acc1); the last block spills into tab
    char* tab = lds + lay.dec_bytes;  // [tau][pair][c] -> M; after the ACS: last block, scratch, image
    u32* img = reinterpret_cast<u32*>(lds + lay.img_off);  // output bit image, 4 frames
    const u32 lane = threadIdx.x;
    const long long f0 = (long long)blockIdx.x * 4;
    // Stagger the waves that share a SIMD: different issue priorities make them drift apart, so the
    // latency-bound traceback of one overlaps the ACS of the others instead of all four hitting it together.
    const u32 prio_slot = hw_id() & 3u;  // wave slot within the SIMD
    set_prio(prio_map(prio_slot));

    // ---- per-frame parameters (wave-uniform loads) ----
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
                // a descriptor the launch was not sized for (longer than max_framebits, or odd) is skipped rather
                // than allowed to run off the LDS layout; so is one whose symbols are not dword aligned.
                // (vmax = the launch's max_framebits; it exceeds lay.maxfb when this kernel only takes the short
                // groups of a length-sorted mixed table, see vit_launch_pk)
                if (fbits[k] > vmax || (fbits[k] & 1u) || (soff[k] & 3u)) fbits[k] = 0;
            } else {
                fbits[k] = framebits_uniform;
                soff[k] = (size_t)f * 4u * (framebits_uniform + VIT_TAIL);
                ooff[k] = (size_t)f * ((framebits_uniform + 7u) >> 3);
            }
        }
        maxfb = fbits[k] > maxfb ? fbits[k] : maxfb;
    }
    if (maxfb == 0 || maxfb > lay.maxfb) return;  // nothing valid / a group of the long-frame kernel
    const u32 nb = (maxfb + VIT_TAIL + 15u) >> 4, R = pk_reg_blocks(nb);
    const u32 fstride = pk_img_stride(maxfb);  // image dwords per frame (+ slack for the shifted spill)
    const u32 T_max = maxfb + VIT_TAIL;

    // ---- ACS lane constants ----
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
    asm volatile("" : "+v"(C.hi));  // keep it in a VGPR
    // ---- pre-pass lane constants: lane = (tau = lane>>1, pair pp = lane&1) ----
    const u32 tau = lane >> 1, pp = lane & 1u;
    const u32 a_fb = pp ? fbits[2] : fbits[0], b_fb = pp ? fbits[3] : fbits[1];
    const u32 a_T = a_fb ? a_fb + VIT_TAIL : 0u, b_T = b_fb ? b_fb + VIT_TAIL : 0u;
    constexpr size_t SB = SYM32 ? 4 : 1;  // bytes per soft symbol in memory
    const uint8_t* a_sym = sym + SB * (pp ? soff[2] : soff[0]);
    const uint8_t* b_sym = sym + SB * (pp ? soff[3] : soff[1]);
    u32 sel[4];
    {
        const u32 hb = (tau & 1u) ? 0x0C000C00u : 0x0D000D00u;  // even step: 0xFF high bytes (= +0xFF00)
#pragma unroll
        for (int k = 0; k < 4; k++) sel[k] = hb | (0x00040000u + 0x00010001u * k);  // byte k of half 0 / half 1
    }
    const PrepassLane PL = prepass_lane(lane);
    u32 A = l5 == 0 ? 0u : 0x003F003Fu, B = 0x003F003Fu;  // const.asm:19-25 (0-based, step 0 is even)
    u32 acc0 = 0, acc1 = 0;
    v32u r0, r1;  // register-resident decisions of blocks [0,R)

    // ---- ACS over the blocks ----
    {
        auto sa = load_step<SYM32>(a_sym, tau, tau < a_T), sb = load_step<SYM32>(b_sym, tau, tau < b_T);
        u32 v = 0;
        // Two blocks per trip - the pre-pass's 32 steps: the even block reads table half 0, the odd one half 1.  (One block per trip cost
        // four v_mov of loop-carried values per block; per pair of blocks it is the same four.)
        const bool last6 = (T_max & 15u) == 6u;  // the frame's last block has six steps
        auto put = [&](const u32 rbx) {  // the block's history words: registers for blocks < R, else LDS (the last one on the dead table)
            u32 rbs = rbx;
            asm volatile("" : "+s"(rbs));  // the address is formed from the scalar block index here: as an induction variable it cost a VALU add in every block
            if (rbx < R) {
                r0[rbx] = acc0;  // s_set_gpr_idx_on / v_mov / s_set_gpr_idx_off
                r1[rbx] = acc1;
            } else {
                if (rbx + 1u == nb) __syncthreads();  // the last block lands on the table: all reads done first
                *reinterpret_cast<uint2*>(dec + (rbs - R) * DEC_BLOCK + dslot) = make_uint2(acc1, acc0);
            }
        };
        for (u32 rb = 0; rb < nb; rb += 2u) {
            u32 rbs = rb;
            asm volatile("" : "+s"(rbs));
            auto rotate = [&](const u32 rbx) {  // one-round launches: the issue priority rotates block by block
                if constexpr (ROT) set_prio((prio_slot + rbx) & 3u);
            };
            rotate(rb);
            __syncthreads();  // every lane is done with the previous table
            prepass(pack_step(sa), pack_step(sb), tab, PL, sel);
            const u32 tn = (rbs + 2u) * 16u + tau;
            sa = load_step<SYM32>(a_sym, tn, tn < a_T);  // prefetch the next 32 steps' symbols
            sb = load_step<SYM32>(b_sym, tn, tn < b_T);
            __syncthreads();
            if (last6 && rb + 1u == nb) steps6(v, A, B, acc0, acc1, tab, L, lane, C);
            else steps16<true>(v, A, B, acc0, acc1, tab, L, lane, C);
            put(rb);
            v = v == 4 ? 0 : v + 1;
            if (rb + 1u < nb) {
                rotate(rb + 1u);
                if (last6 && rb + 2u == nb) steps6(v, A, B, acc0, acc1, tab, L1, lane, C);
                else steps16<true>(v, A, B, acc0, acc1, tab, L1, lane, C);
                put(rb + 1u);
                v = v == 4 ? 0 : v + 1;
            }
        }
    }
    __syncthreads();
#pragma nounroll
    for (u32 i = lane; i < 4u * fstride; i += 64u) img[i] = 0;  // the image aliases the dead table region (two trips for FIC frames)

    // ---- traceback, last part first: lane = (frame fi, block q) ----
#ifdef VIT_DIAG_TIMES
    const unsigned long long diag_t1 = __builtin_amdgcn_s_memrealtime();
#endif
    const u32 fi = lane >> 4;
    const u32 t_fb = fi == 0 ? fbits[0] : fi == 1 ? fbits[1] : fi == 2 ? fbits[2] : fbits[3];
    const u32 t_T = t_fb ? t_fb + VIT_TAIL : 0u;  // steps of this lane's frame
    u32* scratch = reinterpret_cast<u32*>(tab + DEC_BLOCK) + lane * pk_scratch_words(maxfb);  // traceback bit words
    if (fbits[0] == fbits[1] && fbits[1] == fbits[2] && fbits[2] == fbits[3] && (maxfb & 15u) == 0) {
        // ---- fast form (four equally long frames, a multiple of 16 bits): 256-step parts from the top, a window of 17 blocks ----
        u32 hi = T_max, slot0 = R, P16 = P_ZERO;
        for (;;) {
            const u32 lo = hi > 256u + VIT_TAIL ? hi - 256u : VIT_TAIL;
            P16 = traceback_part16(dec, img, fstride, lane, lo, (hi - lo) >> 4, slot0, P16, 0xFFFFFFFFu);
            if (lo == VIT_TAIL) break;
            // the window moves down by d blocks: what stays goes d slots up (every lane moves its own 8 bytes of a block), the
            // d register blocks below come in
            const u32 d = slot0 < DUMP_GROUP ? slot0 : DUMP_GROUP;
            __syncthreads();
            for (u32 sl = DUMP_GROUP; sl >= d; sl--)  // sl = 16 .. d (d >= 1: there are blocks below this part)
                *reinterpret_cast<uint2*>(dec + sl * DEC_BLOCK + dslot) = *reinterpret_cast<const uint2*>(dec + (sl - d) * DEC_BLOCK + dslot);
            const u32 g0 = slot0 - d;
#pragma unroll
            for (u32 b = 0; b < VREG_BLOCKS; b++)
                if (b >= g0 && b < slot0)
                    *reinterpret_cast<uint2*>(dec + (b - g0) * DEC_BLOCK + dslot) = make_uint2(r1[b], r0[b]);
            __syncthreads();
            slot0 = g0;
            hi = lo;
        }
    } else {
    // LDS-resident blocks [R, nb)
    const u32 t_lo = R * 16u;
    u32 warm = TB_WARM;
    u32 P_part = traceback_part(dec, scratch, img, fstride, lane, t_lo > VIT_TAIL ? t_lo : VIT_TAIL, t_T, T_max, R,
                                P_ZERO, warm);
    // register-resident blocks, 16 at a time from the top
    for (u32 g1 = R; g1 > 0;) {
        const u32 g0 = g1 > DUMP_GROUP ? g1 - DUMP_GROUP : 0u;  // group = blocks [g0, g1)
        __syncthreads();
#pragma unroll
        for (u32 b = 0; b < VREG_BLOCKS; b++)
            if (b >= g0 && b < g1)
                *reinterpret_cast<uint2*>(dec + (b - g0) * DEC_BLOCK + dslot) = make_uint2(r1[b], r0[b]);
        __syncthreads();
        const u32 tsg = g0 ? g0 * 16u : VIT_TAIL, tend = g1 * 16u;
        const u32 te = t_T < tend ? t_T : tend, te_max = T_max < tend ? T_max : tend;
        // a frame that reaches beyond this group continues from the position the later part ended in
        const u32 P_top = t_T > tend ? P_part : P_ZERO;
        P_part = traceback_part(dec, scratch, img, fstride, lane, tsg, te, te_max, g0, P_top, warm);
        g1 = g0;
    }
    }
    __syncthreads();

#ifdef VIT_DIAG_TIMES
    diag_times_put(threadIdx.x, blockIdx.x, diag_t0, diag_t1);
#endif
    // bit b of the image is decoded bit b; output bytes are MSB-first (deconvolve.cpp:432-433).  Sixteen lanes per frame,
    // every lane its dwords m = j, j + 16, ...: two trips for a FIC frame (a loop over the frames with 64 lanes each was
    // unrolled eightfold by the compiler: 376 VALU instructions per wave for 4 x 96 bytes).
    {
        const u32 k = lane >> 4, j = lane & 15u;
        const u32 fb_k = k == 0 ? fbits[0] : k == 1 ? fbits[1] : k == 2 ? fbits[2] : fbits[3];
        const size_t oo_k = k == 0 ? ooff[0] : k == 1 ? ooff[1] : k == 2 ? ooff[2] : ooff[3];
        const u32 nbytes = (fb_k + 7u) >> 3;  // a partial last byte is padded with zero bits (ChainBack starts from E = 0)
        uint8_t* o = out + oo_k;
        const u32* im = img + k * fstride;
        if ((((u32)oo_k | nbytes) & 3u) == 0) {
#pragma nounroll
            for (u32 m = j; m < (nbytes >> 2); m += 16u)
                reinterpret_cast<u32*>(o)[m] = __builtin_bswap32(__builtin_bitreverse32(im[m]));
        } else {
#pragma nounroll
            for (u32 b = j; b < nbytes; b += 16u) {
                const u32 byte = (im[b >> 2] >> (8u * (b & 3u))) & 0xFFu;
                o[b] = (uint8_t)(__builtin_bitreverse32(byte) >> 24);
            }
        }
    }
}

constexpr u32 PK_MAX_FRAMEBITS = VIT_MAX_FRAMEBITS;
constexpr u32 PK_SHORT_MAX = SEG_BLOCKS * 16u - VIT_TAIL;  // 778: the longest frame of one segment (49 blocks)

}  // namespace

#ifdef VIT_DIAG_SPEC
extern "C" __attribute__((visibility("default"))) int vit_diag_spec(void* host_buf, int reset) {
    if (reset) {
        unsigned long long z[8] = {};
        return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_diag_spec), z, sizeof z);
    }
    return (int)hipMemcpyFromSymbol(host_buf, HIP_SYMBOL(g_diag_spec), sizeof(unsigned long long) * 8);
}
#endif
#ifdef VIT_DIAG_TIMES
extern "C" __attribute__((visibility("default"))) int vit_diag_times(void* host_buf) {
    return (int)hipMemcpyFromSymbol(host_buf, HIP_SYMBOL(g_diag_times), sizeof(unsigned long long) * 16384 * 4);
}
#endif
bool vit_pk_supported(uint32_t max_framebits) {
    if (max_framebits < 2 || max_framebits > PK_MAX_FRAMEBITS || (max_framebits % 2u) != 0) return false;
    const u32 nblk = (max_framebits + VIT_TAIL + 15u) >> 4;
    return (nblk <= SEG_BLOCKS ? pk_layout(max_framebits) : pk_layout_long(max_framebits)).total <= 160u * 1024u;
}

// Per-thread device scratch of the launcher, grown on demand; its reuse is ordered by an event (a
// thread may alternate between streams).  Layout: [0,256) group counter of the persistent kernel,
// [256,16K) counting-sort bins, then the length-sorted descriptor copy, then the spill slices
// (grid x spill_blocks x 512 B).
struct ScratchCtx {
    void* buf = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    int dev = -1;
    // a split table runs its two kernels side by side: the long-frame kernel goes to `side`, forked from and joined
    // back into the caller's stream with these events
    bool bins_clean = false;  // the sort's histogram in this buffer is zero (the scan kernel leaves it so)
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    void drop_side() {
        if (side) (void)hipStreamDestroy(side);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
        side = nullptr;
        ev_fork = ev_join = nullptr;
    }
    ~ScratchCtx() {
        drop_side();
        if (buf) (void)hipFree(buf);
        if (ev) (void)hipEventDestroy(ev);
    }
};
// one per (thread, device): vit_decode_stream_multi drives every rank from one host thread, and freeing the other
// device's scratch at every step (hipFree = device-wide sync) would serialise its double-buffered pipeline
constexpr int PK_MAX_DEVS = 64;
struct ScratchCtxs {
    ScratchCtx by_dev[PK_MAX_DEVS];
};
thread_local ScratchCtxs t_scratch;
constexpr size_t SCRATCH_HDR = 16384;
constexpr int64_t SORT_MIN_FRAMES = 16;  // below this a table is not worth three extra launches

bool sort_enabled() {
    static const bool on = getenv("VITERBI_AMD_NO_SORT") == nullptr;
    return on;
}

hipError_t vit_launch_pk(const void* d_symbols, bool sym32, uint8_t* d_out, const vit_frame_desc* d_desc,
                         uint32_t framebits, uint32_t max_framebits, int64_t nframes, hipStream_t stream, bool renorm_ge) {
    const u32 rc = pk_renorm_const(renorm_ge);
    const uint8_t* d_sym = static_cast<const uint8_t*>(d_symbols);
    if (sym32 && (reinterpret_cast<uintptr_t>(d_symbols) & 15u)) return hipErrorInvalidValue;  // uint4 loads
    if (nframes <= 0) return hipSuccess;
    if (!vit_pk_supported(max_framebits)) return hipErrorInvalidValue;
    hipError_t e;
    int dev = 0;
    if ((e = hipGetDevice(&dev)) != hipSuccess) return e;
    {  // the dynamic-LDS opt-in is per device
        static uint64_t optin_done = 0;
        const void* ks[6] = {reinterpret_cast<const void*>(vit_pk_kernel<false, false>),
                             reinterpret_cast<const void*>(vit_pk_kernel<true, false>),
                             reinterpret_cast<const void*>(vit_pk_kernel<false, true>),
                             reinterpret_cast<const void*>(vit_pk_kernel<true, true>),
                             reinterpret_cast<const void*>(vit_pk_long_kernel<false>),
                             reinterpret_cast<const void*>(vit_pk_long_kernel<true>)};
        if ((e = vit_optin_dynamic_lds(ks, 6, 160 * 1024, dev, &optin_done)) != hipSuccess) return e;
    }
    const long long groups = (nframes + 3) / 4;
    if (groups > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    const u32 nblk = (max_framebits + VIT_TAIL + 15u) >> 4;
    const bool is_long = nblk > SEG_BLOCKS;
    const bool sort = d_desc != nullptr && nframes >= SORT_MIN_FRAMES && sort_enabled();
    const PkLayout lay = is_long ? pk_layout_long(max_framebits) : pk_layout(max_framebits);
    long long grid = groups;
    if (is_long) {  // the long-frame kernel is persistent: as many workgroups as fit the chip
        u32 per_cu = (160u * 1024u) / lay.total;
        if (per_cu > 16u) per_cu = 16u;  // 4 waves per SIMD (launch bounds)
        grid = (long long)per_cu * vit_device_cus(dev);
        if (grid > groups) grid = groups;
    }
    const bool need_counter = is_long;
    // single-segment kernel: the instantiation with rotating priorities for a launch of one round of waves
    auto launch_short = [&](long long g, const PkLayout& l, u32 vmax, const unsigned* gate, bool may_rotate) {
        u32 per_cu = (160u * 1024u) / l.total;
        if (per_cu > 16u) per_cu = 16u;  // 4 waves per SIMD (launch bounds)
        // (a launch of at most one wave per SIMD has nothing to rotate between, and the s_setprio per block costs it time)
        const bool rot = may_rotate && g <= (long long)per_cu * vit_device_cus(dev) && g > 4ll * vit_device_cus(dev);
#if VIT_FIC_FIXED
        // a uniform batch of FIC frames (no descriptor table, not the gated second launch of a split table): the fixed-geometry
        // instantiation, static LDS.  Forced or chosen, the packed kernel gets here either way.
        if (!d_desc && !gate && framebits == 768u && l.maxfb == 768u) {
#define VIT_LAUNCH_FIXED(S32, R)                                                                                          \
    hipLaunchKernelGGL((vit_pk_fixed_kernel<768u, S32, R>), dim3((unsigned)g), dim3(64), 0, stream, d_sym, d_out, \
                       (long long)nframes, rc)
            if (sym32) {
                if (rot) VIT_LAUNCH_FIXED(true, true);
                else VIT_LAUNCH_FIXED(true, false);
            } else {
                if (rot) VIT_LAUNCH_FIXED(false, true);
                else VIT_LAUNCH_FIXED(false, false);
            }
#undef VIT_LAUNCH_FIXED
            return;
        }
#endif
#define VIT_LAUNCH_SHORT(S32, R)                                                                                          \
    hipLaunchKernelGGL((vit_pk_kernel<S32, R>), dim3((unsigned)g), dim3(64), l.total, stream, d_sym, d_out, d_desc, framebits, \
                       (long long)nframes, l, vmax, gate, rc)
        if (sym32) {
            if (rot) VIT_LAUNCH_SHORT(true, true);
            else VIT_LAUNCH_SHORT(true, false);
        } else {
            if (rot) VIT_LAUNCH_SHORT(false, true);
            else VIT_LAUNCH_SHORT(false, false);
        }
#undef VIT_LAUNCH_SHORT
    };
    if (!need_counter && !sort) {
        launch_short(grid, lay, lay.maxfb, nullptr, true);
        return hipGetLastError();
    }
    const u32 spill_blocks = is_long ? nblk - LONG_KEEP : 0u;
    const size_t desc_bytes = sort ? (((size_t)nframes * sizeof(vit_frame_desc) + 255u) & ~(size_t)255u) : 0u;
    const size_t need = SCRATCH_HDR + desc_bytes + (size_t)grid * spill_blocks * DEC_BLOCK;
    if (dev < 0 || dev >= PK_MAX_DEVS) return hipErrorInvalidDevice;
    ScratchCtx& sc = t_scratch.by_dev[dev];
    if (sc.cap < need) {
        if (sc.buf) (void)hipFree(sc.buf);  // synchronises with the kernels still using it
        sc.buf = nullptr;
        sc.cap = 0;
        sc.bins_clean = false;
        if (sc.ev) (void)hipEventDestroy(sc.ev);
        sc.ev = nullptr;
        if ((e = hipMalloc(&sc.buf, need + need / 4)) != hipSuccess) return e;
        sc.cap = need + need / 4;
        sc.dev = dev;
        if ((e = hipEventCreateWithFlags(&sc.ev, hipEventDisableTiming)) != hipSuccess) return e;
    } else if ((e = hipStreamWaitEvent(stream, sc.ev, 0)) != hipSuccess) {
        return e;
    }
    char* base = static_cast<char*>(sc.buf);
    if (sort) {
        vit_frame_desc* sorted = reinterpret_cast<vit_frame_desc*>(base + SCRATCH_HDR);
        if ((e = vit_sort_descs_launch(d_desc, sorted, nframes, max_framebits, reinterpret_cast<unsigned*>(base + 256),
                                       stream, &sc.bins_clean, reinterpret_cast<unsigned*>(base))) != hipSuccess)
            return e;
        d_desc = sorted;
    }
    unsigned* counter = reinterpret_cast<unsigned*>(base);
    if (need_counter && !sort && (e = hipMemsetAsync(base, 0, 256, stream)) != hipSuccess) return e;  // (the sort's scan kernel clears it)
    if (is_long) {
        // A length-sorted table is split between the two kernels: the long-frame kernel stops at the first group
        // that fits one segment, the single-segment kernel (second launch, same stream) skips the groups before it.
        // That pays only when few frames are long (measured: config 3, 91 % long frames, lost 12 % to the split - the
        // short groups are what levels the tail of the longest-first schedule), so both kernels test the same
        // device-side count: after the sort, bin cursor [98] = number of frames of >= 777 bits.
        const u32 short_max = sort ? PK_SHORT_MAX : 0u;
        const unsigned* gate = sort ? reinterpret_cast<const unsigned*>(base + 256) + VIT_SORT_BINS + ((PK_SHORT_MAX + 7u) >> 3) : nullptr;
        uint2* spill = reinterpret_cast<uint2*>(base + SCRATCH_HDR + desc_bytes);
        // With a split in prospect the long-frame kernel runs on a side stream, forked behind the sort: a handful of
        // long groups cannot fill the chip, the single-segment kernel's workgroups take the rest of it meanwhile.
        hipStream_t ls = stream;
        if (short_max) {
            if (!sc.side) {
                if ((e = hipStreamCreateWithFlags(&sc.side, hipStreamNonBlocking)) != hipSuccess) return e;
                if ((e = hipEventCreateWithFlags(&sc.ev_fork, hipEventDisableTiming)) != hipSuccess) return e;
                if ((e = hipEventCreateWithFlags(&sc.ev_join, hipEventDisableTiming)) != hipSuccess) return e;
            }
            if ((e = hipEventRecord(sc.ev_fork, stream)) != hipSuccess) return e;
            if ((e = hipStreamWaitEvent(sc.side, sc.ev_fork, 0)) != hipSuccess) return e;
            ls = sc.side;
        }
        if (sym32)
            hipLaunchKernelGGL(vit_pk_long_kernel<true>, dim3((unsigned)grid), dim3(64), lay.total, ls, d_sym, d_out,
                               d_desc, framebits, (long long)nframes, lay, spill, spill_blocks, counter, (u32)groups,
                               short_max, gate, rc, 4u * (u32)vit_device_cus(dev));
        else
            hipLaunchKernelGGL(vit_pk_long_kernel<false>, dim3((unsigned)grid), dim3(64), lay.total, ls, d_sym, d_out,
                               d_desc, framebits, (long long)nframes, lay, spill, spill_blocks, counter, (u32)groups,
                               short_max, gate, rc, 4u * (u32)vit_device_cus(dev));
        if (short_max && (e = hipGetLastError()) == hipSuccess) {
            const PkLayout lsh = pk_layout(PK_SHORT_MAX);
            launch_short(groups, lsh, max_framebits, gate, false);  // shares the chip with the long-frame kernel: static priorities
            // join: whatever the caller enqueues next waits for both kernels
            if ((e = hipGetLastError()) != hipSuccess) return e;
            if ((e = hipEventRecord(sc.ev_join, sc.side)) != hipSuccess) return e;
            if ((e = hipStreamWaitEvent(stream, sc.ev_join, 0)) != hipSuccess) return e;
        }
    } else {
        launch_short(grid, lay, lay.maxfb, nullptr, true);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return hipEventRecord(sc.ev, stream);
}
