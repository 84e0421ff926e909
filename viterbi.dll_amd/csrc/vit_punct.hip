// vit_punct.hip -- depuncturing on the device: a punctured stream (transmitted symbols only, one byte each) expanded
// into the decoder's u8 device format, the punctured positions filled with the caller's erasure value.
//
// EN 300 401 clause 11 thins the K=7 rate-1/4 mother code by 32-bit puncturing vectors; a profile
// (include/viterbi_amd.h: vit_punct_profile) writes them as per-segment period-8-step keep masks.  The expansion is a
// separate pass in front of the unchanged decoders (vit_api_decode.hip), like the u32 path's narrowing (vit_pack_kernel).
//
// One lane per trellis step writes that step's output dword, so a wavefront stores 256 contiguous bytes.  A step's
// first transmitted byte is
//     base[seg] + (k / 8) * popc(keep) + popc(keep & ((1 << 4 * (k % 8)) - 1))       (k = step within the segment)
// and its (at most four) transmitted bytes arrive in ONE dword load: unaligned, and clamped to end at the frame's
// last byte, so no byte outside the frame's [first, first + P) is ever read (frames of fewer than 4 bytes take byte
// loads).  v_perm_b32 then places them against a word of erasure bytes.
//
// Uniform batch (one profile): every workgroup first tabulates the frame's T steps in LDS (offset + keep nibble per
// step; the segment is found with a wave-uniform loop over at most 8 segments whose start steps and byte bases the
// host computed), then streams the flat step index of the whole batch with four steps per lane in flight - one load
// per lane at a time leaves the pass latency-bound.  Variable-length batch: one workgroup per frame, each lane
// computes its steps directly (a table would cost as much as the frame).
#include "vit_internal.h"
#include "vit_punct_dev.h"

namespace {

typedef uint32_t u32;
typedef uint64_t u64;
constexpr u32 TPB = 256;

// The step's transmitted bytes, packed from byte 0 (off + popc(nib) <= P).  `in` = the frame's first transmitted byte.
__device__ __forceinline__ u32 gather(const uint8_t* __restrict__ in, u32 P, u32 off, u32 nib) {
    u32 w = 0;
    if (nib) {
        if (P >= 4u) {
            const u32 a = off < P - 4u ? off : P - 4u;  // the dword ends inside the frame
            u32 v;
            __builtin_memcpy(&v, in + a, 4);  // unaligned global_load_dword
            w = v >> (8u * (off - a));
        } else {
            const u32 cnt = __builtin_popcount(nib);
            for (u32 j = 0; j < cnt; j++) w |= (u32)in[off + j] << (8u * j);
        }
    }
    return w;
}

constexpr u32 STEPS_PER_LANE = 4;

// Uniform batch: frame f's transmitted bytes at f*P, its expanded symbols at f*4*T; the steps of all frames are one
// flat index.  rcpT = 1/T (host float); step tables: stab[t] = offset | nib << 16 (P <= 4*9222 < 2^16).
__global__ __launch_bounds__(TPB) void vit_depunct_kernel(const uint8_t* __restrict__ in, u32* __restrict__ out, SegTab tab,
                                                          u32 T, u32 P, float rcpT, u64 total_steps, u32 erasure4) {
    extern __shared__ u32 stab[];  // T entries
    __shared__ u32 seltab[16];
    for (u32 t = threadIdx.x; t < T; t += TPB) {
        u32 off, nib;
        locate(t, tab, off, nib);
        stab[t] = off | nib << 16;
    }
    if (threadIdx.x < 16) seltab[threadIdx.x] = expand_sel(threadIdx.x);
    __syncthreads();
    constexpr u32 CHUNK = TPB * STEPS_PER_LANE;
    for (u64 g0 = (u64)blockIdx.x * CHUNK; g0 < total_steps; g0 += (u64)gridDim.x * CHUNK) {
        const u64 f0 = g0 / T;  // block-uniform
        const u32 r0 = (u32)(g0 - f0 * T);
        u32 w[STEPS_PER_LANE], e[STEPS_PER_LANE];
#pragma unroll
        for (u32 j = 0; j < STEPS_PER_LANE; j++) {  // all loads first
            const u32 tl = r0 + threadIdx.x + j * TPB;  // < T + CHUNK: exact in float
            u32 df = (u32)((float)tl * rcpT);
            int t = (int)(tl - df * T);
            if (t < 0) { t += (int)T; df--; }
            if (t >= (int)T) { t -= (int)T; df++; }
            const bool live = g0 + threadIdx.x + j * TPB < total_steps;
            e[j] = live ? stab[t] : 0u;
            w[j] = live ? gather(in + (f0 + df) * P, P, e[j] & 0xFFFFu, e[j] >> 16) : 0u;
        }
#pragma unroll
        for (u32 j = 0; j < STEPS_PER_LANE; j++) {
            const u64 g = g0 + threadIdx.x + j * TPB;
            if (g < total_steps) out[g] = __builtin_amdgcn_perm(erasure4, w[j], seltab[e[j] >> 16]);
        }
    }
}

// Variable-length batch: one block per frame.  Validates the descriptor and its profile (all block-uniform), writes
// the internal descriptor (slot offset, the caller's out_offset, framebits - or 0xFFFFFFFF, an odd length every
// decoder skips) and expands the frame into its slot.
__global__ __launch_bounds__(TPB) void vit_depunct_varlen_kernel(const uint8_t* __restrict__ in, u64 sym_bytes, u64 out_bytes,
                                                                 const vit_frame_desc* __restrict__ desc, long long nframes,
                                                                 u32 max_framebits, const vit_punct_profile* __restrict__ prof,
                                                                 u32 nprof, u32 erasure4, uint8_t* __restrict__ slots,
                                                                 vit_frame_desc* __restrict__ idesc) {
    const u64 slot_bytes = 4ull * (max_framebits + VIT_TAIL);
    for (long long i = blockIdx.x; i < nframes; i += gridDim.x) {
        const vit_frame_desc d = desc[i];
        const u32 fb = d.framebits, T = fb + VIT_TAIL;
        bool ok = fb <= max_framebits && (fb & 1u) == 0 && d.reserved < nprof &&
                  d.out_offset <= out_bytes && ((fb + 7u) >> 3) <= out_bytes - d.out_offset;
        SegTab tab;
        u32 P = 0;
        if (ok) {
            const vit_punct_profile* p = prof + d.reserved;
            tab.nsegs = p->nsegs;
            ok = tab.nsegs >= 1u && tab.nsegs <= VIT_PUNCT_MAX_SEGS;
            u64 steps = 0, bytes = 0;
#pragma unroll
            for (u32 k = 0; k < VIT_PUNCT_MAX_SEGS; k++) {
                const u32 n = k < tab.nsegs ? p->seg[k].steps : 0u, keep = k < tab.nsegs ? p->seg[k].keep : 0u;
                if (k < tab.nsegs && n == 0) ok = false;
                tab.start[k] = (u32)steps;
                tab.base[k] = (u32)bytes;
                tab.keep[k] = keep;
                steps += n;
                bytes += (u64)(n >> 3) * __builtin_popcount(keep) + __builtin_popcount(keep & ((1u << (4u * (n & 7u))) - 1u));
                if (steps > T) ok = false;  // (also keeps start/base inside 32 bits)
            }
            ok = ok && steps == T;
            P = (u32)bytes;
            ok = ok && d.sym_offset <= sym_bytes && P <= sym_bytes - d.sym_offset;
        }
        if (threadIdx.x == 0) {
            vit_frame_desc o;
            o.sym_offset = (u64)i * slot_bytes;
            o.out_offset = d.out_offset;
            o.framebits = ok ? fb : 0xFFFFFFFFu;
            o.reserved = 0;
            idesc[i] = o;
        }
        if (!ok) continue;
        const uint8_t* fin = in + d.sym_offset;
        u32* fout = reinterpret_cast<u32*>(slots + (u64)i * slot_bytes);
        for (u32 t = threadIdx.x; t < T; t += TPB) {
            u32 off, nib;
            locate(t, tab, off, nib);
            fout[t] = __builtin_amdgcn_perm(erasure4, gather(fin, P, off, nib), expand_sel(nib));
        }
    }
}

u32 erasure_word(uint8_t e) { return 0x01010101u * e; }

}  // namespace

int64_t vit_punct_length_host(const vit_punct_profile* p, uint32_t framebits, uint32_t* start, uint32_t* base) {
    if (!p || p->nsegs < 1u || p->nsegs > VIT_PUNCT_MAX_SEGS) return -1;
    uint64_t steps = 0, bytes = 0;
    for (uint32_t k = 0; k < p->nsegs; k++) {
        const uint32_t n = p->seg[k].steps, keep = p->seg[k].keep;
        if (n == 0) return -1;
        if (start) start[k] = (uint32_t)steps;
        if (base) base[k] = (uint32_t)bytes;
        steps += n;
        bytes += (uint64_t)(n >> 3) * __builtin_popcount(keep) + __builtin_popcount(keep & ((1u << (4u * (n & 7u))) - 1u));
        if (steps > (uint64_t)framebits + VIT_TAIL) return -1;
    }
    return steps == (uint64_t)framebits + VIT_TAIL ? (int64_t)bytes : -1;
}

hipError_t vit_launch_depunct(const uint8_t* d_punct, uint8_t* d_sym8, uint32_t framebits, int64_t nframes,
                              const vit_punct_profile* profile, uint8_t erasure, hipStream_t stream) {
    SegTab tab = {};
    const int64_t P = vit_punct_length_host(profile, framebits, tab.start, tab.base);
    if (P < 0) return hipErrorInvalidValue;
    if (nframes <= 0) return hipSuccess;
    tab.nsegs = profile->nsegs;
    for (uint32_t k = 0; k < tab.nsegs; k++) tab.keep[k] = profile->seg[k].keep;
    const uint32_t T = framebits + VIT_TAIL;
    const u64 total = (u64)nframes * T;
    // persistent-ish grid: every workgroup tabulates the frame's steps once, then strides over the batch
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const u64 chunk = (u64)TPB * STEPS_PER_LANE;
    const u64 blocks = (total + chunk - 1) / chunk, cap = 8ull * (u64)vit_device_cus(dev);
    const unsigned grid = (unsigned)(blocks < cap ? blocks : cap);
    hipLaunchKernelGGL(vit_depunct_kernel, dim3(grid), dim3(TPB), (size_t)T * sizeof(u32), stream, d_punct,
                       reinterpret_cast<u32*>(d_sym8), tab, T, (u32)P, 1.0f / (float)T, total, erasure_word(erasure));
    return hipGetLastError();
}

hipError_t vit_launch_depunct_varlen(const uint8_t* d_punct, uint64_t sym_bytes, uint64_t out_bytes, const vit_frame_desc* d_desc,
                                     int64_t nframes, uint32_t max_framebits, const vit_punct_profile* d_profiles,
                                     uint32_t nprofiles, uint8_t erasure, uint8_t* d_slots, vit_frame_desc* d_idesc,
                                     hipStream_t stream) {
    if (nframes <= 0) return hipSuccess;
    const unsigned grid = (unsigned)(nframes < (1 << 20) ? nframes : (1 << 20));
    hipLaunchKernelGGL(vit_depunct_varlen_kernel, dim3(grid), dim3(TPB), 0, stream, d_punct, (u64)sym_bytes, (u64)out_bytes,
                       d_desc, (long long)nframes, max_framebits, d_profiles, nprofiles, erasure_word(erasure), d_slots, d_idesc);
    return hipGetLastError();
}
