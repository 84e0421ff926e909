// vit_dab.hip -- what a DAB receiver does right after the Viterbi decoder: undo the energy dispersal (EN 300 401
// clause 10), check the FIBs' CRC-16 (clause 5.2.1) and the DAB+ superframe's fire code (TS 102 563 clause 6), all on
// the device, on the decoder's output in place.
//
// The three definitions are built in (include/viterbi_amd.h, "After the decoder"):
//   PRBS        p_i = p_{i-9} ^ p_{i-5}, p_{-9..-1} = 1 (x^9 + x^5 + 1), restarting at every frame's first bit;
//               decoded bit i (MSB first) ^= p_i; padding bits of a partial last byte stay as they are
//   FIB CRC     CRC-16 0x1021, preset 0xFFFF, MSB first over bytes 0..29, ones' complement in bytes 30..31
//   fire code   0x782F = (x^11 + 1)(x^5 + x^3 + x^2 + x + 1), register 0, remainder of bytes 2..10 == bytes 0..1
//
// Dispersal: one wavefront per frame; lane s owns the s-th aligned dword window that meets the frame.  A window that
// lies wholly inside the frame is one aligned dword load, XOR, store; the (at most two) windows a frame shares with
// its neighbours or with the caller's other data are handled byte by byte, so no byte outside the frame is read or
// written and no dword is ever rewritten across a frame boundary.  The PRBS bytes of an unaligned frame offset come
// from two LDS words and v_alignbyte_b32.  The uniform, the descriptor-table and the DAB+ kernel share this body.
//
// FIBs: one lane per 32-byte FIB.  It loads the FIB once, XORs the PRBS bytes of its position in the frame, stores
// it back, runs a byte-table CRC (256 x u32 in LDS) over bytes 0..29 and writes its flag.
#include "vit_internal.h"

namespace {

typedef uint32_t u32;
typedef uint64_t u64;
constexpr u32 TPB = 256;
constexpr u32 WAVE = 64;
constexpr u32 PRBS_BYTES = VIT_MAX_FRAMEBITS / 8u;  // 1152
constexpr u32 PRBS_WORDS = PRBS_BYTES / 4u + 1u;    // + one zero word: the alignbyte of the last offset reads past it

// PRBS bytes of a frame as little-endian words: byte k of the sequence = bits 8k...8k+7, p_{8k} in the MSB
struct PrbsTab {
    u32 w[PRBS_WORDS];
};
constexpr PrbsTab make_prbs() {
    PrbsTab t{};
    u32 reg = 0x1FFu;  // bit j = p_{i-9+j}: p_{i-9} in bit 0, p_{i-1} in bit 8
    for (u32 i = 0; i < VIT_MAX_FRAMEBITS; i++) {
        const u32 p = (reg ^ (reg >> 4)) & 1u;  // p_{i-9} ^ p_{i-5}
        reg = (reg >> 1) | (p << 8);
        t.w[i >> 5] |= p << (8u * ((i >> 3) & 3u) + 7u - (i & 7u));
    }
    return t;
}
constexpr PrbsTab k_prbs = make_prbs();
static_assert((k_prbs.w[0] & 0xFFFFu) == 0xBE07u, "PRBS must start 0000 0111 1011 1110");
__constant__ PrbsTab c_prbs = k_prbs;

// CRC-16 0x1021 of one byte, register 0 (the FIB CRC's byte table)
constexpr u32 crc16_byte(u32 b) {
    u32 r = b << 8;
    for (int k = 0; k < 8; k++) r = (r & 0x8000u) ? ((r << 1) ^ 0x1021u) & 0xFFFFu : (r << 1) & 0xFFFFu;
    return r;
}

__device__ __forceinline__ void load_prbs(u32* s_prbs) {
    for (u32 i = threadIdx.x; i < PRBS_WORDS; i += TPB) s_prbs[i] = c_prbs.w[i];
}
__device__ __forceinline__ u32 prbs_byte(const u32* s_prbs, u32 k) { return (s_prbs[k >> 2] >> (8u * (k & 3u))) & 0xFFu; }

// Window s of the frame at p (nb bytes, the last one keeping only the bits of `lastmask`): XORs the frame's bytes in
// it with the PRBS and returns them descrambled (little-endian, bytes outside the frame 0).  Window s starts at frame
// byte o = 4s - (p & 3).
__device__ __forceinline__ u32 disperse_window(uint8_t* p, u32 nb, u32 lastmask, u32 s, const u32* s_prbs) {
    const u32 a = (u32)(reinterpret_cast<uintptr_t>(p) & 3u);
    const int o = (int)(4u * s) - (int)a;
    if (o >= 0 && (u32)o + 4u <= nb) {
        const u32 uo = (u32)o;
        u32 x = __builtin_amdgcn_alignbyte(s_prbs[(uo >> 2) + 1u], s_prbs[uo >> 2], uo & 3u);
        const u32 last = nb - 1u - uo;  // the frame's last byte in this window?
        if (last < 4u) x &= ~((0xFFu & ~lastmask) << (8u * last));
        u32* w = reinterpret_cast<u32*>(p + o);  // aligned
        const u32 v = *w ^ x;
        *w = v;
        return v;
    }
    u32 v = 0;
    for (u32 j = 0; j < 4u; j++) {
        const int k = o + (int)j;
        if (k < 0 || (u32)k >= nb) continue;
        u32 x = prbs_byte(s_prbs, (u32)k);
        if ((u32)k == nb - 1u) x &= lastmask;
        const u32 b = p[k] ^ x;
        p[k] = (uint8_t)b;
        v |= b << (8u * j);
    }
    return v;
}
__device__ __forceinline__ u32 frame_bytes(u32 framebits) { return (framebits + 7u) >> 3; }
__device__ __forceinline__ u32 frame_lastmask(u32 framebits) { return (framebits & 7u) ? (0xFF00u >> (framebits & 7u)) & 0xFFu : 0xFFu; }
__device__ __forceinline__ u32 frame_windows(uint8_t* p, u32 nb) {
    return nb ? (u32)((reinterpret_cast<uintptr_t>(p) & 3u) + nb + 3u) >> 2 : 0u;
}

// One wavefront disperses one frame
__device__ __forceinline__ void disperse_frame(uint8_t* p, u32 framebits, u32 lane, const u32* s_prbs) {
    const u32 nb = frame_bytes(framebits), lastmask = frame_lastmask(framebits), nw = frame_windows(p, nb);
    for (u32 s = lane; s < nw; s += WAVE) disperse_window(p, nb, lastmask, s, s_prbs);
}

__global__ __launch_bounds__(TPB) void vit_disperse_kernel(uint8_t* __restrict__ buf, u32 framebits, long long nframes) {
    __shared__ u32 s_prbs[PRBS_WORDS];
    load_prbs(s_prbs);
    __syncthreads();
    const u32 lane = threadIdx.x & (WAVE - 1u), nb = frame_bytes(framebits);
    for (long long f = (long long)blockIdx.x * (TPB / WAVE) + (threadIdx.x / WAVE); f < nframes;
         f += (long long)gridDim.x * (TPB / WAVE))
        disperse_frame(buf + (u64)f * nb, framebits, lane, s_prbs);
}

// Descriptor table: a descriptor whose framebits are odd or above 9216, or whose output bytes reach outside
// [0, out_bytes), is skipped (the checks of vit_check_descs_launch's output side)
__global__ __launch_bounds__(TPB) void vit_disperse_varlen_kernel(uint8_t* __restrict__ buf, u64 out_bytes,
                                                                  const vit_frame_desc* __restrict__ desc, long long nframes) {
    __shared__ u32 s_prbs[PRBS_WORDS];
    load_prbs(s_prbs);
    __syncthreads();
    const u32 lane = threadIdx.x & (WAVE - 1u);
    for (long long i = (long long)blockIdx.x * (TPB / WAVE) + (threadIdx.x / WAVE); i < nframes;
         i += (long long)gridDim.x * (TPB / WAVE)) {
        const u64 oo = desc[i].out_offset;
        const u32 fb = desc[i].framebits;
        if (fb > VIT_MAX_FRAMEBITS || (fb & 1u) || oo > out_bytes || frame_bytes(fb) > out_bytes - oo) continue;
        disperse_frame(buf + oo, fb, lane, s_prbs);
    }
}

// Fire code remainder of bytes 2..10 (register 0, MSB first)
__device__ __forceinline__ u32 fire_remainder(const uint8_t* m9) {
    u32 r = 0;
    for (u32 k = 0; k < 9u; k++) {
        r ^= (u32)m9[k] << 8;
        for (u32 j = 0; j < 8u; j++) r = (r & 0x8000u) ? ((r << 1) ^ 0x782Fu) & 0xFFFFu : (r << 1) & 0xFFFFu;
    }
    return r;
}

// DAB+ post-pass: 5*nsf frames of 24*rsdims bytes, back to back; every frame dispersed, and the first frame of every
// superframe also checked by the fire code on its descrambled bytes 0..10, which lanes 0..3 (windows 0..3) hold
__global__ __launch_bounds__(TPB) void vit_dabplus_post_kernel(uint8_t* __restrict__ work, u32 rsdims, long long nframes,
                                                               uint8_t* __restrict__ fire_ok) {
    __shared__ u32 s_prbs[PRBS_WORDS];
    load_prbs(s_prbs);
    __syncthreads();
    const u32 lane = threadIdx.x & (WAVE - 1u), nb = 24u * rsdims;  // 192*rsdims bits: no padding
    for (long long f = (long long)blockIdx.x * (TPB / WAVE) + (threadIdx.x / WAVE); f < nframes;
         f += (long long)gridDim.x * (TPB / WAVE)) {
        uint8_t* p = work + (u64)f * nb;
        const u32 nw = frame_windows(p, nb);  // >= 7: windows 0..3 in the first round
        for (u32 s0 = 0; s0 < nw; s0 += WAVE) {
            const u32 s = s0 + lane;
            const u32 v = s < nw ? disperse_window(p, nb, 0xFFu, s, s_prbs) : 0u;
            if (s0 == 0 && fire_ok && f % 5 == 0) {  // wave-uniform
                const u32 a = (u32)(reinterpret_cast<uintptr_t>(p) & 3u);
                const u32 v0 = __shfl(v, 0), v1 = __shfl(v, 1), v2 = __shfl(v, 2), v3 = __shfl(v, 3);
                const u32 h[3] = {__builtin_amdgcn_alignbyte(v1, v0, a), __builtin_amdgcn_alignbyte(v2, v1, a),
                                  __builtin_amdgcn_alignbyte(v3, v2, a)};
                uint8_t b[12];
                __builtin_memcpy(b, h, 12);
                if (lane == 0) fire_ok[f / 5] = fire_remainder(b + 2) == ((u32)b[0] << 8 | b[1]) ? 1 : 0;
            }
        }
    }
}

// FIBs: nfibs blocks of 32 bytes at fibs + 32*i (any alignment); FIB i is FIB (i mod fpf) of its frame.
// descramble: XOR in PRBS bytes 32*(i mod fpf) ... 32*(i mod fpf) + 31 and store the FIB back before the CRC.
static_assert(TPB == 256, "vit_fib_kernel: one CRC table entry per thread");
__global__ __launch_bounds__(TPB) void vit_fib_kernel(uint8_t* __restrict__ fibs, long long nfibs, u32 fpf, bool descramble,
                                                      uint8_t* __restrict__ ok) {
    __shared__ u32 s_prbs[PRBS_WORDS];
    __shared__ u32 s_crc[256];
    if (descramble) load_prbs(s_prbs);
    s_crc[threadIdx.x] = crc16_byte(threadIdx.x);
    __syncthreads();
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < nfibs; i += (long long)gridDim.x * TPB) {
        uint8_t* p = fibs + (u64)i * 32u;
        u32 w[8];
        __builtin_memcpy(w, p, 32);
        if (descramble) {
            const u32 k = 8u * (u32)((u64)i % fpf);
#pragma unroll
            for (u32 j = 0; j < 8u; j++) w[j] ^= s_prbs[k + j];
            __builtin_memcpy(p, w, 32);
        }
        u32 crc = 0xFFFFu;
#pragma unroll
        for (u32 j = 0; j < 30u; j++) {
            const u32 b = (w[j >> 2] >> (8u * (j & 3u))) & 0xFFu;
            crc = ((crc << 8) ^ s_crc[((crc >> 8) ^ b) & 0xFFu]) & 0xFFFFu;
        }
        const u32 stored = ((w[7] >> 16) & 0xFFu) << 8 | (w[7] >> 24);
        ok[i] = (crc ^ 0xFFFFu) == stored ? 1 : 0;
    }
}

unsigned grid_for(long long items, u32 per_block) {
    const long long b = (items + per_block - 1) / per_block;
    return (unsigned)(b < (1 << 20) ? b : (1 << 20));
}

}  // namespace

int64_t vit_prbs_bytes_host(uint8_t* h_out, uint32_t framebits) {
    const uint32_t nb = (framebits + 7u) >> 3;
    for (uint32_t k = 0; k < nb; k++) h_out[k] = (uint8_t)(k_prbs.w[k >> 2] >> (8u * (k & 3u)));
    if (framebits & 7u) h_out[nb - 1] &= (uint8_t)(0xFF00u >> (framebits & 7u));
    return nb;
}

hipError_t vit_launch_disperse(uint8_t* d_bytes, uint32_t framebits, int64_t nframes, hipStream_t stream) {
    if (nframes <= 0 || framebits == 0) return hipSuccess;
    hipLaunchKernelGGL(vit_disperse_kernel, dim3(grid_for(nframes, TPB / WAVE)), dim3(TPB), 0, stream, d_bytes, framebits,
                       (long long)nframes);
    return hipGetLastError();
}

hipError_t vit_launch_disperse_varlen(uint8_t* d_bytes, uint64_t out_bytes, const vit_frame_desc* d_desc, int64_t nframes,
                                      hipStream_t stream) {
    if (nframes <= 0) return hipSuccess;
    hipLaunchKernelGGL(vit_disperse_varlen_kernel, dim3(grid_for(nframes, TPB / WAVE)), dim3(TPB), 0, stream, d_bytes,
                       (u64)out_bytes, d_desc, (long long)nframes);
    return hipGetLastError();
}

hipError_t vit_launch_fibs(uint8_t* d_fibs, int64_t nfibs, uint32_t fibs_per_frame, bool descramble, uint8_t* d_ok,
                           hipStream_t stream) {
    if (nfibs <= 0) return hipSuccess;
    hipLaunchKernelGGL(vit_fib_kernel, dim3(grid_for(nfibs, TPB)), dim3(TPB), 0, stream, d_fibs, (long long)nfibs,
                       fibs_per_frame ? fibs_per_frame : 1u, descramble, d_ok);
    return hipGetLastError();
}

hipError_t vit_launch_dabplus_post(uint8_t* d_work, uint32_t rsdims, int64_t nsf, uint8_t* d_fire_ok, hipStream_t stream) {
    if (nsf <= 0) return hipSuccess;
    const long long nframes = 5ll * nsf;
    hipLaunchKernelGGL(vit_dabplus_post_kernel, dim3(grid_for(nframes, TPB / WAVE)), dim3(TPB), 0, stream, d_work, rsdims,
                       nframes, d_fire_ok);
    return hipGetLastError();
}
