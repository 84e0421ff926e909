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
#include "vit_crc_dev.h"
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
__host__ __device__ __forceinline__ u32 fire_remainder(const uint8_t* m9) {
    u32 r = 0;
    for (u32 k = 0; k < 9u; k++) {
        r ^= (u32)m9[k] << 8;
        for (u32 j = 0; j < 8u; j++) r = (r & 0x8000u) ? ((r << 1) ^ 0x782Fu) & 0xFFFFu : (r << 1) & 0xFFFFu;
    }
    return r;
}

// vit_dabplus_post_kernel's loop body for vit_ens_post_kernel (the former keeps its own text, so that its code is what it
// was): one wavefront descrambles the frame of nb whole bytes at p; if `fire` (wave-uniform) the frame is a superframe's
// first (nb >= 24: windows 0..3 in the first round) and *flag receives the fire code of its descrambled bytes 0..10,
// which lanes 0..3 (windows 0..3) hold.
__device__ __forceinline__ void post_frame(uint8_t* p, u32 nb, u32 lane, const u32* s_prbs, bool fire, uint8_t* flag) {
    const u32 nw = frame_windows(p, nb);
    for (u32 s0 = 0; s0 < nw; s0 += WAVE) {
        const u32 s = s0 + lane;
        const u32 v = s < nw ? disperse_window(p, nb, 0xFFu, s, s_prbs) : 0u;
        if (s0 == 0 && fire) {
            const u32 a = (u32)(reinterpret_cast<uintptr_t>(p) & 3u);
            const u32 v0 = __shfl(v, 0), v1 = __shfl(v, 1), v2 = __shfl(v, 2), v3 = __shfl(v, 3);
            const u32 h[3] = {__builtin_amdgcn_alignbyte(v1, v0, a), __builtin_amdgcn_alignbyte(v2, v1, a),
                              __builtin_amdgcn_alignbyte(v3, v2, a)};
            uint8_t b[12];
            __builtin_memcpy(b, h, 12);
            if (lane == 0) *flag = fire_remainder(b + 2) == ((u32)b[0] << 8 | b[1]) ? 1 : 0;
        }
    }
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

// ---- DAB+ access units (TS 102 563 clause 5.2): superframe header, AU CRCs ---------------------------------------
// crc16_step (vit_crc_dev.h): CRC-16 0x1021 over one byte without a table
static_assert(crc16_step(0, 1) == crc16_byte(1) && crc16_step(0, 0xA7) == crc16_byte(0xA7) && crc16_step(0x1234, 0) ==
              (crc16_byte(0x12) ^ 0x3400u), "the table-less byte step is the table's");

constexpr u32 AU_MAX_L = 110u * 48u;                // the longest superframe
constexpr u32 AU_MAX_CHUNK = (AU_MAX_L + 63u) / 64u;  // bytes of one lane's chunk of the longest AU
constexpr u32 AU_POW_N = 63u * AU_MAX_CHUNK + 1u;
// x^(8e) mod g for e = 0 ... 63 * 83: what a chunk's remainder is multiplied by when e bytes follow it
struct AuPowTab {
    uint16_t v[AU_POW_N];
};
constexpr AuPowTab make_au_pow() {
    AuPowTab t{};
    u32 r = 1;
    for (u32 e = 0; e < AU_POW_N; e++) {
        t.v[e] = (uint16_t)r;
        r = crc16_step(r, 0);
    }
    return t;
}
__device__ const AuPowTab d_au_pow = make_au_pow();
// the fire code's remainder of a 72-bit message (bytes 2..10, MSB first) with only bit t set
struct FireBitTab {
    uint16_t v[72];
};
constexpr FireBitTab make_fire_bits() {
    FireBitTab t{};
    u32 r = 0x782Fu;  // x^16 mod g: the last bit
    for (int k = 71; k >= 0; k--) {
        t.v[k] = (uint16_t)r;
        r = (r & 0x8000u) ? ((r << 1) ^ 0x782Fu) & 0xFFFFu : (r << 1) & 0xFFFFu;
    }
    return t;
}
__device__ const FireBitTab d_fire_bits = make_fire_bits();

// The header of a superframe of L bytes from its bytes 2..10 (include/viterbi_amd.h): start[0 .. num_aus], unused
// entries 0; valid when every AU has at least 3 bytes.
struct AuHeader {
    u32 num_aus, valid, start[7];
};
__host__ __device__ __forceinline__ AuHeader au_parse(const u32* b /* bytes 0..10 */, u32 L) {
    AuHeader h;
    const u32 dac = (b[2] >> 6) & 1u, sbr = (b[2] >> 5) & 1u;
    h.num_aus = sbr ? (dac ? 3u : 2u) : (dac ? 6u : 4u);
    const u32 f[7] = {sbr ? (dac ? 6u : 5u) : (dac ? 11u : 8u),
                      b[3] << 4 | b[4] >> 4,
                      (b[4] & 15u) << 8 | b[5],
                      b[6] << 4 | b[7] >> 4,
                      (b[7] & 15u) << 8 | b[8],
                      b[9] << 4 | b[10] >> 4,
                      0u};
    h.valid = 1u;
#pragma unroll
    for (u32 n = 0; n < 7u; n++) h.start[n] = n < h.num_aus ? f[n] : n == h.num_aus ? L : 0u;
#pragma unroll
    for (u32 n = 0; n < 6u; n++)
        if (n < h.num_aus && (int)h.start[n + 1] - (int)h.start[n] < 3) h.valid = 0u;
    return h;
}
// The record as its five little-endian dwords
__host__ __device__ __forceinline__ void au_record(u32* w, u32 status, const AuHeader& h, u32 param, u32 crc_ok, u32 fire_ok) {
    w[0] = status | h.num_aus << 8 | param << 16 | crc_ok << 24;
    w[1] = h.start[0] | h.start[1] << 16;
    w[2] = h.start[2] | h.start[3] << 16;
    w[3] = h.start[4] | h.start[5] << 16;
    w[4] = h.start[6] | fire_ok << 16;
}

// XOR over the wavefront, the result in every lane: two quad permutes, the two row mirrors, then the rows' results
// collected in lane 63 by row_bcast15 / row_bcast31
__device__ __forceinline__ u32 wave_xor(u32 v) {
    v ^= (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);   // quad_perm [1,0,3,2]
    v ^= (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
    v ^= (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false);  // row_half_mirror
    v ^= (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false);  // row_mirror
    v ^= (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);  // row_bcast15 into rows 1 and 3
    v ^= (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);  // row_bcast31 into rows 2 and 3
    return (u32)__builtin_amdgcn_readlane((int)v, 63);
}

// One wavefront per superframe, AU_WPB per workgroup.  The superframe comes in as aligned 16-byte windows (the windows
// it shares with its neighbours byte by byte, so nothing outside its L bytes is read) into the wavefront's LDS image,
// byte k at s[(p & 15) + k].  Header and fire code: lane t takes message bit t (and lanes 0..7 bits 64..71) times the
// bit's remainder, XORed over the wavefront.  Each AU: lane i takes the register-0 remainder r_i of the i-th of 64
// chunks of c = ceil(len/64) bytes, right-aligned (the leading chunks of a short AU are empty or short; leading zeros
// do not change a register-0 remainder), the lane that holds the AU's first byte starting from the preset 0xFFFF
// instead of 0; the AU's CRC register is XOR_i r_i * x^(8c(63-i)) mod g: one carry-less 16 x 16 multiply per lane by
// d_au_pow[c(63-i)], an XOR over the wavefront of the 31-bit products, one reduction mod g.
constexpr u32 AU_WPB = TPB / WAVE;
__host__ __device__ constexpr u32 au_lds_bytes(u32 L) { return ((L + 30u) >> 4) << 4; }  // windows of (15 + L) bytes

// The two halves of vit_au_kernel's loop body, for vit_au_table_kernel: the superframe of L bytes at p into the wavefront's
// image s (a = p & 15), and its record from the image (m = s + a: the superframe's byte 0; fbit / fbit2: the lane's
// fire-code remainders) to the five dwords at rec.  vit_au_kernel keeps its own text of them, by measurement
// (profiles/r19_front_isa_same.txt): once it calls these functions too, the compiler gives au_load the callers' common
// range of L, and either the table kernel comes out 30 instructions longer and 0.7 % slower in bench_ensemble's table
// launches (L = 110u * rsdims there), or vit_au_kernel itself 0.7 % slower in bench_au (L from a 16-bit rsdims).
__device__ __forceinline__ void au_load(const uint8_t* p, u32 L, u32 a, uint8_t* s, u32 lane) {
    const u32 nwin = (a + L + 15u) >> 4;
    for (u32 w = lane; w < nwin; w += WAVE) {
        const int o = (int)(16u * w) - (int)a;
        if (o >= 0 && (u32)o + 16u <= L) {
            *reinterpret_cast<uint4*>(s + 16u * w) = *reinterpret_cast<const uint4*>(p + o);
        } else {
            for (u32 j = 0; j < 16u; j++) {
                const int k = o + (int)j;
                if (k >= 0 && (u32)k < L) s[16u * w + j] = p[k];
            }
        }
    }
}
__device__ __forceinline__ void au_eval(const uint8_t* m, u32 L, u32 lane, u32 fbit, u32 fbit2, u32* rec) {
    // bytes 0..10 into scalars through lanes 0..10
    const u32 hb = m[lane < 11u ? lane : 0u];
    u32 b[11];
#pragma unroll
    for (u32 k = 0; k < 11u; k++) b[k] = (u32)__builtin_amdgcn_readlane((int)hb, k);
    const AuHeader h = au_parse(b, L);
    u32 fv = ((m[2u + (lane >> 3)] >> (7u - (lane & 7u))) & 1u) ? fbit : 0u;
    fv ^= ((b[10] >> (7u - (lane & 7u))) & 1u) ? fbit2 : 0u;
    const u32 fire_ok = wave_xor(fv) == (b[0] << 8 | b[1]) ? 1u : 0u;
    u32 crc_ok = 0;
    if (h.valid) {
#pragma unroll
        for (u32 n = 0; n < 6u; n++) {
            if (n >= h.num_aus) break;  // wave-uniform
            const u32 len = h.start[n + 1] - h.start[n] - 2u;  // >= 1 bytes under the CRC
            const uint8_t* q = m + h.start[n];
            const u32 c = (len + 63u) >> 6;
            const int lo = (int)len - (int)((64u - lane) * c), hi = lo + (int)c;
            u32 r = (lo <= 0 && hi > 0) ? 0xFFFFu : 0u;
            for (int k = lo > 0 ? lo : 0; k < hi; k++) r = crc16_step(r, q[k]);
            const u32 x = d_au_pow.v[(63u - lane) * c];
            u32 prod = 0;
#pragma unroll
            for (u32 j = 0; j < 16u; j++) prod ^= ((x >> j) & 1u) ? r << j : 0u;
            prod = wave_xor(prod);
            const u32 crc = (prod & 0xFFFFu) ^ crc16_step(crc16_step(prod >> 16, 0), 0);
            const u32 stored = (u32)q[len] << 8 | q[len + 1u];
            if ((crc ^ 0xFFFFu) == stored) crc_ok |= 1u << n;
        }
    }
    if (lane < 5u) {
        u32 w[5];
        au_record(w, h.valid ? VIT_AU_OK : VIT_AU_BAD_HEADER, h, b[2], crc_ok, fire_ok);
        rec[lane] = lane == 0u ? w[0] : lane == 1u ? w[1] : lane == 2u ? w[2] : lane == 3u ? w[3] : w[4];
    }
}

__global__ __launch_bounds__(TPB) void vit_au_kernel(const uint8_t* __restrict__ sf, u64 stride, u32 rsdims, long long nsf,
                                                     const int32_t* __restrict__ ret, u32* __restrict__ au) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_au[];
    const u32 lane = threadIdx.x & (WAVE - 1u), wave = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    const u32 L = 110u * rsdims;
    uint8_t* s = s_au + wave * au_lds_bytes(L);
    const u32 fbit = d_fire_bits.v[lane], fbit2 = lane < 8u ? d_fire_bits.v[64u + lane] : 0u;
    // every wavefront of a workgroup makes the same number of rounds: the barriers order the LDS image's writes and reads
    for (long long f0 = (long long)blockIdx.x * AU_WPB; f0 < nsf; f0 += (long long)gridDim.x * AU_WPB) {
        const long long f = f0 + wave;
        const bool live = f < nsf;                                  // wave-uniform
        const bool read = live && !(ret && ret[live ? f : 0] < 0);  // RS gave up: the superframe is not read
        const uint8_t* p = sf + (u64)(live ? f : 0) * stride;
        const u32 a = (u32)(reinterpret_cast<uintptr_t>(p) & 15u);
        if (read) {
            const u32 nwin = (a + L + 15u) >> 4;
            for (u32 w = lane; w < nwin; w += WAVE) {
                const int o = (int)(16u * w) - (int)a;
                if (o >= 0 && (u32)o + 16u <= L) {
                    *reinterpret_cast<uint4*>(s + 16u * w) = *reinterpret_cast<const uint4*>(p + o);
                } else {
                    for (u32 j = 0; j < 16u; j++) {
                        const int k = o + (int)j;
                        if (k >= 0 && (u32)k < L) s[16u * w + j] = p[k];
                    }
                }
            }
        }
        __syncthreads();
        if (read) {
            const uint8_t* m = s + a;  // the superframe's byte 0
            // bytes 0..10 into scalars through lanes 0..10
            const u32 hb = m[lane < 11u ? lane : 0u];
            u32 b[11];
#pragma unroll
            for (u32 k = 0; k < 11u; k++) b[k] = (u32)__builtin_amdgcn_readlane((int)hb, k);
            const AuHeader h = au_parse(b, L);
            u32 fv = ((m[2u + (lane >> 3)] >> (7u - (lane & 7u))) & 1u) ? fbit : 0u;
            fv ^= ((b[10] >> (7u - (lane & 7u))) & 1u) ? fbit2 : 0u;
            const u32 fire_ok = wave_xor(fv) == (b[0] << 8 | b[1]) ? 1u : 0u;
            u32 crc_ok = 0;
            if (h.valid) {
#pragma unroll
                for (u32 n = 0; n < 6u; n++) {
                    if (n >= h.num_aus) break;  // wave-uniform
                    const u32 len = h.start[n + 1] - h.start[n] - 2u;  // >= 1 bytes under the CRC
                    const uint8_t* q = m + h.start[n];
                    const u32 c = (len + 63u) >> 6;
                    const int lo = (int)len - (int)((64u - lane) * c), hi = lo + (int)c;
                    u32 r = (lo <= 0 && hi > 0) ? 0xFFFFu : 0u;
                    for (int k = lo > 0 ? lo : 0; k < hi; k++) r = crc16_step(r, q[k]);
                    const u32 x = d_au_pow.v[(63u - lane) * c];
                    u32 prod = 0;
#pragma unroll
                    for (u32 j = 0; j < 16u; j++) prod ^= ((x >> j) & 1u) ? r << j : 0u;
                    prod = wave_xor(prod);
                    const u32 crc = (prod & 0xFFFFu) ^ crc16_step(crc16_step(prod >> 16, 0), 0);
                    const u32 stored = (u32)q[len] << 8 | q[len + 1u];
                    if ((crc ^ 0xFFFFu) == stored) crc_ok |= 1u << n;
                }
            }
            if (lane < 5u) {
                u32 w[5];
                au_record(w, h.valid ? VIT_AU_OK : VIT_AU_BAD_HEADER, h, b[2], crc_ok, fire_ok);
                au[5u * (u64)f + lane] = lane == 0u ? w[0] : lane == 1u ? w[1] : lane == 2u ? w[2] : lane == 3u ? w[3] : w[4];
            }
        } else if (live && lane < 5u) {
            au[5u * (u64)f + lane] = lane == 0u ? (u32)VIT_AU_RS_FAILED : 0u;
        }
        __syncthreads();  // the image is read before the next round overwrites it
    }
}

// One lane per candidate: bytes 0..1 at bytes + i*stride against the fire remainder of bytes 2..10 there
__global__ __launch_bounds__(TPB) void vit_fire_kernel(const uint8_t* __restrict__ bytes, u64 stride, long long n,
                                                       uint8_t* __restrict__ ok) {
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long long)gridDim.x * TPB) {
        const uint8_t* p = bytes + (u64)i * stride;
        uint8_t b[11];
#pragma unroll
        for (u32 k = 0; k < 11u; k++) b[k] = p[k];
        ok[i] = fire_remainder(b + 2) == ((u32)b[0] << 8 | b[1]) ? 1 : 0;
    }
}

// ---- a whole ensemble (vit_internal.h, VitEnsTable): the table forms of the kernels above -----------------------------
// The descriptor of every frame of the table: frame j of sub-channel k is frame phase + j of the de-interleaved span
// (`span` bytes per frame), sym0 bytes in, and framebits/8 bytes of the sub-channel's block in d_work.
__global__ __launch_bounds__(TPB) void vit_ens_desc_kernel(const VitEnsTable tab, const VitEnsSource src, u64 span,
                                                           vit_frame_desc* __restrict__ desc) {
    const u32 i = blockIdx.x * TPB + threadIdx.x;
    if (i >= tab.nframes) return;
    const u32 k = vit_ens_find<&VitEnsEntry::frame0>(tab, i), j = i - tab.e[k].frame0, fb = tab.e[k].framebits;
    vit_frame_desc d;
    d.sym_offset = ((u64)src.phase[k] + j) * span + src.sym0[k];
    d.out_offset = tab.e[k].work_off + (u64)j * (fb >> 3);
    d.framebits = fb;
    d.reserved = src.profile[k];
    desc[i] = d;
}

// vit_dabplus_post_kernel over the table: one wavefront per frame, all sub-channels (one that is not DAB+ is descrambled
// only).  A frame the expansion skipped (idesc[i].framebits 0xFFFFFFFF) keeps its bytes, and its fire code, if it is a
// superframe's first, is that of the bytes as they are.
__global__ __launch_bounds__(TPB) void vit_ens_post_kernel(uint8_t* __restrict__ work, const VitEnsTable tab,
                                                           const vit_frame_desc* __restrict__ idesc,
                                                           uint8_t* __restrict__ fire_ok) {
    __shared__ u32 s_prbs[PRBS_WORDS];
    load_prbs(s_prbs);
    __syncthreads();
    const u32 lane = threadIdx.x & (WAVE - 1u);
    for (u32 i = blockIdx.x * (TPB / WAVE) + (threadIdx.x / WAVE); i < tab.nframes; i += gridDim.x * (TPB / WAVE)) {
        const u32 k = (u32)__builtin_amdgcn_readfirstlane((int)vit_ens_find<&VitEnsEntry::frame0>(tab, i));
        const VitEnsEntry& e = tab.e[k];
        const u32 j = i - e.frame0, nb = e.framebits >> 3;
        uint8_t* p = work + e.work_off + (u64)j * nb;
        const bool fire = fire_ok && e.rsdims && j % 5u == 0;
        if (idesc && idesc[i].framebits == 0xFFFFFFFFu) {
            if (fire && lane == 0) fire_ok[e.rec0 + j / 5u] = fire_remainder(p + 2) == ((u32)p[0] << 8 | p[1]) ? 1 : 0;
            continue;
        }
        post_frame(p, nb, lane, s_prbs, fire, fire_ok + (e.rec0 + j / 5u));
    }
}

// vit_au_kernel over the table: one wavefront per record; its sub-channel gives rsdims and where the superframe lies
// (from_work: in the work layout, 120*rsdims apart).  The LDS images are sized for the table's largest rsdims.
__global__ __launch_bounds__(TPB) void vit_au_table_kernel(const uint8_t* __restrict__ sf, u32 from_work, const VitEnsTable tab,
                                                           const int32_t* __restrict__ ret, u32* __restrict__ au) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_au[];
    const u32 lane = threadIdx.x & (WAVE - 1u), wave = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    uint8_t* s = s_au + wave * au_lds_bytes(110u * tab.max_rsdims);
    const u32 fbit = d_fire_bits.v[lane], fbit2 = lane < 8u ? d_fire_bits.v[64u + lane] : 0u;
    // every wavefront of a workgroup makes the same number of rounds, as in vit_au_kernel
    for (u32 f0 = blockIdx.x * AU_WPB; f0 < tab.nrec; f0 += gridDim.x * AU_WPB) {
        const u32 f = f0 + wave;
        const bool live = f < tab.nrec;  // wave-uniform
        const bool read = live && !(ret && ret[live ? f : 0] < 0);
        const u32 k = (u32)__builtin_amdgcn_readfirstlane((int)vit_ens_find<&VitEnsEntry::rec0>(tab, live ? f : 0u));
        const VitEnsEntry& e = tab.e[k];
        const u32 L = 110u * e.rsdims, sfi = (live ? f : 0u) - e.rec0;
        const uint8_t* p = sf + (from_work ? e.work_off + (u64)sfi * (120u * e.rsdims) : e.rs_off + (u64)sfi * L);
        const u32 a = (u32)(reinterpret_cast<uintptr_t>(p) & 15u);
        if (read) au_load(p, L, a, s, lane);
        __syncthreads();
        if (read) {
            au_eval(s + a, L, lane, fbit, fbit2, au + 5u * (u64)f);
        } else if (live && lane < 5u) {
            au[5u * (u64)f + lane] = lane == 0u ? (u32)VIT_AU_RS_FAILED : 0u;
        }
        __syncthreads();  // the image is read before the next round overwrites it
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

void vit_au_table_host(const uint8_t* h_sf, uint32_t rsdims, vit_au_table* h_out) {
    const u32 L = 110u * rsdims;
    u32 b[11];
    for (u32 k = 0; k < 11u; k++) b[k] = h_sf[k];
    const AuHeader h = au_parse(b, L);
    u32 crc_ok = 0;
    for (u32 n = 0; h.valid && n < h.num_aus; n++) {
        u32 r = 0xFFFFu;
        for (u32 k = h.start[n]; k < h.start[n + 1] - 2u; k++) r = crc16_step(r, h_sf[k]);
        if ((r ^ 0xFFFFu) == ((u32)h_sf[h.start[n + 1] - 2u] << 8 | h_sf[h.start[n + 1] - 1u])) crc_ok |= 1u << n;
    }
    u32 w[5];
    au_record(w, h.valid ? VIT_AU_OK : VIT_AU_BAD_HEADER, h, b[2], crc_ok,
              fire_remainder(h_sf + 2) == (b[0] << 8 | b[1]) ? 1u : 0u);
    uint8_t* o = reinterpret_cast<uint8_t*>(h_out);
    for (u32 k = 0; k < 20u; k++) o[k] = (uint8_t)(w[k >> 2] >> (8u * (k & 3u)));
}

hipError_t vit_launch_aus(const uint8_t* d_sf, uint64_t sf_stride, uint32_t rsdims, int64_t nsf, const int32_t* d_ret,
                          vit_au_table* d_au, hipStream_t stream) {
    if (nsf <= 0) return hipSuccess;
    hipLaunchKernelGGL(vit_au_kernel, dim3(grid_for(nsf, AU_WPB)), dim3(TPB), AU_WPB * au_lds_bytes(110u * rsdims), stream,
                       d_sf, (u64)sf_stride, rsdims, (long long)nsf, d_ret, reinterpret_cast<u32*>(d_au));
    return hipGetLastError();
}

hipError_t vit_launch_fire(const uint8_t* d_bytes, uint64_t stride, int64_t n, uint8_t* d_ok, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(vit_fire_kernel, dim3(grid_for(n, TPB)), dim3(TPB), 0, stream, d_bytes, (u64)stride, (long long)n, d_ok);
    return hipGetLastError();
}

hipError_t vit_launch_ens_descs(const VitEnsTable& tab, const VitEnsSource& src, uint64_t span, vit_frame_desc* d_desc,
                                hipStream_t stream) {
    if (tab.nframes == 0) return hipSuccess;
    hipLaunchKernelGGL(vit_ens_desc_kernel, dim3((tab.nframes + TPB - 1) / TPB), dim3(TPB), 0, stream, tab, src, (u64)span, d_desc);
    return hipGetLastError();
}

hipError_t vit_launch_ens_post(uint8_t* d_work, const VitEnsTable& tab, const vit_frame_desc* d_idesc, uint8_t* d_fire_ok,
                               hipStream_t stream) {
    if (tab.nframes == 0) return hipSuccess;
    hipLaunchKernelGGL(vit_ens_post_kernel, dim3(grid_for(tab.nframes, TPB / WAVE)), dim3(TPB), 0, stream, d_work, tab, d_idesc,
                       d_fire_ok);
    return hipGetLastError();
}

hipError_t vit_launch_aus_table(const uint8_t* d_sf, bool from_work, const VitEnsTable& tab, const int32_t* d_ret,
                                vit_au_table* d_au, hipStream_t stream) {
    if (tab.nrec == 0) return hipSuccess;
    hipLaunchKernelGGL(vit_au_table_kernel, dim3(grid_for(tab.nrec, AU_WPB)), dim3(TPB),
                       AU_WPB * au_lds_bytes(110u * tab.max_rsdims), stream, d_sf, from_work ? 1u : 0u, tab, d_ret,
                       reinterpret_cast<u32*>(d_au));
    return hipGetLastError();
}
