// vit_packet_dev.h -- the device routines of packet mode, one text each: the slot walk and the CRC of a wavefront's logical
// frames and the header score that finds the FEC frames, and what the FEC kernels share beside their body (the generator's
// tables, the geometry); the body itself - RS(204,188) over a workgroup's FEC frames: remainder, Berlekamp-Massey, root
// search and Forney, records and the image's way back - is the text vit_fec_block.inc, included inside both FEC kernels.
// vit_packet.hip uses them in the uniform kernels (one stream per launch), vit_packet_table.hip in the table kernels (up
// to 64 streams per launch); what differs between the two is only where a wavefront's or a workgroup's share of the work
// comes from.  How the routines work is written out at the head of vit_packet.hip; every constant of the format is in
// vit_packet_fmt.h.
#pragma once
#include "rs_dev.h"
#include "vit_crc_dev.h"
#include "vit_image_dev.h"
#include "vit_packet_fmt.h"

namespace {

using namespace pktfmt;
typedef uint32_t u32;
typedef uint64_t u64;
constexpr u32 TPB = 256;
constexpr u32 WAVE = 64;
constexpr u32 WPB = TPB / WAVE;

// ---- packets ------------------------------------------------------------------------------------------------------------
// (crc_xpow and crc_mul: vit_crc_dev.h)
constexpr u32 PKT_X192 = crc_xpow(SLOT, 1u);
// the register-0 remainder of a whole packet of n slots whose last two bytes are right
constexpr u32 pkt_good(u32 n) { return crc_xpow(2u, 0xFFFFu ^ crc_xpow(SLOT * n - 2u, 0xFFFFu)); }
constexpr u32 crc16_of(const char* s, u32 n) {
    u32 r = 0xFFFFu;
    for (u32 k = 0; k < n; k++) r = crc16_step(r, (uint8_t)s[k]);
    return r ^ 0xFFFFu;
}
static_assert(crc16_of("123456789", 9) == 0xD64Eu, "CRC-16 0x1021, preset 0xFFFF, complemented");

constexpr u32 PKT_IMG = WAVE * SLOT + 32u;  // 64 slots at any phase, and the seventh dword of the last one

// The records of a wavefront's nf > 0 logical frames of S slots, whose bytes lie in the wavefront's image s at phase a
// (load_image, behind a barrier): lane = g * S + i is slot i of the wavefront's frame g, the frame fw + g of the stream
// whose records start at rec.
__device__ __forceinline__ void pkt_wave_records(const uint8_t* s, u32 a, u32 nf, u32 S, long long fw, u32* rec) {
    const u32 lane = threadIdx.x & (WAVE - 1u);
    const u32 g = lane / S, i = lane - g * S;  // frame of the wavefront, slot of the frame
    const bool live = g < nf;
    const u32 base = live ? a + SLOT * lane : 0u, sh = base & 3u;
    const u32* q = reinterpret_cast<const u32*>(s + (base & ~3u));
    u32 d[7], w[6];
#pragma unroll
    for (u32 k = 0; k < 7u; k++) d[k] = q[k];
#pragma unroll
    for (u32 k = 0; k < 6u; k++) w[k] = __builtin_amdgcn_alignbyte(d[k + 1u], d[k], sh);
    u32 r = 0;
#pragma unroll
    for (u32 k = 0; k < SLOT; k++) r = crc16_step(r, (w[k >> 2] >> (8u * (k & 3u))) & 0xFFu);
    const u32 b0 = w[0] & 0xFFu, b1 = (w[0] >> 8) & 0xFFu, b2 = (w[0] >> 16) & 0xFFu;
    const u32 addr = (b0 & ADDR_HI_MASK) << 8 | b1;
    const u32 len = addr == ADDR_FEC ? 1u : (b0 >> LEN_SHIFT) + 1u;
    const u32 nx = i + len;
    // the chain from slot 0 up to this lane's slot
    u32 kind = VIT_PKT_CONT, cur = 0;
    bool walking = live;
    while (__any(walking)) {
        const u32 src = live ? g * S + cur : lane;
        const u32 nxc = (u32)__builtin_amdgcn_ds_bpermute((int)(4u * src), (int)nx);
        if (walking) {
            if (nxc > S) {
                kind = VIT_PKT_OVERRUN;
                walking = false;
            } else if (cur == i) {
                kind = VIT_PKT_DATA;
                walking = false;
            } else if (nxc > i) {
                walking = false;
            } else {
                cur = nxc;
            }
        }
    }
    // the whole packet's remainder, for 1 ... 4 slots
    const u32 r1 = (u32)__builtin_amdgcn_ds_bpermute((int)(4u * ((lane + 1u) & 63u)), (int)r);
    const u32 r2 = (u32)__builtin_amdgcn_ds_bpermute((int)(4u * ((lane + 2u) & 63u)), (int)r);
    const u32 r3 = (u32)__builtin_amdgcn_ds_bpermute((int)(4u * ((lane + 3u) & 63u)), (int)r);
    const u32 R2 = crc_mul<PKT_X192>(r) ^ r1, R3 = crc_mul<PKT_X192>(R2) ^ r2, R4 = crc_mul<PKT_X192>(R3) ^ r3;
    const u32 R = len == 1u ? r : len == 2u ? R2 : len == 3u ? R3 : R4;
    const u32 good = len == 1u ? pkt_good(1) : len == 2u ? pkt_good(2) : len == 3u ? pkt_good(3) : pkt_good(4);
    u32 w0 = kind, w1 = 0;
    if (kind == VIT_PKT_DATA) {
        if (addr == ADDR_FEC) {
            w0 = VIT_PKT_FEC | 1u << 16 | ((b0 >> FEC_CNT_SHIFT) & 15u) << 24;
            w1 = addr;
        } else {
            const u32 flags = ((b0 >> CONT_SHIFT) & 3u) | ((b0 >> FL_SHIFT) & 3u) << 2 | ((b2 & CMD_MASK) ? 16u : 0u);
            w0 = (addr == ADDR_PADDING ? VIT_PKT_PADDING : VIT_PKT_DATA) | (R == good ? 1u << 8 : 0u) | len << 16 | flags << 24;
            w1 = addr | (b2 & USEFUL_MASK) << 16;
        }
    }
    if (live) {
        u32* o = rec + 2u * ((u64)(fw + g) * S + i);
        o[0] = w0;
        o[1] = w1;
    }
}

// ---- FEC frames: where they lie ---------------------------------------------------------------------------------------------
// A slot that carries the header of FEC packet c counts for exactly one phase: p = i - 94 - c mod 103.
// Which of the workgroups that share a stream this one is, block() of nblocks(): the launch's own grid for the uniform
// kernels, a range of the launch's workgroups taken from the table for the table kernels.  The routines ask where they
// use the answer.
struct PktLaunchGrid {
    __device__ __forceinline__ u32 block() const { return blockIdx.x; }
    __device__ __forceinline__ u32 nblocks() const { return gridDim.x; }
};
struct PktTableGrid {
    u32 b, n;
    __device__ __forceinline__ u32 block() const { return b; }
    __device__ __forceinline__ u32 nblocks() const { return n; }
};

// A workgroup's share of a stream's scores: a thread's slots are TPB * nblocks apart; they are counted in s_h, FEC_SLOTS
// words of LDS, then added to the stream's score words.
template <class Grid>
__device__ __forceinline__ void fec_sync_slots(const uint8_t* bytes, long long nslots, const Grid& grid, u32* score, u32* s_h) {
    for (u32 t = threadIdx.x; t < FEC_SLOTS; t += TPB) s_h[t] = 0;
    __syncthreads();
    for (long long i = (long long)grid.block() * TPB + threadIdx.x; i < nslots; i += (long long)grid.nblocks() * TPB) {
        const uint8_t* p = bytes + (u64)i * SLOT;
        const u32 b0 = p[0], b1 = p[1], c = b0 >> FEC_CNT_SHIFT;
        if (b1 == FEC_HDR1 && c < FEC_PACKETS && b0 == fec_hdr0(c))
            atomicAdd(&s_h[((u32)(i % FEC_SLOTS) + 2u * FEC_SLOTS - FEC_DATA_SLOTS - c) % FEC_SLOTS], 1u);
    }
    __syncthreads();
    for (u32 t = threadIdx.x; t < FEC_SLOTS; t += TPB)
        if (s_h[t]) atomicAdd(&score[t], s_h[t]);
}

// ---- FEC frames: RS(204,188) ---------------------------------------------------------------------------------------------
constexpr GfTables k_gf = make_tables();
struct FecGen {
    uint8_t g[NPAR + 1];  // g_0 ... g_16 = 1
};
constexpr FecGen make_fec_gen() {
    FecGen G{};
    G.g[0] = 1;
    for (u32 i = 0; i < NPAR; i++) {  // multiply by (x + alpha^i)
        uint8_t ng[NPAR + 1] = {};
        for (u32 j = 0; j <= i; j++) {
            ng[j + 1] ^= G.g[j];
            if (G.g[j]) ng[j] ^= k_gf.ato[k_gf.iof[G.g[j]] + i];
        }
        for (u32 j = 0; j <= i + 1u; j++) G.g[j] = ng[j];
    }
    return G;
}
constexpr FecGen k_fec_gen = make_fec_gen();
static_assert(k_fec_gen.g[NPAR] == 1, "g(x) is monic of degree 16");
// Row(x) = (x*g_0, ..., x*g_15) = LO[x & 15] ^ HI[x >> 4], 16 bytes a row (rs_dev.h, NibTable)
struct FecNib {
    u32 w[2 * 16 * 4];
};
constexpr FecNib make_fec_nib() {
    FecNib N{};
    for (u32 half = 0; half < 2u; half++)
        for (u32 n = 1; n < 16u; n++) {
            const u32 x = half ? n << 4 : n;
            for (u32 j = 0; j < NPAR; j++) {
                const u32 gj = k_fec_gen.g[j];
                const u32 prod = gj ? k_gf.ato[k_gf.iof[x] + k_gf.iof[gj]] : 0u;
                N.w[(half * 16u + n) * 4u + j / 4u] |= prod << (8u * (j % 4u));
            }
        }
    return N;
}
__constant__ FecNib c_fec_nib = make_fec_nib();

constexpr u32 FEC_FPW = WAVE / ROWS;  // frames per wavefront
constexpr u32 FEC_FPB = FEC_FPW * WPB;
constexpr u32 FEC_IMG = (FEC_FPB * FEC_FRAME_BYTES + 15u + 15u) & ~15u;  // the workgroup's frames at any phase, whole windows
static_assert(FEC_FPW * ROWS <= WAVE && NCODE <= 4u * WAVE, "a lane per row; four positions per lane in the root search");

}  // namespace
