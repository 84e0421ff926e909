// vit_packet.hip -- packet-mode data sub-channels (EN 300 401 clause 5.3) behind the decoder, on the device: where the FEC
// frames of enhanced packet mode lie (vit_fec_sync_kernel), their RS(204,188) code over the 12-row interleaver
// (vit_fec_kernel, with its host twin vit_fec_frame_host), and the packets with their CRCs (vit_packets_kernel).  The
// definitions are written out in include/viterbi_amd.h ("Packet mode"); every constant of the format is in
// vit_packet_fmt.h.
//
// Packets: a wavefront takes 64 / S logical frames of S slots, a lane per slot.  The frames come into the wavefront's LDS
// image as aligned 16-byte windows (the edge windows byte by byte: nothing outside the frames is read), each lane takes its
// slot as seven dwords and one v_alignbyte per dword, and runs the CRC register from 0 over its 24 bytes.  A packet of n
// slots is checked on the register-0 remainder of ALL its bytes, R = sum_k r_(i+k) * x^(192(n-1-k)) mod g - Horner over the
// next lanes' remainders with one carry-less multiply by x^192 mod g per step - against the one value K_n that a good packet
// leaves there (the preset and the ones' complement are both linear: K_n = (0xFFFF + 0xFFFF * x^(8(24n-2))) * x^16 mod g).
// Which slots are starts: every lane walks the chain 0 -> next(0) -> ... up to its own slot, the links fetched from the
// lanes by ds_bpermute, all lanes in step; the loop ends with the frame's last packet.
//
// FEC: a lane per (frame, row), five frames per wavefront (60 lanes), twenty per workgroup.  The workgroup's frames are
// one contiguous block of the stream; it comes into LDS like the packets' image, so frame f's byte k is
// s_img[a + 2472 f + k] with a = the block's address mod 16.  A lane's bytes are 12 apart, a wavefront's frames 618 dwords
// = 10 banks apart: the 32 lanes of a ds_read_u8 lane group meet on no bank (frames at dwords 0..3, 10..13, 20..23 and
// 22..23, 30..33, 40..43 mod 32).  Syndromes come from the remainder mod g(x): the sixteen products x * g_j of the feedback
// byte are one 16-byte row, LO[x & 15] ^ HI[x >> 4] as in rs_dev.h (16 rows of 16 bytes fill the 64 banks once, so the two
// ds_read_b128 of a step never conflict).  A wavefront without a nonzero remainder is done there.  Otherwise the lanes
// with errors run Berlekamp-Massey on their own (to degree 8; compile-time indices only), and then the rows are taken one
// at a time by the whole wavefront: lane l evaluates the owner's locator at the positions l, l+64, l+128 and l+192 (< 204),
// a ballot counts the roots among the 204 real positions - a locator of degree L with L of them has no root in the padding
// and none twice - and the lanes that found a root evaluate Forney's formula there and patch the byte in LDS.
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

unsigned grid_for(long long items, u32 per_block) {
    const long long b = (items + per_block - 1) / per_block;
    return (unsigned)(b < (1 << 20) ? b : (1 << 20));
}

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

__global__ __launch_bounds__(TPB) void vit_packets_kernel(const uint8_t* __restrict__ bytes, u32 S, u32 G, long long nframes,
                                                          u32* __restrict__ rec) {
    __shared__ __attribute__((aligned(16))) uint8_t s_img[WPB][PKT_IMG];
    const u32 lane = threadIdx.x & (WAVE - 1u), wave = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    uint8_t* s = s_img[wave];
    const u32 g = lane / S, i = lane - g * S;  // frame of the wavefront, slot of the frame
    const long long per_block = (long long)WPB * G;
    // every wavefront of a workgroup makes the same number of rounds: the barriers order the image's writes and reads
    for (long long f0 = (long long)blockIdx.x * per_block; f0 < nframes; f0 += (long long)gridDim.x * per_block) {
        const long long fw = f0 + (long long)wave * G;
        const u32 nf = fw < nframes ? (u32)(nframes - fw < (long long)G ? nframes - fw : (long long)G) : 0u;  // wave-uniform
        const uint8_t* p = bytes + (u64)(nf ? fw : 0) * (S * SLOT);
        const u32 a = (u32)(reinterpret_cast<uintptr_t>(p) & 15u);
        if (nf) load_image(p, nf * S * SLOT, s, lane, WAVE);
        __syncthreads();
        if (nf) {
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
                    w0 = (addr == ADDR_PADDING ? VIT_PKT_PADDING : VIT_PKT_DATA) | (R == good ? 1u << 8 : 0u) | len << 16 |
                         flags << 24;
                    w1 = addr | (b2 & USEFUL_MASK) << 16;
                }
            }
            if (live) {
                u32* o = rec + 2u * ((u64)(fw + g) * S + i);
                o[0] = w0;
                o[1] = w1;
            }
        }
        __syncthreads();  // the image is read before the next round overwrites it
    }
}

// ---- FEC frames: where they lie ---------------------------------------------------------------------------------------------
// A slot that carries the header of FEC packet c counts for exactly one phase: p = i - 94 - c mod 103.
__global__ __launch_bounds__(TPB) void vit_fec_sync_kernel(const uint8_t* __restrict__ bytes, long long nslots,
                                                           u32* __restrict__ score) {
    __shared__ u32 s_h[FEC_SLOTS];
    for (u32 t = threadIdx.x; t < FEC_SLOTS; t += TPB) s_h[t] = 0;
    __syncthreads();
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < nslots; i += (long long)gridDim.x * TPB) {
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

// In place (in == out) a workgroup whose rows are all clean writes nothing.  Out of place every frame is written, and the
// first workgroup copies the slots in front of the first frame and behind the last.
__global__ __launch_bounds__(TPB) void vit_fec_kernel(const uint8_t* in, uint8_t* out, long long nslots, u32 phase, long long nfec,
                                                      u32* __restrict__ rec) {
    __shared__ __attribute__((aligned(16))) uint8_t s_img[FEC_IMG];
    __shared__ __attribute__((aligned(16))) u32 s_nib[2 * 16 * 4];
    __shared__ uint8_t s_ato[ATO_SIZE], s_iof[256];
    __shared__ __attribute__((aligned(4))) uint8_t s_rec[FEC_FPB * 16u];
    const u32 tid = threadIdx.x;
    const u32 lane = tid & (WAVE - 1u), wave = (u32)__builtin_amdgcn_readfirstlane((int)(tid / WAVE));
    if (tid < 2u * 16u * 4u) s_nib[tid] = c_fec_nib.w[tid];
    for (u32 k = tid; k < (u32)ATO_SIZE; k += TPB) s_ato[k] = g_gf.ato[k];
    s_iof[tid] = g_gf.iof[tid];
    const uint8_t* ato = s_ato;
    const uint8_t* iof = s_iof;
    const bool inplace = in == out;

    const long long F0 = (long long)blockIdx.x * FEC_FPB;
    const u32 nF = F0 < nfec ? (u32)(nfec - F0 < (long long)FEC_FPB ? nfec - F0 : (long long)FEC_FPB) : 0u;
    const u64 off = (u64)SLOT * ((u64)phase + (u64)FEC_SLOTS * (u64)F0);  // the workgroup's first byte
    const u32 n = nF * FEC_FRAME_BYTES;
    const u32 a = (u32)(reinterpret_cast<uintptr_t>(in + off) & 15u);
    if (nF) load_image(in + off, n, s_img, tid, TPB);
    if (!inplace && blockIdx.x == 0) {
        const u64 end = (u64)SLOT * (u64)nslots;
        const u64 head = nfec > 0 ? (u64)SLOT * phase : end;  // without a whole frame: everything
        const u64 tail = nfec > 0 ? (u64)SLOT * ((u64)phase + (u64)FEC_SLOTS * (u64)nfec) : end;
        for (u64 k = tid; k < head; k += TPB) out[k] = in[k];
        for (u64 k = tail + tid; k < end; k += TPB) out[k] = in[k];
    }
    __syncthreads();

    const u32 fl = wave * FEC_FPW + lane / ROWS, row = lane % ROWS;
    const bool active = lane < FEC_FPW * ROWS && fl < nF;
    const u32 fb = a + (active ? fl : 0u) * FEC_FRAME_BYTES;  // the frame in the image (idle lanes walk frame 0, to no effect)
    // remainder mod g(x): coefficient j = byte j of (r0, r1, r2, r3)
    u32 r0 = 0, r1 = 0, r2 = 0, r3 = 0;
    const u32 nibbase = (u32)(uintptr_t)(const LDS u32*)s_nib;  // LDS byte address
    {
        const uint8_t* q = s_img + fb + row;
        auto step = [&](u32 d) {
            const u32 f = r3 >> 24;
            const u32x4 lo = *reinterpret_cast<const LDS u32x4*>(nibbase + ((f << 4) & 0xF0u));
            const u32x4 hi = *reinterpret_cast<const LDS u32x4*>(nibbase + 256u + (f & 0xF0u));
            r3 = xor3(__builtin_amdgcn_alignbit(r3, r2, 24), lo.w, hi.w);
            r2 = xor3(__builtin_amdgcn_alignbit(r2, r1, 24), lo.z, hi.z);
            r1 = xor3(__builtin_amdgcn_alignbit(r1, r0, 24), lo.y, hi.y);
            r0 = xor3((r0 << 8) | d, lo.x, hi.x);
        };
#pragma unroll 4
        for (u32 c = 0; c < COLS; c++) step(q[ROWS * c]);
#pragma unroll
        for (u32 j = 0; j < NPAR; j++) step(s_img[fb + fec_byte(row, COLS + j)]);
    }
    const bool err = active && (r0 | r1 | r2 | r3) != 0;
    int nerr = 0;
    bool changed = false;
    if (__any(err)) {
        u32 L = 0;
        bool bad = true;
        u32 lz[TCORR + 1], oz[TCORR];  // locator and evaluator in index form, a zero coefficient as ATO_ZERO
#pragma unroll
        for (u32 k = 0; k <= TCORR; k++) lz[k] = ATO_ZERO;
#pragma unroll
        for (u32 k = 0; k < TCORR; k++) oz[k] = ATO_ZERO;
        if (err) {
            // syndromes S_i = rem(alpha^i) in index form (255: zero)
            u32 slog[NPAR];
            {
                u32 lg[NPAR], s0 = 0;
#pragma unroll
                for (u32 j = 0; j < NPAR; j++) {
                    const u32 c = ((j < 4u ? r0 : j < 8u ? r1 : j < 12u ? r2 : r3) >> (8u * (j & 3u))) & 0xFFu;
                    s0 ^= c;
                    lg[j] = c ? (u32)iof[c] : (u32)ATO_ZERO;
                }
                slog[0] = iof[s0];
#pragma unroll
                for (u32 i = 1; i < NPAR; i++) {
                    u32 v = 0;
#pragma unroll
                    for (u32 j = 0; j < NPAR; j++) v ^= ato[lg[j] + i * j];  // <= 512 + 225
                    slog[i] = iof[v];
                }
            }
            // Berlekamp-Massey; polynomials cut at degree 8: a term above it means L > 8, which fails anyway
            u32 lam[TCORR + 1], llog[TCORR + 1], blog[TCORR + 1];
#pragma unroll
            for (u32 k = 0; k <= TCORR; k++) {
                lam[k] = k ? 0u : 1u;
                llog[k] = blog[k] = k ? (u32)NN : 0u;
            }
#pragma unroll
            for (u32 r = 1; r <= NPAR; r++) {
                u32 dsc = 0;
#pragma unroll
                for (u32 k = 0; k <= TCORR; k++)
                    if (k < r && llog[k] != (u32)NN && slog[r - 1u - k] != (u32)NN) dsc ^= ato[llog[k] + slog[r - 1u - k]];
                const bool grow = dsc != 0 && 2u * L <= r - 1u;
                u32 nb[TCORR + 1];
#pragma unroll
                for (u32 k = 0; k <= TCORR; k++) {
                    const u32 shifted = k ? blog[k - 1u] : (u32)NN;
                    nb[k] = grow ? (llog[k] == (u32)NN ? (u32)NN : mod510(llog[k] + NN - iof[dsc])) : shifted;
                }
                if (dsc) {
                    const u32 dl = iof[dsc];
#pragma unroll
                    for (u32 k = 1; k <= TCORR; k++) {
                        if (blog[k - 1u] != (u32)NN) lam[k] ^= ato[dl + blog[k - 1u]];
                        llog[k] = iof[lam[k]];
                    }
                }
                if (grow) L = r - L;
#pragma unroll
                for (u32 k = 0; k <= TCORR; k++) blog[k] = nb[k];
            }
            u32 deg = 0;
#pragma unroll
            for (u32 k = 1; k <= TCORR; k++)
                if (llog[k] != (u32)NN) deg = k;
            bad = L > TCORR || deg != L;
#pragma unroll
            for (u32 k = 0; k <= TCORR; k++) lz[k] = llog[k] == (u32)NN ? (u32)ATO_ZERO : llog[k];
            // evaluator Omega = S * Lambda mod x^16; only its terms below degree L are used
#pragma unroll
            for (u32 k = 0; k < TCORR; k++) {
                u32 v = 0;
#pragma unroll
                for (u32 j = 0; j <= k; j++)
                    if (llog[j] != (u32)NN && slog[k - j] != (u32)NN) v ^= ato[llog[j] + slog[k - j]];
                oz[k] = v ? (u32)iof[v] : (u32)ATO_ZERO;
            }
            nerr = -1;
        }
        // one row at a time, the whole wavefront on it
        u64 work = __ballot(err && !bad);
        while (work) {
            const int owner = __builtin_ctzll(work);
            work &= work - 1;
            const u32 Lo = (u32)__builtin_amdgcn_readlane((int)L, owner);
            const u32 ofb = (u32)__builtin_amdgcn_readlane((int)fb, owner), orow = (u32)__builtin_amdgcn_readlane((int)row, owner);
            u32 lo_[TCORR + 1];
#pragma unroll
            for (u32 j = 1; j <= TCORR; j++) lo_[j] = (u32)__builtin_amdgcn_readlane((int)lz[j], owner);
            u32 z = 0, cnt = 0;
#pragma unroll
            for (u32 qd = 0; qd < 4u; qd++) {
                const u32 d = lane + WAVE * qd;  // the position whose coefficient has degree d: X = alpha^d
                u32 v = 1;
#pragma unroll
                for (u32 j = 1; j <= TCORR; j++)
                    if (j <= Lo) v ^= ato[lo_[j] + NN - mod255(j * d)];  // lambda_j * X^-j
                const bool hit = d < NCODE && v == 0;
                cnt += (u32)__popcll(__ballot(hit));
                z |= hit ? 1u << qd : 0u;
            }
            if (cnt == Lo) {  // Lo distinct roots, all at real positions
                u32 oo[TCORR];
#pragma unroll
                for (u32 k = 0; k < TCORR; k++) oo[k] = (u32)__builtin_amdgcn_readlane((int)oz[k], owner);
#pragma unroll
                for (u32 qd = 0; qd < 4u; qd++) {
                    if (!((z >> qd) & 1u)) continue;
                    const u32 d = lane + WAVE * qd;
                    u32 num = 0, den = 0;  // Omega(1/X) and Lambda'(1/X); the value is X * num / den
#pragma unroll
                    for (u32 k = 0; k < TCORR; k++)
                        if (k < Lo) num ^= ato[oo[k] + NN - mod255(k * d)];
#pragma unroll
                    for (u32 j = 1; j <= TCORR; j += 2)
                        if (j <= Lo) den ^= ato[lo_[j] + NN - mod255((j - 1u) * d)];
                    if (num && den) s_img[ofb + fec_byte(orow, NCODE - 1u - d)] ^= ato[mod255(d + iof[num] + NN - iof[den])];
                }
                if (lane == (u32)owner) nerr = (int)Lo;
                changed = true;
            }
        }
    }
    if (active) s_rec[fl * 16u + row] = (uint8_t)nerr;
    const bool write = __syncthreads_or(changed) || !inplace;  // (the barrier also orders the patches and s_rec)
    if (tid < nF * 4u) {
        const u32 f = tid >> 2, w = tid & 3u;
        const u32* nr = reinterpret_cast<const u32*>(s_rec + f * 16u);
        u32 v;
        if (w < 3u) {
            v = nr[w];
        } else {
            const uint8_t* h = s_img + a + f * FEC_FRAME_BYTES + FEC_DATA_BYTES;
            u32 ok = 0;
            for (u32 c = 0; c < FEC_PACKETS; c++)
                if (h[SLOT * c] == fec_hdr0(c) && h[SLOT * c + 1u] == FEC_HDR1) ok |= 1u << c;
            v = ok | (((nr[0] | nr[1] | nr[2]) & 0x80808080u) ? 1u << 16 : 0u);
        }
        rec[4u * (u64)(F0 + f) + w] = v;
    }
    if (write && nF) {
        uint8_t* dst = out + off;
        if (((u32)(reinterpret_cast<uintptr_t>(dst)) & 15u) == a) {
            const u32 nwin = (a + n + 15u) >> 4;
            for (u32 w = tid; w < nwin; w += TPB) {
                const int o = (int)(16u * w) - (int)a;
                if (o >= 0 && (u32)o + 16u <= n) {
                    *reinterpret_cast<uint4*>(dst + o) = *reinterpret_cast<const uint4*>(s_img + 16u * w);
                } else {
                    for (u32 j = 0; j < 16u; j++) {
                        const int k = o + (int)j;
                        if (k >= 0 && (u32)k < n) dst[k] = s_img[16u * w + j];
                    }
                }
            }
        } else {  // d_out at another phase in 16 bytes than d_stream
            for (u32 k = tid; k < n; k += TPB) dst[k] = s_img[a + k];
        }
    }
}

// ---- the host twin -------------------------------------------------------------------------------------------------------
inline u32 hmul(u32 x, u32 y) { return x && y ? k_gf.ato[k_gf.iof[x] + k_gf.iof[y]] : 0u; }
inline u32 hdiv(u32 x, u32 y) { return x ? k_gf.ato[k_gf.iof[x] + NN - k_gf.iof[y]] : 0u; }  // y != 0

// One row: cw[0..203], position k the coefficient of x^(203-k).  Returns the number of bytes changed, or -1.
int fec_row_host(uint8_t* cw) {
    u32 s[NPAR], any = 0;
    for (u32 i = 0; i < NPAR; i++) {  // Horner at alpha^i
        u32 v = 0;
        for (u32 k = 0; k < NCODE; k++) v = hmul(v, k_gf.ato[i]) ^ cw[k];
        s[i] = v;
        any |= v;
    }
    if (!any) return 0;
    u32 lam[NPAR + 2] = {1}, b[NPAR + 2] = {1}, L = 0;
    for (u32 r = 1; r <= NPAR; r++) {
        u32 dsc = 0;
        for (u32 k = 0; k < r && k <= NPAR; k++) dsc ^= hmul(lam[k], s[r - 1u - k]);
        u32 t[NPAR + 2];
        t[0] = lam[0];
        for (u32 k = 1; k <= NPAR + 1u; k++) t[k] = lam[k] ^ hmul(dsc, b[k - 1u]);
        if (dsc && 2u * L <= r - 1u) {
            L = r - L;
            for (u32 k = 0; k <= NPAR + 1u; k++) b[k] = hdiv(lam[k], dsc);
        } else {
            for (u32 k = NPAR + 1u; k > 0; k--) b[k] = b[k - 1u];
            b[0] = 0;
        }
        for (u32 k = 0; k <= NPAR + 1u; k++) lam[k] = t[k];
    }
    u32 deg = 0;
    for (u32 k = 0; k <= NPAR + 1u; k++)
        if (lam[k]) deg = k;
    if (L > TCORR || deg != L) return -1;
    u32 pos[TCORR], nroots = 0;
    for (u32 d = 0; d < NCODE; d++) {  // the real positions only: L roots there leave none for the padding
        u32 v = 0;
        for (u32 j = 0; j <= L; j++) v ^= hmul(lam[j], k_gf.ato[(NN - d) * j % NN]);
        if (v == 0) {
            if (nroots == L) return -1;
            pos[nroots++] = d;
        }
    }
    if (nroots != L) return -1;
    u32 om[TCORR] = {};
    for (u32 k = 0; k < L; k++)
        for (u32 j = 0; j <= k; j++) om[k] ^= hmul(lam[j], s[k - j]);
    for (u32 e = 0; e < L; e++) {
        const u32 d = pos[e], xi = k_gf.ato[(NN - d) % NN];  // 1/X
        u32 num = 0, den = 0, xp = 1;
        for (u32 k = 0; k < L; k++, xp = hmul(xp, xi)) num ^= hmul(om[k], xp);
        xp = 1;
        for (u32 j = 1; j <= L; j += 2, xp = hmul(xp, hmul(xi, xi))) den ^= hmul(lam[j], xp);
        if (!num || !den) return -1;  // cannot happen for L distinct roots of a minimal locator
        cw[NCODE - 1u - d] ^= (uint8_t)hmul(k_gf.ato[d], hdiv(num, den));
    }
    return (int)L;
}

}  // namespace

void vit_fec_frame_host(uint8_t* frame, vit_fec_rec* h_out) {
    uint8_t* o = reinterpret_cast<uint8_t*>(h_out);
    u32 failed = 0, hdr = 0;
    for (u32 r = 0; r < ROWS; r++) {
        uint8_t cw[NCODE];
        for (u32 k = 0; k < NCODE; k++) cw[k] = frame[fec_byte(r, k)];
        const int ne = fec_row_host(cw);
        if (ne > 0)
            for (u32 k = 0; k < NCODE; k++) frame[fec_byte(r, k)] = cw[k];
        if (ne < 0) failed = 1;
        o[r] = (uint8_t)(int8_t)ne;
    }
    for (u32 c = 0; c < FEC_PACKETS; c++)
        if (frame[FEC_DATA_BYTES + SLOT * c] == fec_hdr0(c) && frame[FEC_DATA_BYTES + SLOT * c + 1u] == FEC_HDR1) hdr |= 1u << c;
    o[12] = (uint8_t)hdr;
    o[13] = (uint8_t)(hdr >> 8);
    o[14] = (uint8_t)failed;
    o[15] = 0;
}

hipError_t vit_launch_fec_sync(const uint8_t* d_stream, int64_t nslots, uint32_t* d_score, hipStream_t stream) {
    if (nslots <= 0) return hipSuccess;
    const hipError_t e = hipMemsetAsync(d_score, 0, FEC_SLOTS * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(vit_fec_sync_kernel, dim3(grid_for(nslots, 4u * TPB)), dim3(TPB), 0, stream, d_stream, (long long)nslots,
                       d_score);
    return hipGetLastError();
}

hipError_t vit_launch_fec(const uint8_t* d_stream, uint8_t* d_out, int64_t nslots, uint32_t phase, int64_t nfec, vit_fec_rec* d_fec,
                          hipStream_t stream) {
    const bool inplace = d_stream == d_out;
    if (nslots <= 0 || (nfec <= 0 && inplace)) return hipSuccess;
    const long long blocks = nfec > 0 ? (nfec + FEC_FPB - 1) / FEC_FPB : 1;
    hipLaunchKernelGGL(vit_fec_kernel, dim3((unsigned)blocks), dim3(TPB), 0, stream, d_stream, d_out, (long long)nslots, phase,
                       (long long)nfec, reinterpret_cast<u32*>(d_fec));
    return hipGetLastError();
}

hipError_t vit_launch_packets(const uint8_t* d_bytes, uint32_t framebytes, int64_t nframes, vit_packet_rec* d_rec,
                              hipStream_t stream) {
    if (nframes <= 0) return hipSuccess;
    const u32 S = framebytes / SLOT, G = WAVE / S;
    hipLaunchKernelGGL(vit_packets_kernel, dim3(grid_for(nframes, WPB * G)), dim3(TPB), 0, stream, d_bytes, S, G, (long long)nframes,
                       reinterpret_cast<u32*>(d_rec));
    return hipGetLastError();
}
