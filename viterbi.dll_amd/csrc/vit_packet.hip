// vit_packet.hip -- packet-mode data sub-channels (EN 300 401 clause 5.3) behind the decoder, on the device: where the FEC
// frames of enhanced packet mode lie (vit_fec_sync_kernel), their RS(204,188) code over the 12-row interleaver
// (vit_fec_kernel, with its host twin vit_fec_frame_host), and the packets with their CRCs (vit_packets_kernel).  The
// definitions are written out in include/viterbi_amd.h ("Packet mode"); every constant of the format is in
// vit_packet_fmt.h.  The kernels here take one stream per launch; their bodies are the routines of vit_packet_dev.h and the
// text vit_fec_block.inc, which the kernels of vit_packet_table.hip (a table of streams per launch) use too.
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
#include "vit_packet_dev.h"

namespace {

unsigned grid_for(long long items, u32 per_block) {
    const long long b = (items + per_block - 1) / per_block;
    return (unsigned)(b < (1 << 20) ? b : (1 << 20));
}

// ---- the uniform kernels: one stream per launch; the routines are vit_packet_dev.h's -----------------------------------------
__global__ __launch_bounds__(TPB) void vit_packets_kernel(const uint8_t* __restrict__ bytes, u32 S, u32 G, long long nframes,
                                                          u32* __restrict__ rec) {
    __shared__ __attribute__((aligned(16))) uint8_t s_img[WPB][PKT_IMG];
    const u32 lane = threadIdx.x & (WAVE - 1u), wave = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    uint8_t* s = s_img[wave];
    const long long per_block = (long long)WPB * G;
    // every wavefront of a workgroup makes the same number of rounds: the barriers order the image's writes and reads
    for (long long f0 = (long long)blockIdx.x * per_block; f0 < nframes; f0 += (long long)gridDim.x * per_block) {
        const long long fw = f0 + (long long)wave * G;
        const u32 nf = fw < nframes ? (u32)(nframes - fw < (long long)G ? nframes - fw : (long long)G) : 0u;  // wave-uniform
        const uint8_t* p = bytes + (u64)(nf ? fw : 0) * (S * SLOT);
        const u32 a = (u32)(reinterpret_cast<uintptr_t>(p) & 15u);
        if (nf) load_image(p, nf * S * SLOT, s, lane, WAVE);
        __syncthreads();
        if (nf) pkt_wave_records(s, a, nf, S, fw, rec);
        __syncthreads();  // the image is read before the next round overwrites it
    }
}

__global__ __launch_bounds__(TPB) void vit_fec_sync_kernel(const uint8_t* __restrict__ bytes, long long nslots,
                                                           u32* __restrict__ score) {
    __shared__ u32 s_h[FEC_SLOTS];
    fec_sync_slots(bytes, nslots, PktLaunchGrid{}, score, s_h);
}

__global__ __launch_bounds__(TPB) void vit_fec_kernel(const uint8_t* in, uint8_t* out, long long nslots, u32 phase, long long nfec,
                                                      u32* __restrict__ rec) {
#define FEC_BLOCK blockIdx.x
#include "vit_fec_block.inc"
#undef FEC_BLOCK
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
