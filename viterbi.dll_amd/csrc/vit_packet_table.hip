// vit_packet_table.hip -- packet mode over a table of streams in a fixed number of launches (include/viterbi_amd.h,
// vit_packet_table_dev): the kernels of vit_packet.hip with each pass's stream, place and count taken from the table
// (vit_internal.h, VitPktTable), and between sync and FEC the pick that replaces the host's argmax.  The passes
// themselves are one text (vit_packet_dev.h, vit_fec_block.inc); this unit holds the table lookups and the pick.  A pass never mixes streams.
#include "vit_packet_dev.h"

namespace {

// ---- sync: a workgroup per FEC_SEARCH stream and chunk of slots, on the stream's own 103 words ----------------------------
__global__ __launch_bounds__(TPB) void vit_pkt_table_sync_kernel(const uint8_t* __restrict__ bytes, u32* __restrict__ score,
                                                                 const VitPktTable tab) {
    __shared__ u32 s_h[FEC_SLOTS];
    const u32 k = vit_table_find<VitPktEntry, &VitPktEntry::sync0>(tab.e, tab.nstreams, blockIdx.x);
    const VitPktEntry& e = tab.e[k];
    const u32 nchunk = (k + 1u < tab.nstreams ? tab.e[k + 1u].sync0 : tab.nsync) - e.sync0;  // the stream's workgroups
    // the uniform launch with a grid of nchunk, on this stream
    fec_sync_slots(bytes + e.offset, (long long)e.nslots, PktTableGrid{blockIdx.x - e.sync0, nchunk}, score + FEC_SLOTS * k, s_h);
}

// ---- pick: a wavefront per stream -----------------------------------------------------------------------------------------
struct VitPktMinScore {
    u32 v[VIT_PKT_MAX_STREAMS];
};
__device__ __forceinline__ u32 wave_max(u32 v) {
#pragma unroll
    for (u32 m = 1; m < WAVE; m <<= 1) {
        const u32 o = (u32)__shfl_xor((int)v, (int)m, (int)WAVE);
        v = o > v ? o : v;
    }
    return v;
}
// Lane l holds the scores of phases l and l + 64 (< 103).  The largest score, the smallest phase that has it and the
// largest score at any other phase come from three reductions over the wavefront; lane 0 writes the record.
__global__ __launch_bounds__(TPB) void vit_pkt_table_pick_kernel(const u32* __restrict__ score, u32* __restrict__ srec,
                                                                 const VitPktTable tab, const VitPktMinScore min_score) {
    const u32 lane = threadIdx.x & (WAVE - 1u);
    const u32 k = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * WPB + threadIdx.x / WAVE));
    if (k >= tab.nstreams) return;  // wave-uniform; no barrier follows
    const VitPktEntry& e = tab.e[k];
    u32 phase = VIT_PKT_NO_PHASE, best = 0, second = 0;
    if (e.fec == VIT_PKT_FEC_PHASE) {
        phase = e.phase;
    } else if (e.fec == VIT_PKT_FEC_SEARCH) {
        const u32* sc = score + FEC_SLOTS * k;
        const u32 lo = sc[lane], hi = lane + WAVE < FEC_SLOTS ? sc[lane + WAVE] : 0u;
        best = wave_max(lo > hi ? lo : hi);
        const u64 at_lo = __ballot(lo == best), at_hi = __ballot(lane + WAVE < FEC_SLOTS && hi == best);
        const u32 p = at_lo ? (u32)__builtin_ctzll(at_lo) : WAVE + (u32)__builtin_ctzll(at_hi);  // one of them is not empty
        const u32 lo_x = lane == p ? 0u : lo, hi_x = lane + WAVE == p ? 0u : hi;
        second = wave_max(lo_x > hi_x ? lo_x : hi_x);
        const u32 need = min_score.v[k] > 1u ? min_score.v[k] : 1u;
        if (best >= need) phase = p;
    }
    const u32 nfec = phase != VIT_PKT_NO_PHASE && e.nslots > phase ? (e.nslots - phase) / FEC_SLOTS : 0u;
    if (lane == 0) {
        u32* o = srec + 4u * k;
        o[0] = phase;
        o[1] = best;
        o[2] = second;
        o[3] = nfec;
    }
}

// ---- FEC: a workgroup per 20 frames of one stream, phase and count from the pick's record ----------------------------------
__global__ __launch_bounds__(TPB) void vit_pkt_table_fec_kernel(uint8_t* bytes, const u32* __restrict__ srec, u32* __restrict__ rec_all,
                                                                const VitPktTable tab) {
    const u32 k = vit_table_find<VitPktEntry, &VitPktEntry::fecwg0>(tab.e, tab.nstreams, blockIdx.x);
    const VitPktEntry& e = tab.e[k];
    const u32 block = blockIdx.x - e.fecwg0;  // among the stream's
    // written by the pick kernel, earlier on the same stream; the grid is the host's upper bound, so a workgroup may find
    // nothing to do: it leaves here, all of it (blockIdx and the record are workgroup-uniform), in front of every barrier
    const u32 phase = (u32)__builtin_amdgcn_readfirstlane((int)srec[4u * k]);
    const u32 nfec_k = (u32)__builtin_amdgcn_readfirstlane((int)srec[4u * k + 3u]);
    if ((u64)block * FEC_FPB >= nfec_k) return;
    const uint8_t* in = bytes + e.offset;
    uint8_t* out = bytes + e.offset;
    const long long nslots = e.nslots, nfec = nfec_k;
    u32* rec = rec_all + 4u * (u64)e.fec0;
#define FEC_BLOCK block
#include "vit_fec_block.inc"
#undef FEC_BLOCK
}

// ---- packets: a wavefront's round takes 64 / S frames of one stream ------------------------------------------------------
__global__ __launch_bounds__(TPB) void vit_pkt_table_packets_kernel(const uint8_t* __restrict__ bytes, u32* __restrict__ rec,
                                                                    const VitPktTable tab) {
    __shared__ __attribute__((aligned(16))) uint8_t s_img[WPB][PKT_IMG];
    const u32 lane = threadIdx.x & (WAVE - 1u), wave = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    uint8_t* s = s_img[wave];
    // The workgroup's round q0 takes the passes q0 ... q0 + 3, one per wavefront, whichever streams they belong to.  The
    // loop's condition and step depend on blockIdx, gridDim and the table alone, so every wavefront of a workgroup makes
    // the same number of rounds and meets both barriers of each: what a wavefront's own pass decides (its stream, S, nf,
    // or that there is none behind the table's last pass) only switches its work between the barriers on and off.
    for (u32 q0 = blockIdx.x * WPB; q0 < tab.npkt; q0 += gridDim.x * WPB) {  // npkt <= 2^31, the grid at most 2^20: no wrap
        const u32 q = q0 + wave;
        u32 S = 1, nf = 0, a = 0;
        long long fw = 0;
        u32* rec_k = rec;
        if (q < tab.npkt) {  // wave-uniform
            const u32 k = vit_table_find<VitPktEntry, &VitPktEntry::pkt0>(tab.e, tab.nstreams, q);
            const VitPktEntry& e = tab.e[k];
            S = e.S;
            const u32 G = WAVE / S;
            fw = (long long)(q - e.pkt0) * G;
            nf = e.nframes - (u32)fw < G ? e.nframes - (u32)fw : G;  // >= 1: the stream has ceil(nframes / G) passes
            const uint8_t* p = bytes + e.offset + (u64)fw * (S * SLOT);
            a = (u32)(reinterpret_cast<uintptr_t>(p) & 15u);
            rec_k = rec + 2u * (u64)e.rec0;
            load_image(p, nf * S * SLOT, s, lane, WAVE);
        }
        __syncthreads();
        if (nf) pkt_wave_records(s, a, nf, S, fw, rec_k);
        __syncthreads();  // the image is read before the next round overwrites it
    }
}

}  // namespace

hipError_t vit_launch_pkt_table_sync(const uint8_t* d_bytes, const VitPktTable& tab, uint32_t* d_score, hipStream_t stream) {
    const hipError_t e = hipMemsetAsync(d_score, 0, (size_t)tab.nstreams * FEC_SLOTS * sizeof(uint32_t), stream);
    if (e != hipSuccess || tab.nsync == 0) return e;
    hipLaunchKernelGGL(vit_pkt_table_sync_kernel, dim3(tab.nsync), dim3(TPB), 0, stream, d_bytes, d_score, tab);
    return hipGetLastError();
}

hipError_t vit_launch_pkt_table_pick(const VitPktTable& tab, const uint32_t* d_score, const uint32_t* h_min_score,
                                     vit_pkt_stream_rec* d_srec, hipStream_t stream) {
    VitPktMinScore ms = {};
    for (u32 k = 0; k < tab.nstreams; k++) ms.v[k] = h_min_score[k];
    hipLaunchKernelGGL(vit_pkt_table_pick_kernel, dim3((tab.nstreams + WPB - 1u) / WPB), dim3(TPB), 0, stream, d_score,
                       reinterpret_cast<u32*>(d_srec), tab, ms);
    return hipGetLastError();
}

hipError_t vit_launch_pkt_table_fec(uint8_t* d_bytes, const VitPktTable& tab, const vit_pkt_stream_rec* d_srec, vit_fec_rec* d_fec,
                                    hipStream_t stream) {
    if (tab.nfecwg == 0) return hipSuccess;
    hipLaunchKernelGGL(vit_pkt_table_fec_kernel, dim3(tab.nfecwg), dim3(TPB), 0, stream, d_bytes, reinterpret_cast<const u32*>(d_srec),
                       reinterpret_cast<u32*>(d_fec), tab);
    return hipGetLastError();
}

hipError_t vit_launch_pkt_table_packets(const uint8_t* d_bytes, const VitPktTable& tab, vit_packet_rec* d_rec, hipStream_t stream) {
    const u32 blocks = (tab.npkt + WPB - 1u) / WPB;
    hipLaunchKernelGGL(vit_pkt_table_packets_kernel, dim3(blocks < (1u << 20) ? blocks : (1u << 20)), dim3(TPB), 0, stream, d_bytes,
                       reinterpret_cast<u32*>(d_rec), tab);
    return hipGetLastError();
}
