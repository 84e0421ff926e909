// vit_dgroup.hip -- MSC data groups from the packets of a packet-mode sub-channel (include/viterbi_amd.h, "Packet mode":
// vit_data_groups_dev and its host twin).  The format's constants are in vit_packet_fmt.h, the CRC arithmetic in
// vit_crc_dev.h.
//
// The run rule is local: whether a packet continues its predecessor of the same address depends on the two of them only.
// So a stretch of one address's packets is summed up by what its first and last packet are and by its last run (head
// slot, whether the head has the first flag, packets, bytes, and whether that run began at the stretch's first packet), and
// two such summaries combine associatively (RunState / run_join).  No sort is needed:
//   presence   which of the 1024 addresses have usable packets (a bit set), usable and unusable packets counted
//   link       a workgroup per present address and chunk of 16384 slots, a thread per slot of a tile of 1024: slots of other
//              addresses are the identity, a scan of run_join over the tile (shuffles inside a wavefront, the wavefronts'
//              totals through LDS) and the state carried from tile to tile give every packet the run it closes.  A first
//              launch leaves each chunk's total (only with more than one chunk), the second starts from the join of the
//              chunks before and writes, for every usable packet with the last flag, a marker (head slot + 1 or 0, packets,
//              bytes) at its slot, and the address's open run, if any
//   number     the prefix sum over the slots (4096 a workgroup: sums, their scan with the summary's totals, then again with
//              the bases) numbers the groups and places them; the groups that are written get the first five words of their
//              record
//   gather     a wavefront per written group: it looks through the group's slots 64 at a time, lists the group's packets
//              (ballot and prefix) and takes 64 listed packets a step, a lane per packet: the lanes take
//              their bytes through a row of LDS each (aligned dword loads, all in flight at once), copy them out (dwords
//              where d_data's address allows) and run the CRC over them from register 0; the
//              remainders combine in slot order as (r, x^(8 len)) pairs under carry-less multiplication mod g; the first
//              nine bytes and the last two go through LDS to lane 0, which parses the header and writes the record
// Nothing in the output depends on an order of arrival: the counts are integer sums, open_from and the first group that is
// not written are minima.
#include "vit_dgroup_dev.h"
#include "vit_internal.h"

#include <cstring>
#include <vector>

namespace {

// ---- the per-stream kernels: one stream per launch; the routines are vit_dgroup_dev.h's -------------------------------------
__global__ __launch_bounds__(PRES_TPB) void vit_dg_presence_kernel(const u32* __restrict__ rec, long long nslots, u32* __restrict__ hdr) {
    __shared__ u32 s_bits[NADDR / 32u], s_cnt[2];
    dg_presence(rec, nslots, hdr, blockIdx.x, gridDim.x, s_bits, s_cnt);
}

// (this kernel keeps its own text of what the table kernels call as dg_link: as a call of the routine it compiled to other
// code - 31 for 32 VGPRs, 82 for 86 SGPRs, the blocks in another order - profiles/r26_dgroup_table_isa_same.txt)
// EMIT false: totals[address][chunk] = the chunk's state.  EMIT true: markers and the address's open run.
template <bool EMIT>
__global__ __launch_bounds__(TILE) void vit_dg_link_kernel(const u32* __restrict__ rec, long long nslots, const u32* __restrict__ hdr,
                                                           uint4* totals, u32 nchunks, uint4* __restrict__ marker,
                                                           uint2* __restrict__ open) {
    __shared__ uint4 s_tot[2][TILE / WAVE];
    const u32 A = blockIdx.y, chunk = blockIdx.x;
    if (!((hdr[H_BITS + (A >> 5)] >> (A & 31u)) & 1u)) return;  // the same for the whole workgroup
    const u32 tid = threadIdx.x, lane = tid & (WAVE - 1u), wave = tid / WAVE;
    RunState carry = {0, 0, 0, 0};
    if (EMIT)
        for (u32 c = 0; c < chunk; c++) carry = run_join(carry, run_from(totals[(size_t)A * nchunks + c]));
    for (u32 t = 0; t < CHUNK_TILES; t++) {
        const long long tile0 = (long long)chunk * CHUNK + (long long)t * TILE;
        if (tile0 >= nslots) break;
        const long long i = tile0 + tid;
        u32 w0 = 0, w1 = 0;
        if (i < nslots) {
            w0 = rec[2 * i];
            w1 = rec[2 * i + 1];
        }
        const bool mine = i < nslots && rec_usable(w0, w1, (u64)i, (u64)nslots) && rec_addr(w1) == A;
        RunState x = {0, 0, 0, 0};
        if (mine) x = run_leaf(rec_flags(w0), (u32)i, rec_useful(w1));
#pragma unroll
        for (u32 d = 1; d < WAVE; d <<= 1) {
            const RunState o = run_shfl_up(x, d);
            if (lane >= d) x = run_join(o, x);
        }
        if (lane == WAVE - 1u) s_tot[t & 1u][wave] = run_words(x);
        __syncthreads();  // one barrier a tile: the totals alternate between two buffers
        RunState pre = carry, before = carry;
        for (u32 k = 0; k < TILE / WAVE; k++) {
            if (k == wave) before = pre;
            pre = run_join(pre, run_from(s_tot[t & 1u][k]));
        }
        carry = pre;
        if (EMIT && mine && (rec_flags(w0) & VIT_PKT_LAST)) {
            const RunState r = run_join(before, x);
            marker[i] = make_uint4((r.w0 & RS_HF) ? r.head + 1u : 0u, r.npk, r.bytes, 0u);
        }
    }
    if (tid == 0) {
        if (!EMIT) {
            totals[(size_t)A * nchunks + chunk] = run_words(carry);
        } else if (chunk == nchunks - 1u) {
            const bool is_open = (carry.w0 & RS_VALID) && (carry.w0 & RS_HF) && !(carry.w0 & RS_LL);
            open[A] = is_open ? make_uint2(carry.head, carry.npk) : make_uint2(0xFFFFFFFFu, 0u);
        }
    }
}

__global__ __launch_bounds__(NUM_TPB) void vit_dg_sums_kernel(const u32* __restrict__ rec, const uint4* __restrict__ marker,
                                                              long long nslots, uint4* __restrict__ bsum) {
    __shared__ u32 s_w[NUM_TPB / WAVE][2], s_out[2], s_used;
    dg_sums(rec, marker, nslots, bsum, blockIdx.x, s_w, s_out, s_used);
}

__global__ __launch_bounds__(NUM_TPB) void vit_dg_bases_kernel(const uint4* __restrict__ bsum, u32 nblocks, uint4* __restrict__ bbase,
                                                               const uint2* __restrict__ open, long long nslots, u32* hdr) {
    __shared__ u32 s_w[NUM_TPB / WAVE][2], s_out[2], s_red[3];
    dg_bases(bsum, nblocks, bbase, open, nslots, hdr, s_w, s_out, s_red);
}

__global__ __launch_bounds__(NUM_TPB) void vit_dg_place_kernel(const u32* __restrict__ rec, const uint4* __restrict__ marker,
                                                               long long nslots, const uint4* __restrict__ bbase, u32* __restrict__ dg,
                                                               u32 max_groups, u32 has_data, u32 capacity, u32* hdr) {
    __shared__ u32 s_w[NUM_TPB / WAVE][2], s_out[2];
    dg_place(rec, marker, nslots, bbase, dg, max_groups, has_data, capacity, hdr, blockIdx.x, s_w, s_out);
}

__global__ __launch_bounds__(WAVE) void vit_dg_gather_kernel(const uint8_t* __restrict__ bytes, const u32* __restrict__ rec,
                                                             long long nslots, const u32* __restrict__ hdr, u32* dg,
                                                             u32* __restrict__ sum, uint8_t* __restrict__ data) {
    __shared__ uint8_t s_hdr[16], s_tail[DG_CRC_BYTES];
    __shared__ u32 s_list[2u * GATHER_STEP];
    __shared__ u32 s_row[WAVE][GATHER_ROW_DWORDS + 1u];
    const u32 ngroups = hdr[H_NGROUPS];
    const u32 nwritten = hdr[H_FIRST_UNWRITTEN] < ngroups ? hdr[H_FIRST_UNWRITTEN] : ngroups;
    if (blockIdx.x == 0 && threadIdx.x == 0) dg_summary(hdr, ngroups, nwritten, sum);
    // the same trips for the whole workgroup (one wavefront)
    for (u32 k = blockIdx.x; k < nwritten; k += gridDim.x) dg_gather_group(bytes, rec, nslots, dg, data, k, s_hdr, s_tail, s_list, s_row);
}

unsigned grid_for(long long items, u32 per_block, u32 cap) {
    const long long b = (items + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : b < (long long)cap ? b : (long long)cap);
}

}  // namespace

size_t vit_data_groups_scratch(int64_t nslots) { return layout(nslots).end; }

hipError_t vit_launch_data_groups(const uint8_t* d_bytes, const vit_packet_rec* d_rec, int64_t nslots, vit_dgroup_rec* d_dg,
                                  uint32_t max_groups, vit_dgroup_summary* d_sum, uint8_t* d_data, uint32_t data_capacity,
                                  void* d_scratch, hipStream_t stream) {
    if (nslots <= 0) return hipSuccess;
    const Layout L = layout(nslots);
    uint8_t* s = static_cast<uint8_t*>(d_scratch);
    u32* hdr = reinterpret_cast<u32*>(s + L.hdr);
    uint2* open = reinterpret_cast<uint2*>(s + L.open);
    uint4* totals = reinterpret_cast<uint4*>(s + L.totals);
    uint4* marker = reinterpret_cast<uint4*>(s + L.marker);
    uint4* bsum = reinterpret_cast<uint4*>(s + L.bsum);
    uint4* bbase = reinterpret_cast<uint4*>(s + L.bbase);
    const u32* rec = reinterpret_cast<const u32*>(d_rec);
    u32* dg = reinterpret_cast<u32*>(d_dg);
    const long long n = (long long)nslots;
    hipError_t e = hipMemsetAsync(hdr, 0, H_WORDS * sizeof(u32), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(vit_dg_presence_kernel, dim3(grid_for(n, 4u * 256u, 2048u)), dim3(256), 0, stream, rec, n, hdr);
    if (L.nchunks > 1u)
        hipLaunchKernelGGL(vit_dg_link_kernel<false>, dim3(L.nchunks - 1u, NADDR), dim3(TILE), 0, stream, rec, n, hdr, totals, L.nchunks,
                           marker, open);
    hipLaunchKernelGGL(vit_dg_link_kernel<true>, dim3(L.nchunks, NADDR), dim3(TILE), 0, stream, rec, n, hdr, totals, L.nchunks, marker,
                       open);
    hipLaunchKernelGGL(vit_dg_sums_kernel, dim3(L.nblocks), dim3(NUM_TPB), 0, stream, rec, marker, n, bsum);
    hipLaunchKernelGGL(vit_dg_bases_kernel, dim3(1), dim3(NUM_TPB), 0, stream, bsum, L.nblocks, bbase, open, n, hdr);
    hipLaunchKernelGGL(vit_dg_place_kernel, dim3(L.nblocks), dim3(NUM_TPB), 0, stream, rec, marker, n, bbase, dg, max_groups,
                       d_data ? 1u : 0u, data_capacity, hdr);
    const long long bound = (long long)max_groups < n ? (long long)max_groups : n;
    hipLaunchKernelGGL(vit_dg_gather_kernel, dim3(grid_for(bound, 1u, GATHER_MAX_GRID)), dim3(WAVE), 0, stream, d_bytes, rec, n, hdr, dg,
                       reinterpret_cast<u32*>(d_sum), d_data);
    return hipGetLastError();
}

// ---- the host twin: the walk per address ---------------------------------------------------------------------------------------
void vit_data_groups_host_impl(const uint8_t* bytes, const vit_packet_rec* rec_, int64_t nslots, vit_dgroup_rec* dg_, uint32_t max_groups,
                               vit_dgroup_summary* sum_, uint8_t* data, uint32_t data_capacity) {
    struct Walk {
        bool any, closed, head_first, last;
        u32 cont, head, npk, bytes;
    };
    std::vector<Walk> st(NADDR, Walk{false, false, false, false, 0, 0, 0, 0});
    std::vector<uint8_t> D;
    u32 ngroups = 0, nwritten = 0, data_bytes = 0, used = 0, dropped = 0, unusable = 0, open_from = (u32)nslots;
    auto word = [&](int64_t i, int w) {
        u32 v;
        memcpy(&v, reinterpret_cast<const uint8_t*>(rec_) + 8 * i + 4 * w, 4);
        return v;
    };
    for (int64_t i = 0; i < nslots; i++) {
        const u32 w0 = word(i, 0), w1 = word(i, 1);
        if (!rec_usable(w0, w1, (u64)i, (u64)nslots)) {
            if (rec_kind(w0) == VIT_PKT_DATA) unusable++;
            continue;
        }
        const u32 fl = rec_flags(w0), cont = fl & 3u, A = rec_addr(w1);
        Walk& w = st[A];
        const bool goes_on = w.any && !(fl & VIT_PKT_FIRST) && !w.last && cont == ((w.cont + 1u) & 3u);
        if (!goes_on) {
            if (w.any && !w.closed) dropped += w.npk;
            w = Walk{true, false, (fl & VIT_PKT_FIRST) != 0, false, 0, (u32)i, 0, 0};
        }
        w.cont = cont;
        w.last = (fl & VIT_PKT_LAST) != 0;
        w.npk++;
        w.bytes += rec_useful(w1);
        if (!w.last || !w.head_first) continue;
        w.closed = true;
        used += w.npk;
        const u32 k = ngroups++, off = data_bytes, L = w.bytes;
        data_bytes += roundup_dg(L);
        if (k != nwritten || k >= max_groups || (data && (u64)off + L > (u64)data_capacity)) continue;
        nwritten++;
        D.clear();
        for (int64_t j = w.head; j <= i; j++) {
            const u32 v0 = word(j, 0), v1 = word(j, 1);
            if (rec_usable(v0, v1, (u64)j, (u64)nslots) && rec_addr(v1) == A)
                D.insert(D.end(), bytes + SLOT * j + PKT_DATA_OFFSET, bytes + SLOT * j + PKT_DATA_OFFSET + rec_useful(v1));
        }
        if (data && L) memcpy(data + off, D.data(), L);
        bool match = false;
        if (L >= DG_CRC_BYTES) {
            u32 r = 0xFFFFu;
            for (u32 b = 0; b < L - DG_CRC_BYTES; b++) r = crc16_step(r, D[b]);
            match = (r ^ 0xFFFFu) == ((u32)D[L - 2u] << 8 | D[L - 1u]);
        }
        uint8_t h[DG_HDR_PEEK] = {};
        for (u32 b = 0; b < DG_HDR_PEEK && b < L; b++) h[b] = D[b];
        u32 words[8];
        dg_record_words(words, w.head, (u32)i, w.npk, off, L, A, dg_parse(h, L, match), (rec_flags(word(w.head, 0)) >> 4) & 1u);
        memcpy(reinterpret_cast<uint8_t*>(dg_) + 32 * (size_t)k, words, 32);
    }
    for (u32 A = 0; A < NADDR; A++) {
        const Walk& w = st[A];
        if (!w.any || w.closed) continue;
        if (w.head_first && !w.last) open_from = w.head < open_from ? w.head : open_from;
        else dropped += w.npk;
    }
    const u32 words[8] = {ngroups, nwritten, data_bytes, open_from, used, dropped, unusable, 0};
    memcpy(sum_, words, 32);
}
