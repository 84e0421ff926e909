// vit_dgroup_table.hip -- data groups over a table of streams in a fixed number of launches (include/viterbi_amd.h,
// vit_data_groups_table_dev): the kernels of vit_dgroup.hip with each workgroup's stream, its share of the stream and the
// stream's arrays taken from the table (vit_internal.h, VitDgTable).  The passes themselves are one text
// (vit_dgroup_dev.h); this unit holds the table lookups and the scratch's layout.  A workgroup never mixes streams: it
// finds its stream from blockIdx alone, in front of every barrier, and then counts slots, groups and bytes from that
// stream's 0.
//
// Scratch: the streams' 256-byte headers back to back (one memset clears them), then per stream the arrays of
// vit_dgroup.hip's Layout behind its header - open runs, chunk totals (only with more than one chunk), markers, block
// sums, block bases - from 16 * scr0 on.
#include "vit_dgroup_dev.h"
#include "vit_internal.h"

namespace {

// one stream of the table, as the routines take it
struct DgView {
    const u32* rec;
    long long nslots;
    u32* hdr;
    uint2* open;
    uint4 *totals, *marker, *bsum, *bbase;
    u32 nchunks, nblocks;
};
__device__ __forceinline__ DgView dg_view(const VitDgTable& tab, u32 k, const u32* rec_all, uint8_t* scratch) {
    const VitDgEntry& e = tab.e[k];
    const Layout L = layout(e.nslots);
    uint8_t* s = scratch + 16ull * e.scr0;  // L.open of this stream
    DgView v;
    v.rec = rec_all + 2ull * e.rec0;
    v.nslots = (long long)e.nslots;
    v.hdr = reinterpret_cast<u32*>(scratch) + (size_t)H_WORDS * k;
    v.open = reinterpret_cast<uint2*>(s);
    v.totals = reinterpret_cast<uint4*>(s + (L.totals - L.open));
    v.marker = reinterpret_cast<uint4*>(s + (L.marker - L.open));
    v.bsum = reinterpret_cast<uint4*>(s + (L.bsum - L.open));
    v.bbase = reinterpret_cast<uint4*>(s + (L.bbase - L.open));
    v.nchunks = L.nchunks;
    v.nblocks = L.nblocks;
    return v;
}

// ---- presence: the stream's blocks of 4096 slots, a workgroup each ---------------------------------------------------------
__global__ __launch_bounds__(PRES_TPB) void vit_dg_table_presence_kernel(const u32* __restrict__ rec_all, uint8_t* scratch,
                                                                         const VitDgTable tab) {
    __shared__ u32 s_bits[NADDR / 32u], s_cnt[2];
    const u32 k = vit_table_find<VitDgEntry, &VitDgEntry::blk0>(tab.e, tab.nstreams, blockIdx.x);
    const DgView v = dg_view(tab, k, rec_all, scratch);
    dg_presence(v.rec, v.nslots, v.hdr, blockIdx.x - tab.e[k].blk0, v.nblocks, s_bits, s_cnt);
}

// ---- link: blockIdx.y the address, blockIdx.x a chunk of one stream ---------------------------------------------------------
// The totals launch leaves out every stream's last chunk: stream k's share starts at chunk0 - k (one chunk left out per
// earlier stream), and a stream of one chunk has none and is never the answer.
__device__ __forceinline__ u32 dg_find_totals(const VitDgTable& tab, u32 x) {
    u32 lo = 0, hi = tab.nstreams;  // e[0].chunk0 - 0 is 0
    while (hi - lo > 1u) {
        const u32 mid = (lo + hi) >> 1;
        if (tab.e[mid].chunk0 - mid <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}
template <bool EMIT>
__global__ __launch_bounds__(TILE) void vit_dg_table_link_kernel(const u32* __restrict__ rec_all, uint8_t* scratch, const VitDgTable tab) {
    __shared__ uint4 s_tot[2][TILE / WAVE];
    const u32 k = EMIT ? vit_table_find<VitDgEntry, &VitDgEntry::chunk0>(tab.e, tab.nstreams, blockIdx.x) : dg_find_totals(tab, blockIdx.x);
    const u32 chunk = blockIdx.x - (EMIT ? tab.e[k].chunk0 : tab.e[k].chunk0 - k);
    const DgView v = dg_view(tab, k, rec_all, scratch);
    dg_link<EMIT>(v.rec, v.nslots, v.hdr, v.totals, v.nchunks, v.marker, v.open, blockIdx.y, chunk, s_tot);
}

// ---- number: sums and place a workgroup per 4096 slots of one stream, bases a workgroup per stream -------------------------
__global__ __launch_bounds__(NUM_TPB) void vit_dg_table_sums_kernel(const u32* __restrict__ rec_all, uint8_t* scratch, const VitDgTable tab) {
    __shared__ u32 s_w[NUM_TPB / WAVE][2], s_out[2], s_used;
    const u32 k = vit_table_find<VitDgEntry, &VitDgEntry::blk0>(tab.e, tab.nstreams, blockIdx.x);
    const DgView v = dg_view(tab, k, rec_all, scratch);
    dg_sums(v.rec, v.marker, v.nslots, v.bsum, blockIdx.x - tab.e[k].blk0, s_w, s_out, s_used);
}

__global__ __launch_bounds__(NUM_TPB) void vit_dg_table_bases_kernel(const u32* __restrict__ rec_all, uint8_t* scratch, const VitDgTable tab) {
    __shared__ u32 s_w[NUM_TPB / WAVE][2], s_out[2], s_red[3];
    const DgView v = dg_view(tab, blockIdx.x, rec_all, scratch);
    dg_bases(v.bsum, v.nblocks, v.bbase, v.open, v.nslots, v.hdr, s_w, s_out, s_red);
}

__global__ __launch_bounds__(NUM_TPB) void vit_dg_table_place_kernel(const u32* __restrict__ rec_all, uint8_t* scratch, u32* __restrict__ dg,
                                                                     const VitDgTable tab) {
    __shared__ u32 s_w[NUM_TPB / WAVE][2], s_out[2];
    const u32 k = vit_table_find<VitDgEntry, &VitDgEntry::blk0>(tab.e, tab.nstreams, blockIdx.x);
    const VitDgEntry& e = tab.e[k];
    const DgView v = dg_view(tab, k, rec_all, scratch);
    dg_place(v.rec, v.marker, v.nslots, v.bbase, dg + 8ull * e.dg0, e.max_groups, e.has_data, e.capacity, v.hdr, blockIdx.x - e.blk0,
             s_w, s_out);
}

// ---- gather: the written groups of all streams numbered through, on the device ---------------------------------------------
// The grid comes from the host's bound, a pass per group that may be written: max(1, min(max_groups, nslots)) per stream,
// at most GATHER_MAX_GRID wavefronts.  Which groups ARE written only the headers say, so every wavefront first takes the
// streams' written counts, lane k stream k's, and their prefix sum: work item w of sum(nwritten) is group w - before[k] of
// the stream k whose range holds w, and the wavefronts stride over the items.  (Passes numbered by the host's bound instead -
// stream k's from gat0 on, those at or behind nwritten idle - put every stream's groups on the same few wavefronts when
// the bound is a multiple of the grid: 64 streams with max_groups 4096 and 150 groups each took 3.04 ms in this kernel
// against 0.044 ms for one stream's launch, profiles/HISTORY.md.)  Wavefront k < nstreams also writes stream k's summary:
// every stream owns at least one pass, so the grid is never shorter than the table.
static_assert(VIT_DG_MAX_STREAMS == WAVE, "a lane per stream");
__global__ __launch_bounds__(WAVE) void vit_dg_table_gather_kernel(const uint8_t* __restrict__ bytes, const u32* __restrict__ rec_all,
                                                                   const uint8_t* __restrict__ scratch, u32* dg, u32* __restrict__ sum,
                                                                   uint8_t* __restrict__ data, const VitDgTable tab) {
    __shared__ uint8_t s_hdr[16], s_tail[DG_CRC_BYTES];
    __shared__ u32 s_list[2u * GATHER_STEP];
    __shared__ u32 s_row[WAVE][GATHER_ROW_DWORDS + 1u];
    const u32 lane = threadIdx.x;
    const u32* hdrs = reinterpret_cast<const u32*>(scratch);
    u32 ngroups = 0, nwritten = 0;
    if (lane < tab.nstreams) {
        const u32* hdr = hdrs + (size_t)H_WORDS * lane;
        ngroups = hdr[H_NGROUPS];
        nwritten = hdr[H_FIRST_UNWRITTEN] < ngroups ? hdr[H_FIRST_UNWRITTEN] : ngroups;
    }
    if (blockIdx.x < tab.nstreams && lane == blockIdx.x) dg_summary(hdrs + (size_t)H_WORDS * lane, ngroups, nwritten, sum + 8ull * lane);
    u32 incl = nwritten;  // <= min(max_groups, nslots) each: the sum is at most ngat
#pragma unroll
    for (u32 d = 1; d < WAVE; d <<= 1) {
        const u32 v = __shfl_up(incl, d, WAVE);
        if (lane >= d) incl += v;
    }
    const u32 total = __shfl(incl, WAVE - 1u, WAVE);
    // the same trips for the whole workgroup (one wavefront); the item, its stream and its group are uniform
    for (u32 w = blockIdx.x; w < total; w += gridDim.x) {  // total <= 2^26 + 64, the grid at most 4096: no wrap
        const u32 k = (u32)__builtin_amdgcn_readfirstlane((int)__builtin_ctzll(__ballot(incl > w)));  // incl[63] = total > w
        const u32 g = w - (u32)__builtin_amdgcn_readfirstlane((int)(__shfl(incl, k, WAVE) - __shfl(nwritten, k, WAVE)));
        const VitDgEntry& e = tab.e[k];
        dg_gather_group(bytes + e.offset, rec_all + 2ull * e.rec0, (long long)e.nslots, dg + 8ull * e.dg0,
                        e.has_data ? data + e.data0 : nullptr, g, s_hdr, s_tail, s_list, s_row);
    }
}

}  // namespace

size_t vit_dg_table_geometry(VitDgTable* tab) {
    size_t at = (size_t)tab->nstreams * H_WORDS * sizeof(u32);
    u32 chunk = 0, blk = 0, gat = 0;
    for (u32 k = 0; k < tab->nstreams; k++) {
        VitDgEntry& e = tab->e[k];
        const Layout L = layout(e.nslots);
        e.scr0 = (u32)(at / 16u);  // at most 2^26 slots in the table: 1 GiB of markers and 66 MB of totals
        at += L.end - L.open;
        e.chunk0 = chunk;
        e.blk0 = blk;
        chunk += L.nchunks;
        blk += L.nblocks;
        gat += e.max_groups < e.nslots ? (e.max_groups ? e.max_groups : 1u) : e.nslots;
    }
    tab->nchunk = chunk;
    tab->nblk = blk;
    tab->ngat = gat;
    return at;
}

hipError_t vit_launch_data_groups_table(const uint8_t* d_bytes, const vit_packet_rec* d_rec, const VitDgTable& tab, vit_dgroup_rec* d_dg,
                                        vit_dgroup_summary* d_sum, uint8_t* d_data, void* d_scratch, hipStream_t stream) {
    uint8_t* s = static_cast<uint8_t*>(d_scratch);
    const u32* rec = reinterpret_cast<const u32*>(d_rec);
    u32* dg = reinterpret_cast<u32*>(d_dg);
    const hipError_t e = hipMemsetAsync(s, 0, (size_t)tab.nstreams * H_WORDS * sizeof(u32), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(vit_dg_table_presence_kernel, dim3(tab.nblk), dim3(PRES_TPB), 0, stream, rec, s, tab);
    if (tab.nchunk > tab.nstreams)  // some stream has more than one chunk
        hipLaunchKernelGGL(vit_dg_table_link_kernel<false>, dim3(tab.nchunk - tab.nstreams, NADDR), dim3(TILE), 0, stream, rec, s, tab);
    hipLaunchKernelGGL(vit_dg_table_link_kernel<true>, dim3(tab.nchunk, NADDR), dim3(TILE), 0, stream, rec, s, tab);
    hipLaunchKernelGGL(vit_dg_table_sums_kernel, dim3(tab.nblk), dim3(NUM_TPB), 0, stream, rec, s, tab);
    hipLaunchKernelGGL(vit_dg_table_bases_kernel, dim3(tab.nstreams), dim3(NUM_TPB), 0, stream, rec, s, tab);
    hipLaunchKernelGGL(vit_dg_table_place_kernel, dim3(tab.nblk), dim3(NUM_TPB), 0, stream, rec, s, dg, tab);
    hipLaunchKernelGGL(vit_dg_table_gather_kernel, dim3(tab.ngat < GATHER_MAX_GRID ? tab.ngat : GATHER_MAX_GRID), dim3(WAVE), 0, stream,
                       d_bytes, rec, s, dg, reinterpret_cast<u32*>(d_sum), d_data, tab);
    return hipGetLastError();
}
