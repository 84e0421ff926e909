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
#include "vit_crc_dev.h"
#include "vit_internal.h"
#include "vit_packet_fmt.h"

#include <cstring>
#include <vector>

namespace {

using namespace pktfmt;
typedef uint32_t u32;
typedef uint64_t u64;
constexpr u32 WAVE = 64;
constexpr u32 TILE = 1024;                     // link: threads of a workgroup = slots of a tile
constexpr u32 CHUNK_TILES = 16;
constexpr u32 CHUNK = TILE * CHUNK_TILES;      // 16384 slots per link workgroup
constexpr u32 NUM_TPB = 1024, NUM_PER = 4;
constexpr u32 NUM_BLOCK = NUM_TPB * NUM_PER;   // 4096 slots per workgroup of the prefix sum
constexpr u32 GATHER_STEP = WAVE;              // packets (and slots of the search for them) a wavefront takes per step
// (the four slot counts stand again in viterbi.dll_amd/__init__.py, DGROUP_GEOMETRY: the tests take their edges from it)
constexpr u32 GATHER_MAX_GRID = 4096;
static_assert(TILE == NADDR, "the summary kernel takes an address per thread");
static_assert(DG_MAX_SLOTS <= (1 << 24) && MAX_USEFUL < 256u, "the gather lists a packet as slot | useful << 24");

// scratch: header words
enum { H_BITS = 0, H_UNUSABLE = 32, H_USABLE, H_FIRST_UNWRITTEN, H_NGROUPS, H_DATA_BYTES, H_OPEN_FROM, H_USED, H_OPEN_PK, H_WORDS = 64 };

struct Layout {
    size_t hdr, open, totals, marker, bsum, bbase, end;
    u32 nchunks, nblocks;
};
Layout layout(int64_t nslots) {
    Layout L;
    L.nchunks = (u32)((nslots + CHUNK - 1) / CHUNK);
    L.nblocks = (u32)((nslots + NUM_BLOCK - 1) / NUM_BLOCK);
    L.hdr = 0;
    L.open = L.hdr + H_WORDS * sizeof(u32);
    L.totals = L.open + NADDR * sizeof(uint2);
    L.marker = L.totals + (L.nchunks > 1 ? (size_t)NADDR * L.nchunks * sizeof(uint4) : 0);
    L.bsum = L.marker + (size_t)nslots * sizeof(uint4);
    L.bbase = L.bsum + (size_t)L.nblocks * sizeof(uint4);
    L.end = L.bbase + (size_t)L.nblocks * sizeof(uint4);
    return L;
}

// ---- a record, as its two words ------------------------------------------------------------------------------------------
__host__ __device__ inline u32 rec_kind(u32 w0) { return w0 & 0xFFu; }
__host__ __device__ inline u32 rec_flags(u32 w0) { return w0 >> 24; }
__host__ __device__ inline u32 rec_addr(u32 w1) { return w1 & 0xFFFFu; }
__host__ __device__ inline u32 rec_useful(u32 w1) { return (w1 >> 16) & 0xFFu; }
__host__ __device__ inline bool rec_usable(u32 w0, u32 w1, u64 slot, u64 nslots) {
    const u32 n = (w0 >> 16) & 0xFFu;
    return rec_kind(w0) == VIT_PKT_DATA && ((w0 >> 8) & 0xFFu) == 1u && rec_addr(w1) < NADDR && rec_useful(w1) + PKT_OVERHEAD <= SLOT * n &&
           slot + n <= nslots;
}
__host__ __device__ inline u32 roundup_dg(u32 n) { return (n + DG_ALIGN - 1u) & ~(DG_ALIGN - 1u); }

// ---- the header of a group: one text for the kernel and the host twin -------------------------------------------------------
// h: D[0 ... DG_HDR_PEEK), of which only the bytes below L are looked at
struct DgHeader {
    u32 type, cont_rep, flags, segment, transport_id, payload_offset;
};
__host__ __device__ inline DgHeader dg_parse(const uint8_t* h, u32 L, bool crc_match) {
    DgHeader H = {0, 0, 0, 0, 0, 0};
    if (L < DG_FIXED_BYTES) return H;
    const u32 b0 = h[0];
    H.type = b0 & DG_TYPE_MASK;
    H.cont_rep = h[1];
    const u32 E = L - ((b0 & DG_CRC) ? DG_CRC_BYTES : 0u);
    u32 p = DG_FIXED_BYTES, flags = DGF_WELLFORMED, segment = 0, tid = 0;
    bool ok = true;
    if (b0 & DG_CRC) flags |= DGF_CRCF;
    if (b0 & DG_EXT) {
        flags |= DGF_EXT;
        p += DG_EXT_BYTES;
    }
    if (b0 & DG_SEG) {
        flags |= DGF_SEG;
        if (p + DG_SEG_BYTES <= E) segment = (u32)h[p] << 8 | h[p + 1u];
        else ok = false;
        p += DG_SEG_BYTES;
    }
    if (ok && (b0 & DG_UA)) {
        flags |= DGF_UA;
        if (p + 1u <= E) {
            const u32 li = h[p] & DG_UA_LI_MASK, tidf = h[p] & DG_UA_TIDF;
            p += 1u;
            if (tidf) {
                flags |= DGF_TIDF;
                if (li >= DG_TID_BYTES && p + DG_TID_BYTES <= E) tid = (u32)h[p] << 8 | h[p + 1u];
                else ok = false;
            }
            p += li;
        } else {
            ok = false;
        }
    }
    if (!ok || p > E) return H;
    if ((b0 & DG_CRC) && crc_match) flags |= DGF_CRC_OK;
    H.flags = flags;
    H.segment = segment;
    H.transport_id = tid;
    H.payload_offset = p;
    return H;
}
__host__ __device__ inline void dg_record_words(u32* w, u32 first, u32 last, u32 npk, u32 off, u32 L, u32 addr, const DgHeader& H,
                                                u32 command) {
    w[0] = first;
    w[1] = last;
    w[2] = npk;
    w[3] = off;
    w[4] = L;
    w[5] = addr | H.segment << 16;
    w[6] = H.transport_id | H.payload_offset << 16;
    w[7] = H.type | H.cont_rep << 8 | H.flags << 16 | command << 24;
}

// ---- presence --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vit_dg_presence_kernel(const u32* __restrict__ rec, long long nslots, u32* __restrict__ hdr) {
    __shared__ u32 s_bits[NADDR / 32u], s_cnt[2];
    if (threadIdx.x < NADDR / 32u) s_bits[threadIdx.x] = 0;
    if (threadIdx.x < 2u) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    u32 usable = 0, unusable = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nslots; i += (long long)gridDim.x * 256) {
        const u32 w0 = rec[2 * i], w1 = rec[2 * i + 1];
        if (rec_usable(w0, w1, (u64)i, (u64)nslots)) {
            usable++;
            atomicOr(&s_bits[rec_addr(w1) >> 5], 1u << (rec_addr(w1) & 31u));
        } else if (rec_kind(w0) == VIT_PKT_DATA) {
            unusable++;
        }
    }
    if (usable) atomicAdd(&s_cnt[0], usable);
    if (unusable) atomicAdd(&s_cnt[1], unusable);
    __syncthreads();
    if (threadIdx.x < NADDR / 32u && s_bits[threadIdx.x]) atomicOr(&hdr[H_BITS + threadIdx.x], s_bits[threadIdx.x]);
    if (threadIdx.x == 0 && s_cnt[0]) atomicAdd(&hdr[H_USABLE], s_cnt[0]);
    if (threadIdx.x == 1 && s_cnt[1]) atomicAdd(&hdr[H_UNUSABLE], s_cnt[1]);
}

// ---- link -------------------------------------------------------------------------------------------------------------------
// What a stretch of one address's usable packets hands on.  w0: bit 0 not empty; of the first packet bit 1 first flag,
// bits 3..2 continuity; of the last packet bit 4 last flag, bits 6..5 continuity; bit 7 the last run began at the stretch's
// first packet; bit 8 the last run's head has the first flag.  head, npk, bytes: of the last run.
struct RunState {
    u32 w0, head, npk, bytes;
};
constexpr u32 RS_VALID = 1, RS_FF = 2, RS_FC_SHIFT = 2, RS_LL = 16, RS_LC_SHIFT = 5, RS_WHOLE = 128, RS_HF = 256;
constexpr u32 RS_FIRST_MASK = RS_FF | 3u << RS_FC_SHIFT, RS_LAST_MASK = RS_LL | 3u << RS_LC_SHIFT;

__device__ __forceinline__ RunState run_leaf(u32 flags, u32 slot, u32 useful) {
    const u32 cont = flags & 3u, first = flags & VIT_PKT_FIRST ? 1u : 0u, last = flags & VIT_PKT_LAST ? 1u : 0u;
    RunState r;
    r.w0 = RS_VALID | first * RS_FF | cont << RS_FC_SHIFT | last * RS_LL | cont << RS_LC_SHIFT | RS_WHOLE | first * RS_HF;
    r.head = slot;
    r.npk = 1;
    r.bytes = useful;
    return r;
}
// a, then b
__device__ __forceinline__ RunState run_join(const RunState a, const RunState b) {
    const bool link = !(b.w0 & RS_FF) && !(a.w0 & RS_LL) && ((b.w0 >> RS_FC_SHIFT) & 3u) == (((a.w0 >> RS_LC_SHIFT) + 1u) & 3u);
    const bool on = link && (b.w0 & RS_WHOLE);  // b's only run goes on a's last
    const bool only_a = !(b.w0 & RS_VALID), only_b = !(a.w0 & RS_VALID);
    const u32 w0 = RS_VALID | (a.w0 & RS_FIRST_MASK) | (b.w0 & RS_LAST_MASK) | (on ? a.w0 & (RS_WHOLE | RS_HF) : b.w0 & RS_HF);
    RunState r;  // selects only: no branch, nothing in memory
    r.w0 = only_a ? a.w0 : only_b ? b.w0 : w0;
    r.head = only_a || (on && !only_b) ? a.head : b.head;
    r.npk = only_a ? a.npk : only_b || !on ? b.npk : a.npk + b.npk;
    r.bytes = only_a ? a.bytes : only_b || !on ? b.bytes : a.bytes + b.bytes;
    return r;
}
__device__ __forceinline__ RunState run_shfl_up(const RunState& x, u32 d) {
    RunState o;
    o.w0 = __shfl_up(x.w0, d, WAVE);
    o.head = __shfl_up(x.head, d, WAVE);
    o.npk = __shfl_up(x.npk, d, WAVE);
    o.bytes = __shfl_up(x.bytes, d, WAVE);
    return o;
}
__device__ __forceinline__ RunState run_from(const uint4& v) { return RunState{v.x, v.y, v.z, v.w}; }
__device__ __forceinline__ uint4 run_words(const RunState& r) { return make_uint4(r.w0, r.head, r.npk, r.bytes); }

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

// ---- number -----------------------------------------------------------------------------------------------------------------
// the sums of a and b over the workgroup in s_out[0], s_out[1]; a and b become the sums of the threads before this one
__device__ __forceinline__ void block_scan2(u32& a, u32& b, u32 (*s_w)[2], u32* s_out) {
    const u32 tid = threadIdx.x, lane = tid & (WAVE - 1u), wave = tid / WAVE, nw = blockDim.x / WAVE;
    u32 ia = a, ib = b;
#pragma unroll
    for (u32 d = 1; d < WAVE; d <<= 1) {
        const u32 oa = __shfl_up(ia, d, WAVE), ob = __shfl_up(ib, d, WAVE);
        if (lane >= d) {
            ia += oa;
            ib += ob;
        }
    }
    if (lane == WAVE - 1u) {
        s_w[wave][0] = ia;
        s_w[wave][1] = ib;
    }
    __syncthreads();
    u32 pa = 0, pb = 0, ta = 0, tb = 0;
    for (u32 k = 0; k < nw; k++) {
        if (k == wave) {
            pa = ta;
            pb = tb;
        }
        ta += s_w[k][0];
        tb += s_w[k][1];
    }
    a = pa + ia - a;
    b = pb + ib - b;
    if (tid == 0) {
        s_out[0] = ta;
        s_out[1] = tb;
    }
    __syncthreads();
}

// the marker of slot i if a group closes there
__device__ __forceinline__ bool group_at(const u32* __restrict__ rec, const uint4* __restrict__ marker, long long i, long long nslots,
                                         uint4& m) {
    if (i >= nslots) return false;
    const u32 w0 = rec[2 * i], w1 = rec[2 * i + 1];
    if (!rec_usable(w0, w1, (u64)i, (u64)nslots) || !(rec_flags(w0) & VIT_PKT_LAST)) return false;
    m = marker[i];
    return m.x != 0u;
}

__global__ __launch_bounds__(NUM_TPB) void vit_dg_sums_kernel(const u32* __restrict__ rec, const uint4* __restrict__ marker,
                                                              long long nslots, uint4* __restrict__ bsum) {
    __shared__ u32 s_w[NUM_TPB / WAVE][2], s_out[2], s_used;
    if (threadIdx.x == 0) s_used = 0;
    u32 g = 0, by = 0, used = 0;
    const long long i0 = (long long)blockIdx.x * NUM_BLOCK + (long long)threadIdx.x * NUM_PER;
    for (u32 j = 0; j < NUM_PER; j++) {
        uint4 m;
        if (group_at(rec, marker, i0 + j, nslots, m)) {
            g++;
            by += roundup_dg(m.z);
            used += m.y;
        }
    }
    block_scan2(g, by, s_w, s_out);
    if (used) atomicAdd(&s_used, used);  // LDS, an integer sum
    __syncthreads();
    if (threadIdx.x == 0) bsum[blockIdx.x] = make_uint4(s_out[0], s_out[1], s_used, 0u);
}

// one workgroup of 1024: the bases of the blocks, the totals, and over the addresses open_from and the open runs' packets
__global__ __launch_bounds__(NUM_TPB) void vit_dg_bases_kernel(const uint4* __restrict__ bsum, u32 nblocks, uint4* __restrict__ bbase,
                                                               const uint2* __restrict__ open, long long nslots, u32* hdr) {
    __shared__ u32 s_w[NUM_TPB / WAVE][2], s_out[2], s_red[3];
    const u32 tid = threadIdx.x;
    const u32 per = (nblocks + NUM_TPB - 1u) / NUM_TPB;
    u32 g = 0, by = 0, used = 0;
    for (u32 j = 0; j < per; j++) {
        const u32 b = tid * per + j;
        if (b < nblocks) {
            const uint4 v = bsum[b];
            g += v.x;
            by += v.y;
            used += v.z;
        }
    }
    if (tid < 3u) s_red[tid] = tid == 0 ? 0xFFFFFFFFu : 0u;
    block_scan2(g, by, s_w, s_out);
    for (u32 j = 0; j < per; j++) {
        const u32 b = tid * per + j;
        if (b < nblocks) {
            bbase[b] = make_uint4(g, by, 0u, 0u);
            const uint4 v = bsum[b];
            g += v.x;
            by += v.y;
        }
    }
    u32 cand = 0xFFFFFFFFu, opk = 0;
    if ((hdr[H_BITS + (tid >> 5)] >> (tid & 31u)) & 1u) {
        const uint2 o = open[tid];
        cand = o.x;
        opk = o.y;
    }
    if (cand != 0xFFFFFFFFu) atomicMin(&s_red[0], cand);  // LDS: a minimum and two integer sums
    if (opk) atomicAdd(&s_red[1], opk);
    if (used) atomicAdd(&s_red[2], used);
    __syncthreads();
    if (tid == 0) {
        hdr[H_NGROUPS] = s_out[0];
        hdr[H_DATA_BYTES] = s_out[1];
        hdr[H_USED] = s_red[2];
        hdr[H_OPEN_PK] = s_red[1];
        hdr[H_OPEN_FROM] = s_red[0] < (u32)nslots ? s_red[0] : (u32)nslots;
        hdr[H_FIRST_UNWRITTEN] = 0xFFFFFFFFu;
    }
}

__global__ __launch_bounds__(NUM_TPB) void vit_dg_place_kernel(const u32* __restrict__ rec, const uint4* __restrict__ marker,
                                                               long long nslots, const uint4* __restrict__ bbase, u32* __restrict__ dg,
                                                               u32 max_groups, u32 has_data, u32 capacity, u32* hdr) {
    __shared__ u32 s_w[NUM_TPB / WAVE][2], s_out[2];
    const long long i0 = (long long)blockIdx.x * NUM_BLOCK + (long long)threadIdx.x * NUM_PER;
    uint4 m[NUM_PER];
    bool is[NUM_PER];
    u32 g = 0, by = 0;
#pragma unroll
    for (u32 j = 0; j < NUM_PER; j++) {
        is[j] = group_at(rec, marker, i0 + j, nslots, m[j]);
        if (is[j]) {
            g++;
            by += roundup_dg(m[j].z);
        }
    }
    block_scan2(g, by, s_w, s_out);
    const uint4 base = bbase[blockIdx.x];
    u32 k = base.x + g, off = base.y + by;
#pragma unroll
    for (u32 j = 0; j < NUM_PER; j++) {
        if (!is[j]) continue;
        const u32 L = m[j].z;
        if (k < max_groups && (!has_data || (u64)off + L <= (u64)capacity)) {
            u32* o = dg + 8u * (size_t)k;
            o[0] = m[j].x - 1u;
            o[1] = (u32)(i0 + j);
            o[2] = m[j].y;
            o[3] = off;
            o[4] = L;
        } else {
            atomicMin(&hdr[H_FIRST_UNWRITTEN], k);
        }
        k++;
        off += roundup_dg(L);
    }
}

// ---- gather -----------------------------------------------------------------------------------------------------------------
struct XPow {
    uint16_t v[MAX_USEFUL + 1];
};
constexpr XPow make_xpow() {
    XPow t{};
    for (u32 n = 0; n <= MAX_USEFUL; n++) t.v[n] = (uint16_t)crc_xpow(n, 1u);
    return t;
}
__device__ const XPow g_xpow = make_xpow();  // x^(8n) mod g

constexpr u32 GATHER_ROW_DWORDS = (3u + MAX_USEFUL + 3u) / 4u;  // 24: a packet's data at any phase in 4 bytes
// the aligned dword at p, whose first byte lies inside the stream; the bytes at and behind `end` are not read
__device__ __forceinline__ u32 load_dword_inside(const uint8_t* p, const uint8_t* end) {
    if (p + 4 <= end) return *reinterpret_cast<const u32*>(p);
    u32 v = 0;
    for (u32 j = 0; j < 3u; j++)
        if (p + j < end) v |= (u32)p[j] << (8u * j);
    return v;
}

__global__ __launch_bounds__(WAVE) void vit_dg_gather_kernel(const uint8_t* __restrict__ bytes, const u32* __restrict__ rec,
                                                             long long nslots, const u32* __restrict__ hdr, u32* dg,
                                                             u32* __restrict__ sum, uint8_t* __restrict__ data) {
    __shared__ uint8_t s_hdr[16], s_tail[DG_CRC_BYTES];
    __shared__ u32 s_list[2u * GATHER_STEP];  // slot | useful << 24 of the group's packets not gathered yet
    __shared__ u32 s_row[WAVE][GATHER_ROW_DWORDS + 1u];  // (an odd stride: the lanes' rows start on different banks)
    const u32 lane = threadIdx.x;
    const uint8_t* bytes_end = bytes + (u64)SLOT * (u64)nslots;
    const u32 ngroups = hdr[H_NGROUPS];
    const u32 nwritten = hdr[H_FIRST_UNWRITTEN] < ngroups ? hdr[H_FIRST_UNWRITTEN] : ngroups;
    if (blockIdx.x == 0 && lane == 0) {
        sum[0] = ngroups;
        sum[1] = nwritten;
        sum[2] = hdr[H_DATA_BYTES];
        sum[3] = hdr[H_OPEN_FROM];
        sum[4] = hdr[H_USED];
        sum[5] = hdr[H_USABLE] - hdr[H_USED] - hdr[H_OPEN_PK];
        sum[6] = hdr[H_UNUSABLE];
        sum[7] = 0;
    }
    for (u32 k = blockIdx.x; k < nwritten; k += gridDim.x) {  // the same trips for the whole workgroup (one wavefront)
        u32* o = dg + 8u * (size_t)k;
        const u32 first = o[0], last = o[1], npk = o[2], off = o[3], L = o[4];
        const u32 A = rec_addr(rec[2 * (size_t)last + 1]);
        const u32 command = (rec_flags(rec[2 * (size_t)first]) >> 4) & 1u;
        const u32 ncrc = L >= DG_CRC_BYTES ? L - DG_CRC_BYTES : 0u;  // the bytes the group's CRC covers, if it has one
        u32 S = 0xFFFFu, done = 0, nlist = 0;
        for (u32 base = first; base <= last; base += GATHER_STEP) {
            // the group's packets among the next 64 slots go onto a list, in slot order; 64 packets of the list are a step
            const u32 slot = base + lane;
            u32 w0 = 0, w1 = 0;
            if (slot <= last) {
                w0 = rec[2 * (size_t)slot];
                w1 = rec[2 * (size_t)slot + 1];
            }
            const bool mine = slot <= last && rec_usable(w0, w1, (u64)slot, (u64)nslots) && rec_addr(w1) == A;
            const u64 found = __ballot(mine);
            if (mine) s_list[nlist + (u32)__popcll(found & ((1ull << lane) - 1ull))] = slot | rec_useful(w1) << 24;  // < 63 + 64
            nlist += (u32)__popcll(found);
            const bool at_end = last - base < GATHER_STEP;
            while (nlist >= GATHER_STEP || (at_end && nlist)) {  // the same for every lane
            __syncthreads();
            const u32 n = nlist < GATHER_STEP ? nlist : GATHER_STEP;
            const u32 entry = lane < n ? s_list[lane] : 0u;
            const u32 behind = lane + GATHER_STEP < nlist ? s_list[lane + GATHER_STEP] : 0u;
            __syncthreads();
            if (lane + GATHER_STEP < nlist) s_list[lane] = behind;
            nlist -= n;
            const u32 i = entry & 0xFFFFFFu, u = entry >> 24;  // (a lane without a packet: 0 bytes, nothing loaded)
            u32 incl = u;
#pragma unroll
            for (u32 d = 1; d < WAVE; d <<= 1) {
                const u32 v = __shfl_up(incl, d, WAVE);
                if (lane >= d) incl += v;
            }
            const u32 at = done + incl - u;  // D[at ...) are this packet's
            done += __shfl(incl, WAVE - 1u, WAVE);
            // the packet's data into the lane's own LDS row as the aligned dwords that hold it - the loads all in flight
            // together - then out of the row a dword of the destination at a time
            const uint8_t* src = bytes + (u64)SLOT * i + PKT_DATA_OFFSET;
            const u32 lead = (u32)(reinterpret_cast<uintptr_t>(src) & 3u);
            const u32 un = at < L ? (u < L - at ? u : L - at) : 0u;  // (= u: the link pass summed the same lengths)
            const u32 ndw = un ? (lead + un + 3u) >> 2 : 0u;
            u32* row = s_row[lane];
#pragma unroll
            for (u32 w = 0; w < GATHER_ROW_DWORDS; w++)
                if (w < ndw) row[w] = load_dword_inside(src - lead + 4u * w, bytes_end);
            const uint8_t* rb = reinterpret_cast<const uint8_t*>(row) + lead;
            uint8_t* dst = data ? data + off : nullptr;
            u32 r = 0, cnt = 0;
            for (u32 pos = 0; pos < un;) {
                const u32 idx = at + pos;
                u32 nb = un - pos < 4u ? un - pos : 4u;
                const u32 mis = dst ? (u32)(reinterpret_cast<uintptr_t>(dst + idx) & 3u) : 0u;
                if (mis && nb > 4u - mis) nb = 4u - mis;
                u32 word = 0;
#pragma unroll
                for (u32 j = 0; j < 4u; j++) {
                    if (j >= nb) break;
                    const u32 b = rb[pos + j], q = idx + j;
                    word |= b << (8u * j);
                    if (q < ncrc) {
                        r = crc16_step(r, b);
                        cnt++;
                    } else {
                        s_tail[q - ncrc] = (uint8_t)b;  // q < L, and L >= 2 if ncrc > 0: one of the last two bytes
                    }
                    if (q < DG_HDR_PEEK) s_hdr[q] = (uint8_t)b;
                }
                if (dst) {
                    if (nb == 4u) {
                        *reinterpret_cast<u32*>(dst + idx) = word;
                    } else {
                        for (u32 j = 0; j < nb; j++) dst[idx + j] = (uint8_t)(word >> (8u * j));
                    }
                }
                pos += nb;
            }
            // (r, x^(8 cnt)) of the lanes in slot order: (ra, ma) then (rb, mb) = (ra * mb + rb, ma * mb)
            u32 mlt = g_xpow.v[cnt];
#pragma unroll
            for (u32 d = 1; d < WAVE; d <<= 1) {
                const u32 rb = __shfl_down(r, d, WAVE), mb = __shfl_down(mlt, d, WAVE);
                if (lane + d < WAVE) {
                    r = crc_mulg(r, mb) ^ rb;
                    mlt = crc_mulg(mlt, mb);
                }
            }
            S = crc_mulg(S, mlt) ^ r;  // lane 0's is the step's
            }
        }
        __syncthreads();
        if (lane == 0) {
            const bool match = L >= DG_CRC_BYTES && (S ^ 0xFFFFu) == ((u32)s_tail[0] << 8 | s_tail[1]);
            const DgHeader H = dg_parse(s_hdr, L, match);
            dg_record_words(o, first, last, npk, off, L, A, H, command);
        }
        __syncthreads();  // s_hdr and s_tail are read before the next group's bytes arrive
    }
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
