// vit_dgroup_dev.h -- the device routines of the data group passes, one text each: presence, link, the prefix sum's three
// parts and the gather, with the record and header arithmetic that the host twin shares.  vit_dgroup.hip uses them in the
// per-stream kernels (one stream per launch), vit_dgroup_table.hip in the table kernels (up to 64 streams per launch); what
// differs between the two is only where a workgroup's stream and its share of the stream come from.  How the passes work
// is written out at the head of vit_dgroup.hip; the format's constants are in vit_packet_fmt.h, the CRC arithmetic in
// vit_crc_dev.h.  A routine takes one stream's pointers and counts, and slot indices are that stream's own.
#pragma once
#include "vit_crc_dev.h"
#include "vit_internal.h"
#include "vit_packet_fmt.h"

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
__host__ __device__ inline Layout layout(int64_t nslots) {
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
constexpr u32 PRES_TPB = 256;
// workgroup `block` of the stream's `nblocks` (256 threads); s_bits: NADDR / 32 words, s_cnt: 2
__device__ __forceinline__ void dg_presence(const u32* __restrict__ rec, long long nslots, u32* __restrict__ hdr, u32 block, u32 nblocks,
                                            u32* s_bits, u32* s_cnt) {
    if (threadIdx.x < NADDR / 32u) s_bits[threadIdx.x] = 0;
    if (threadIdx.x < 2u) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    u32 usable = 0, unusable = 0;
    for (long long i = (long long)block * 256 + threadIdx.x; i < nslots; i += (long long)nblocks * 256) {
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
// The workgroup (TILE threads) of address A and chunk `chunk` of the stream's nchunks; s_tot: the wavefronts' totals, twice.
template <bool EMIT>
__device__ __forceinline__ void dg_link(const u32* __restrict__ rec, long long nslots, const u32* __restrict__ hdr, uint4* totals,
                                        u32 nchunks, uint4* __restrict__ marker, uint2* __restrict__ open, u32 A, u32 chunk,
                                        uint4 (*s_tot)[TILE / WAVE]) {
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

// block `block` of the stream's prefix sum (NUM_TPB threads); s_w: a pair per wavefront, s_out: 2 words, s_used: 1
__device__ __forceinline__ void dg_sums(const u32* __restrict__ rec, const uint4* __restrict__ marker, long long nslots,
                                        uint4* __restrict__ bsum, u32 block, u32 (*s_w)[2], u32* s_out, u32& s_used) {
    if (threadIdx.x == 0) s_used = 0;
    u32 g = 0, by = 0, used = 0;
    const long long i0 = (long long)block * NUM_BLOCK + (long long)threadIdx.x * NUM_PER;
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
    if (threadIdx.x == 0) bsum[block] = make_uint4(s_out[0], s_out[1], s_used, 0u);
}

// one workgroup of 1024 for a stream: the bases of the blocks, the totals, and over the addresses open_from and the open
// runs' packets; s_red: 3 words
__device__ __forceinline__ void dg_bases(const uint4* __restrict__ bsum, u32 nblocks, uint4* __restrict__ bbase,
                                         const uint2* __restrict__ open, long long nslots, u32* hdr, u32 (*s_w)[2], u32* s_out,
                                         u32* s_red) {
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

// block `block` again, with the bases: dg is the stream's first record, the numbers and offsets its own
__device__ __forceinline__ void dg_place(const u32* __restrict__ rec, const uint4* __restrict__ marker, long long nslots,
                                         const uint4* __restrict__ bbase, u32* __restrict__ dg, u32 max_groups, u32 has_data,
                                         u32 capacity, u32* hdr, u32 block, u32 (*s_w)[2], u32* s_out) {
    const long long i0 = (long long)block * NUM_BLOCK + (long long)threadIdx.x * NUM_PER;
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
    const uint4 base = bbase[block];
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

// the stream's summary, by one lane
__device__ __forceinline__ void dg_summary(const u32* __restrict__ hdr, u32 ngroups, u32 nwritten, u32* __restrict__ sum) {
    sum[0] = ngroups;
    sum[1] = nwritten;
    sum[2] = hdr[H_DATA_BYTES];
    sum[3] = hdr[H_OPEN_FROM];
    sum[4] = hdr[H_USED];
    sum[5] = hdr[H_USABLE] - hdr[H_USED] - hdr[H_OPEN_PK];
    sum[6] = hdr[H_UNUSABLE];
    sum[7] = 0;
}

// Written group k < nwritten of the stream, by one wavefront (the whole workgroup): dg is the stream's first record, data
// its block (or nullptr).  LDS: s_hdr 16 bytes, s_tail DG_CRC_BYTES, s_list 2 * GATHER_STEP words (slot | useful << 24 of
// the group's packets not gathered yet), s_row a row per lane (an odd stride: the rows start on different banks).
__device__ __forceinline__ void dg_gather_group(const uint8_t* __restrict__ bytes, const u32* __restrict__ rec, long long nslots, u32* dg,
                                                uint8_t* __restrict__ data, u32 k, uint8_t* s_hdr, uint8_t* s_tail, u32* s_list,
                                                u32 (*s_row)[GATHER_ROW_DWORDS + 1u]) {
    const u32 lane = threadIdx.x;
    const uint8_t* bytes_end = bytes + (u64)SLOT * (u64)nslots;
    {
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

}  // namespace
