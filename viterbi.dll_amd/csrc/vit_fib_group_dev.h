// vit_fib_group_dev.h -- what the units that resolve groups of G FIBs share, one text each: the workgroup's geometry, the
// walk over a FIB's FIGs, the FIG 0/2 service list, the per-FIB counts, the host twins' loop over a group's FIBs and the
// launch grid.  vit_mci.hip (sub-channel records) and vit_mci_dir.hip (service directory) are built on it.  It is for
// such .hip units alone: it opens their anonymous namespace (figfmt's names, u32 / u64) and holds their host helpers too.
//
// Shape.  A workgroup of 256 lanes makes passes; a pass resolves four groups (G <= 64: a wavefront per group, a lane per
// FIB) or one group (G > 64: tiles of 256 FIBs, a lane per FIB).  A group is one workgroup's.  A tile's FIBs come into LDS
// as aligned 16-byte windows (load_image: nothing outside the FIBs is read); each lane then takes its own FIB as nine
// dwords and one v_alignbyte per dword (image_row) into a row of 36 bytes - 9 dwords, odd, so the 64 lanes' byte reads at
// one offset meet on no bank - and walks it there byte by byte (fib_walk, or mci_walk's own text: no register is
// indexed with a run-time value).  A lane leaves its entries as two words each in LDS, entry j of lane l at [j][l]; a
// tile's entries are ordered by the key (FIB of the tile, entry of the FIB).  What a kernel makes of them is its own.
#pragma once
#include "vit_fig_fmt.h"
#include "vit_image_dev.h"

namespace {

using namespace figfmt;
typedef uint32_t u32;
typedef uint64_t u64;
constexpr u32 TPB = 256;
constexpr u32 WAVE = 64;
constexpr u32 SLOTS = TPB / WAVE;     // groups of a pass for G <= 64
constexpr u32 TILE = TPB;             // FIBs of a tile for G > 64
constexpr u32 ROW_DWORDS = 9;         // a lane's FIB in LDS: 32 bytes and one dword of skew
constexpr u32 IMG_BYTES = TILE * FIB_BYTES + 32u;  // a tile at any phase, whole windows, a 9th dword
constexpr u32 MAX_GRID = 1024;
constexpr u32 KEY_STRIDE = 16;        // entry j of FIB idx of the tile has the key idx * KEY_STRIDE + 1 + j; 0 is no entry's
static_assert(NSUBCH == WAVE && DIR_MAX == WAVE, "a lane per SubChId, a lane per record");
static_assert(MAX_ENTRIES <= KEY_STRIDE && DIR_MAX_ENTRIES <= KEY_STRIDE && TILE * KEY_STRIDE < (1u << 16), "keys");

struct FibLanes {
    u32 tid, lane, wave;  // (wave, lane) is also the (group of the pass, record) that this lane clears and writes out
    bool small;           // G <= 64: a wavefront per group
    u32 gpp, slot;        // groups per pass; this lane's FIB belongs to this group of the pass
    long long npasses;    // every lane of a workgroup makes the same passes and tiles: the barriers are uniform
};
__host__ __device__ __forceinline__ u32 fib_gpp(u32 G) { return G <= WAVE ? SLOTS : 1u; }
__host__ __device__ __forceinline__ long long fib_npasses(long long ngroups, u32 G) { return (ngroups + fib_gpp(G) - 1) / fib_gpp(G); }
__device__ __forceinline__ FibLanes fib_lanes(u32 G, long long ngroups) {
    const u32 tid = threadIdx.x, wave = tid / WAVE;
    return {tid, tid & (WAVE - 1u), wave, G <= WAVE, fib_gpp(G), G <= WAVE ? wave : 0u, fib_npasses(ngroups, G)};
}

struct FibPass {
    long long g0, f0;   // first group, first FIB
    u32 total, ntiles;  // FIBs (<= 4096) and tiles (1 for G <= 64)
};
__device__ __forceinline__ FibPass fib_pass(const FibLanes& L, long long pass, u32 G, long long nfibs) {
    const long long g0 = pass * L.gpp, f0 = g0 * G, fe = f0 + (long long)L.gpp * G < nfibs ? f0 + (long long)L.gpp * G : nfibs;
    const u32 total = (u32)(fe - f0);
    return {g0, f0, total, (total + TILE - 1u) / TILE};
}

struct FibTile {
    const uint8_t* p;         // the tile's tn FIBs: load_image(p, tn * FIB_BYTES, s_img, tid, TPB), then a barrier
    u32 tn, idx, base, key0;  // this lane's FIB of the tile, its byte offset in the image, the key of its entry 0
    long long fib;            // of the call
    bool live;                // it exists
};
__device__ __forceinline__ FibTile fib_tile(const FibLanes& L, const FibPass& P, u32 tile, u32 G, const uint8_t* fibs) {
    const u32 t0 = tile * TILE, tn = P.total - t0 < TILE ? P.total - t0 : TILE, idx = L.small ? L.wave * G + L.lane : L.tid;
    const uint8_t* p = fibs + (u64)(P.f0 + t0) * FIB_BYTES;
    return {p, tn, idx, (u32)(reinterpret_cast<uintptr_t>(p) & 15u) + FIB_BYTES * idx, idx * KEY_STRIDE + 1u, P.f0 + t0 + idx,
            (!L.small || L.lane < G) && idx < tn};
}
// is the lane's FIB to be walked (fib_ok is optional); called behind the tile's barrier (profiles/HISTORY.md, round 28)
__device__ __forceinline__ bool fib_in_use(const FibTile& T, const uint8_t* fib_ok) { return T.live && (!fib_ok || fib_ok[T.fib] != 0); }

// a walked FIB into its group's counts in LDS; the status byte of the lane's FIB, walked (st) or not (0)
__device__ __forceinline__ void fib_count(u32 st, u32 nnext, u32* used, u32* malf, u32* next) {
    atomicAdd(used, 1u);
    if (st & ST_MALFORMED) atomicAdd(malf, 1u);
    if (nnext) atomicAdd(next, nnext);
}
__device__ __forceinline__ void fib_status(const FibTile& T, u32 st, uint8_t* status) { if (T.live && status) status[T.fib] = (uint8_t)st; }

// One used FIB, b[0 ... 29]: fig(type, p, len) for every FIG in the order of their byte offsets, its header at b[p] and its
// len bytes behind it; what it returns is or-ed into the status byte, which fib_walk returns.  The end marker ends the
// walk, and so does a FIG that runs past byte 30, with ST_MALFORMED: fig never sees a byte outside b[0 ... 29].
template <class Fig>
__host__ __device__ __forceinline__ u32 fib_walk(const uint8_t* b, Fig&& fig) {
    u32 st = ST_USED, p = 0;
    while (p < FIB_DATA) {
        const u32 h = b[p];
        if (h == END_MARKER) break;
        const u32 type = h >> FIG_TYPE_SHIFT, len = h & FIG_LEN_MASK;
        if (p + 1u + len > FIB_DATA) return st | ST_MALFORMED;
        st |= fig(type, p, len);
        p += 1u + len;
    }
    return st;
}

// a big-endian identifier of 2 or 4 bytes
__host__ __device__ __forceinline__ u32 fig_id(const uint8_t* b, u32 idlen) {
    const u32 id = (u32)b[0] << 8 | b[1];
    return idlen == 4u ? id << 16 | (u32)b[2] << 8 | b[3] : id;
}

// The service list of a FIG 0/2, b[q ... e-1], with 32-bit SIds if pd: svc(sid, count byte) for every service, then
// comp(sid, c0, c1) for each of its components.  Returns 0, or ST_MALFORMED where one did not fit: the list ends there.
template <class Svc, class Comp>
__host__ __device__ __forceinline__ u32 fig02_services(const uint8_t* b, u32 q, u32 e, u32 pd, Svc&& svc, Comp&& comp) {
    const u32 sidlen = pd ? 4u : 2u;
    while (q < e) {
        if (e - q < sidlen + 1u) return ST_MALFORMED;
        const u32 sid = fig_id(b + q, sidlen), count = b[q + sidlen], nc = count & FIG02_NCOMP_MASK;
        svc(sid, count);
        q += sidlen + 1u;
        for (u32 c = 0; c < nc; c++) {
            if (e - q < 2u) return ST_MALFORMED;
            comp(sid, (u32)b[q], (u32)b[q + 1u]);
            q += 2u;
        }
    }
    return 0u;
}

inline long long fib_ngroups(long long nfibs, u32 G) { return (nfibs + G - 1) / G; }

// The FIBs of group g for a host twin: st = walk(b, n_next) for every used one (the unit's walk with its entry sink
// bound), the status bytes, and the group's counts.
struct FibCounts { u32 used, malf, next; };
template <class Walk>
FibCounts fib_group_host(const uint8_t* h_fibs, const uint8_t* h_fib_ok, int64_t nfibs, u32 G, int64_t g, uint8_t* h_status, Walk&& walk) {
    const int64_t f0 = g * G, fe = f0 + G < nfibs ? f0 + G : nfibs;
    FibCounts n = {};
    for (int64_t f = f0; f < fe; f++) {
        u32 st = 0;
        if (!h_fib_ok || h_fib_ok[f]) {
            st = walk(h_fibs + FIB_BYTES * (u64)f, n.next);
            n.used++;
            if (st & ST_MALFORMED) n.malf++;
        }
        if (h_status) h_status[f] = (uint8_t)st;
    }
    return n;
}

// the grid of a launch over ngroups groups: a workgroup per pass up to MAX_GRID, which then stride
inline dim3 fib_grid(long long ngroups, u32 G) {
    const long long npasses = fib_npasses(ngroups, G);
    return dim3((unsigned)(npasses < (long long)MAX_GRID ? npasses : (long long)MAX_GRID));
}

}  // namespace
