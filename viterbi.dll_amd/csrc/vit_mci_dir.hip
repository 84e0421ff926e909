// vit_mci_dir.hip -- the service directory from the FIBs on the device: FIG 0/2 (services and their packet-mode
// components), FIG 0/3 (where a packet-mode component lies) and the labels of FIG 1/0, 1/1 and 1/5 of every group of G
// FIBs, resolved to up to 64 service records, up to 64 packet component records and one group record
// (vit_mci_dir_kernel), and its host twin (vit_mci_dir_host_impl) over the same walk.  The definition is written out in
// include/viterbi_amd.h ("Service directory"); every constant of the format is in vit_fig_fmt.h.
//
// Shape: passes, tiles, a lane per FIB, the FIB's row in LDS and the walk over its FIGs are written out in
// vit_fib_group_dev.h and shared with vit_mci_kernel (vit_mci.hip).  Here a lane leaves at most 13 entries (dir_walk); a
// label entry carries the offset of its 18 bytes in the lane's row, not a copy.
//
// Which keys get records.  The records are keyed by SId (32 bits) and SCId (12 bits), so a group first agrees on its 64
// smallest keys of each table: rounds between barriers, in round r every entry whose key lies above the key chosen in
// round r-1 joins an LDS atomic minimum on cell r of the group's key array - a 64-bit minimum, whose idle value 2^64-1 is
// no key, SId 0xFFFFFFFF included.  The loop ends at a test every lane of the workgroup evaluates alike (no group of the
// pass chose a key in this round), after 64 rounds at the latest; an entry left above the 64th key sets the overflow flag.
// The array then holds the chosen keys in ascending order and an entry finds its record by binary search.  Minimum, the
// order of the rounds and the search depend on no scheduling.
// Groups of several tiles: TWO SWEEPS.  The first walks every tile and only chooses, the array's keys re-entering each
// tile's rounds as candidates (a key that falls out of the 64 smallest never comes back, so nothing the definition keeps
// is lost); the second walks the tiles again, from the last to the first, and resolves.  So a record's index is final
// before anything is written to it and records never move; the price is the second walk, paid only above 256 FIBs a
// group - a group of one tile (a transmission frame, or twenty) is walked once and its entries stay in LDS for both.
// Carrying the set from tile to tile in one sweep would need every record shifted whenever an earlier tile brings a
// smaller key.
// Resolving is vit_mci_kernel's three rounds between barriers per tile (raise the key unless a later tile has set the
// reference; write the reference; compare and count), per record and kind.  A label's value is its 18 bytes and charset
// as five words, compared word by word in LDS.
//
// Resources (hipcc -O3, gfx950, the compiler's report in profiles/r28_fib_group_resource_usage.txt): 121 VGPRs, 69,872
// bytes of LDS (two workgroups per CU), no scratch, no VGPR spills; 15 scalars are parked in lanes of a VGPR ahead of
// the passes and fetched at a pass's head and end, none inside the loops over steps, rounds or entries.  The stores are
// vector stores of plain C++.
#include <algorithm>
#include <string.h>
#include <vector>

#include "vit_fib_group_dev.h"
#include "vit_internal.h"

namespace {

typedef unsigned long long ull;
constexpr u32 LAB_WORDS = 5;          // a label value: 16 bytes, then 1 << 31 | charset << 16 | character flag field
constexpr ull NONE = ~0ull;           // an idle cell of a key array: above every key

// an entry as two words: w1 = kind | record index << 3 (filled in once the keys are chosen) | rest << 10
//   E_SVC     w0 = SId, rest = P/D | count byte << 1           E_LABEL   w0 = SId, rest = offset in the FIB | charset << 5
//   E_COMP    w0 = SId, rest = SCId | P/S << 12 | CA << 13     E_LOC     w0 = loc, rest = SCId
//   E_ELABEL  w0 = EId, rest as E_LABEL
enum : u32 { E_SVC = 1, E_LABEL = 2, E_COMP = 3, E_LOC = 4, E_ELABEL = 5 };
constexpr u32 E_KIND_MASK = 7, E_IDX_SHIFT = 3, E_IDX_MASK = 127, E_REST_SHIFT = 10, E_NO_RECORD = DIR_MAX;
constexpr u32 R_SCID_MASK = 0xFFF, R_PS_SHIFT = 12, R_CA_SHIFT = 13, R_OFF_MASK = 31, R_CHARSET_SHIFT = 5, R_COUNT_SHIFT = 1;
constexpr u32 SEEN = 1u << 31;        // of every reference word

// The walk of one used FIB, b[0 ... 29]: emit(kind, w0, rest) for every entry in the order of their byte offsets; n_next
// counts the FIGs passed over for C/N, OE or bit 3 of a label FIG; returns the status byte.
template <class Emit>
__host__ __device__ __forceinline__ u32 dir_walk(const uint8_t* b, u32& n_next, Emit&& emit) {
    return fib_walk(b, [&](u32 type, u32 p, u32 len) -> u32 {
        if (type > 1u || len < 1u) return 0u;
        const u32 t = b[p + 1u], e = p + 1u + len;
        u32 q = p + 2u, st = 0;
        if (type == 1u) {
            const u32 ext = t & FIG1_EXT_MASK;
            if (ext == EXT_LABEL_ENS || ext == EXT_LABEL_SVC16 || ext == EXT_LABEL_SVC32) {
                const u32 idlen = ext == EXT_LABEL_SVC32 ? 4u : 2u;
                if (t & FIG1_OE) {
                    n_next++;
                } else {
                    st |= ST_DIR_FIG1;
                    if (len < 1u + idlen + LABEL_VALUE_BYTES)
                        st |= ST_MALFORMED;
                    else
                        emit(ext == EXT_LABEL_ENS ? E_ELABEL : E_LABEL, fig_id(b + q, idlen),
                             (q + idlen) | (t >> FIG1_CHARSET_SHIFT) << R_CHARSET_SHIFT);
                }
            }
        } else if ((t & FIG0_EXT_MASK) == EXT_SERVICE || (t & FIG0_EXT_MASK) == EXT_PACKET) {
            if (t & (FIG0_CN | FIG0_OE)) {
                n_next++;
            } else if ((t & FIG0_EXT_MASK) == EXT_SERVICE) {  // an entry per service, and its components with TMId 3, keyed by SCId
                const u32 pd = (t & FIG0_PD) ? 1u : 0u;
                st |= ST_DIR_FIG02 | fig02_services(
                    b, q, e, pd, [&](u32 sid, u32 count) { emit(E_SVC, sid, pd | count << R_COUNT_SHIFT); },
                    [&](u32 sid, u32 c0, u32 c1) {
                        if ((c0 >> 6) == TMID_PACKET)
                            emit(E_COMP, sid, ((c0 & 63u) << 6 | c1 >> 2) | ((c1 >> 1) & 1u) << R_PS_SHIFT | (c1 & 1u) << R_CA_SHIFT);
                    });
            } else {
                st |= ST_DIR_FIG03;
                while (q < e) {
                    if (e - q < LOC_BYTES) {
                        st |= ST_MALFORMED;
                        break;
                    }
                    const u32 b1 = b[q + 1u], b2 = b[q + 2u], b3 = b[q + 3u], caorg = b1 & 1u;
                    if (caorg && e - q < LOC_BYTES + LOC_CAORG_BYTES) {
                        st |= ST_MALFORMED;
                        break;
                    }
                    emit(E_LOC, (b3 >> 2) | ((b3 & 3u) << 8 | b[q + 4u]) << LOC_ADDR_SHIFT | (b2 & 63u) << LOC_DSCTY_SHIFT |
                                    (b2 >> 7) << LOC_DG_SHIFT | caorg << LOC_CAORG_SHIFT, (u32)b[q] << 4 | b1 >> 4);
                    q += LOC_BYTES + (caorg ? LOC_CAORG_BYTES : 0u);
                }
            }
        }
        return st;
    });
}

// word k of the label value whose 18 bytes lie at r[0 ... 17]
__host__ __device__ __forceinline__ u32 label_word(const uint8_t* r, u32 k, u32 charset) {
    if (k < 4u) return (u32)r[4u * k] | (u32)r[4u * k + 1u] << 8 | (u32)r[4u * k + 2u] << 16 | (u32)r[4u * k + 3u] << 24;
    return SEEN | charset << 16 | (u32)r[LABEL_BYTES] << 8 | r[LABEL_BYTES + 1u];
}

// the position of k in the ascending key array a[0 ... 63] (idle cells behind the keys), E_NO_RECORD if it is not there
__device__ __forceinline__ u32 find_key(const ull* a, ull k) {
    u32 pos = 0;
#pragma unroll
    for (u32 s = DIR_MAX / 2u; s > 0u; s >>= 1)
        if (a[pos + s - 1u] < k) pos += s;
    return a[pos] == k ? pos : E_NO_RECORD;
}

__global__ __launch_bounds__(TPB) void vit_mci_dir_kernel(const uint8_t* __restrict__ fibs, const uint8_t* __restrict__ fib_ok,
                                                          long long nfibs, u32 G, long long ngroups, u32* __restrict__ svc,
                                                          u32* __restrict__ pkt, u32* __restrict__ dir, uint8_t* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) uint8_t s_img[IMG_BYTES];
    __shared__ u32 s_row[TPB * ROW_DWORDS];
    __shared__ u32 s_e0[DIR_MAX_ENTRIES][TPB], s_e1[DIR_MAX_ENTRIES][TPB];
    // per group of the pass: the chosen keys in ascending order; per record the keys of the tile, the references, the counts
    __shared__ ull s_sk[SLOTS][DIR_MAX], s_ck[SLOTS][DIR_MAX];
    __shared__ u32 s_vkey[SLOTS][DIR_MAX], s_lkey[SLOTS][DIR_MAX], s_pkey[SLOTS][DIR_MAX], s_okey[SLOTS][DIR_MAX];
    __shared__ u32 s_sval[SLOTS][DIR_MAX], s_lab[SLOTS][LAB_WORDS][DIR_MAX];              // SEEN | P/D | count byte << 1; label
    __shared__ u32 s_cfl[SLOTS][DIR_MAX], s_csid[SLOTS][DIR_MAX], s_loc[SLOTS][DIR_MAX];  // SEEN | P/S | CA << 1; SId; SEEN | loc
    __shared__ u32 s_nv[SLOTS][DIR_MAX], s_nv_o[SLOTS][DIR_MAX], s_nl[SLOTS][DIR_MAX], s_nl_o[SLOTS][DIR_MAX];
    __shared__ u32 s_np[SLOTS][DIR_MAX], s_np_o[SLOTS][DIR_MAX], s_no[SLOTS][DIR_MAX], s_no_o[SLOTS][DIR_MAX];
    // per group: FIG 1/0 (s_eid = SEEN | EId once one is seen), overflow flags and the FIB counts
    __shared__ u32 s_ekey[SLOTS], s_eid[SLOTS], s_elab[SLOTS][LAB_WORDS], s_ne[SLOTS], s_ne_o[SLOTS];
    __shared__ u32 s_ovf[SLOTS], s_used[SLOTS], s_malf[SLOTS], s_next[SLOTS];

    const FibLanes L = fib_lanes(G, ngroups);
    const u32 tid = L.tid, slot = L.slot, gpp = L.gpp, os = L.wave, oc = L.lane;  // (os, oc): the group of the pass and the record to write out
    u32* row = s_row + ROW_DWORDS * tid;
    const uint8_t* row8 = reinterpret_cast<const uint8_t*>(row);
    // every lane of a workgroup makes the same passes, steps and rounds: the barriers are uniform
    for (long long pass = blockIdx.x; pass < L.npasses; pass += gridDim.x) {
        s_sk[os][oc] = s_ck[os][oc] = NONE;
        s_vkey[os][oc] = s_lkey[os][oc] = s_pkey[os][oc] = s_okey[os][oc] = 0;
        s_sval[os][oc] = s_cfl[os][oc] = s_csid[os][oc] = s_loc[os][oc] = 0;
#pragma unroll
        for (u32 k = 0; k < LAB_WORDS; k++) s_lab[os][k][oc] = 0;
        s_nv[os][oc] = s_nv_o[os][oc] = s_nl[os][oc] = s_nl_o[os][oc] = 0;
        s_np[os][oc] = s_np_o[os][oc] = s_no[os][oc] = s_no_o[os][oc] = 0;
        if (oc == 0) s_ekey[os] = s_eid[os] = s_ne[os] = s_ne_o[os] = s_ovf[os] = s_used[os] = s_malf[os] = s_next[os] = 0;
        if (oc < LAB_WORDS) s_elab[os][oc] = 0;
        const FibPass P = fib_pass(L, pass, G, nfibs);
        // one tile: a single step that chooses and resolves; more: a sweep that chooses, then one that resolves, backwards
        const u32 ntiles = P.ntiles, nsteps = ntiles == 1u ? 1u : 2u * ntiles;
        for (u32 step = 0; step < nsteps; step++) {
            const bool choose = step < ntiles, resolve = step + ntiles >= nsteps;
            const FibTile T = fib_tile(L, P, choose ? step : nsteps - 1u - step, G, fibs);
            load_image(T.p, T.tn * FIB_BYTES, s_img, tid, TPB);
            __syncthreads();  // (also: the cleared records, and the previous step's last round)
            u32 cnt = 0, st = 0, nnext = 0;
            if (fib_in_use(T, fib_ok)) {
                image_row<ROW_DWORDS>(s_img, T.base, row);
                st = dir_walk(row8, nnext, [&](u32 kind, u32 w0, u32 rest) {
                    if (cnt < DIR_MAX_ENTRIES) {
                        s_e0[cnt][tid] = w0;
                        s_e1[cnt][tid] = kind | rest << E_REST_SHIFT;
                        cnt++;
                    }
                });
                if (resolve) fib_count(st, nnext, &s_used[slot], &s_malf[slot], &s_next[slot]);
            }
            if (resolve) fib_status(T, st, status);
            if (choose) {
                // the keys chosen so far re-enter as candidates, a lane per key; the array starts idle again
                const ull old_s = s_sk[os][oc], old_c = s_ck[os][oc];
                s_sk[os][oc] = s_ck[os][oc] = NONE;
                __syncthreads();
                ull lo_s = 0, lo_c = 0;  // keys from here on are still to be chosen
                bool more = cnt > 0u;
                u32 r = 0;
                for (; r < DIR_MAX; r++) {
                    if (more) {
                        more = false;
                        for (u32 j = 0; j < cnt; j++) {
                            const u32 w1 = s_e1[j][tid], kind = w1 & E_KIND_MASK;
                            if (kind == E_SVC || kind == E_LABEL) {
                                const ull k = s_e0[j][tid];
                                if (k >= lo_s) {
                                    atomicMin(&s_sk[slot][r], k);
                                    more = true;
                                }
                            } else if (kind == E_COMP || kind == E_LOC) {
                                const ull k = (w1 >> E_REST_SHIFT) & R_SCID_MASK;
                                if (k >= lo_c) {
                                    atomicMin(&s_ck[slot][r], k);
                                    more = true;
                                }
                            }
                        }
                    }
                    if (os < gpp) {  // (then os is this lane's slot as well)
                        if (old_s != NONE && old_s >= lo_s) atomicMin(&s_sk[os][r], old_s);
                        if (old_c != NONE && old_c >= lo_c) atomicMin(&s_ck[os][r], old_c);
                    }
                    __syncthreads();
                    ull all = NONE;  // (the cells of a slot that holds no group stay idle)
#pragma unroll
                    for (u32 s = 0; s < SLOTS; s++) all &= s_sk[s][r] & s_ck[s][r];
                    if (all == NONE) break;
                    const ull ms = s_sk[slot][r], mc = s_ck[slot][r];
                    lo_s = ms == NONE ? NONE : ms + 1u;
                    lo_c = mc == NONE ? NONE : mc + 1u;
                }
                if (r == DIR_MAX) {  // 64 rounds chose keys: whatever lies above the 64th leaves only the flag
                    u32 ovf = 0;
                    for (u32 j = 0; j < cnt; j++) {
                        const u32 w1 = s_e1[j][tid], kind = w1 & E_KIND_MASK;
                        if ((kind == E_SVC || kind == E_LABEL) && (ull)s_e0[j][tid] >= lo_s) ovf |= DIR_SVC_OVERFLOW;
                        if ((kind == E_COMP || kind == E_LOC) && (ull)((w1 >> E_REST_SHIFT) & R_SCID_MASK) >= lo_c) ovf |= DIR_PKT_OVERFLOW;
                    }
                    if (os < gpp && old_s != NONE && old_s >= lo_s) ovf |= DIR_SVC_OVERFLOW;
                    if (os < gpp && old_c != NONE && old_c >= lo_c) ovf |= DIR_PKT_OVERFLOW;
                    if (ovf) atomicOr(&s_ovf[slot], ovf);
                }
            }
            if (resolve) {
                // every entry finds its record; round 1: the last entry of the tile for every record and kind that has no
                // reference yet
                const u32 key0 = T.key0;
                for (u32 j = 0; j < cnt; j++) {
                    const u32 w0 = s_e0[j][tid], w1 = s_e1[j][tid], kind = w1 & E_KIND_MASK;
                    u32 i = 0;
                    if (kind == E_SVC || kind == E_LABEL) i = find_key(s_sk[slot], (ull)w0);
                    else if (kind == E_COMP || kind == E_LOC) i = find_key(s_ck[slot], (ull)((w1 >> E_REST_SHIFT) & R_SCID_MASK));
                    s_e1[j][tid] = w1 | i << E_IDX_SHIFT;
                    if (i == E_NO_RECORD) continue;
                    if (kind == E_SVC) {
                        if (!(s_sval[slot][i] & SEEN)) atomicMax(&s_vkey[slot][i], key0 + j);
                    } else if (kind == E_LABEL) {
                        if (!(s_lab[slot][LAB_WORDS - 1u][i] & SEEN)) atomicMax(&s_lkey[slot][i], key0 + j);
                    } else if (kind == E_COMP) {
                        if (!(s_cfl[slot][i] & SEEN)) atomicMax(&s_pkey[slot][i], key0 + j);
                    } else if (kind == E_LOC) {
                        if (!(s_loc[slot][i] & SEEN)) atomicMax(&s_okey[slot][i], key0 + j);
                    } else {
                        if (!(s_eid[slot] & SEEN)) atomicMax(&s_ekey[slot], key0 + j);
                    }
                }
                __syncthreads();
                // round 2: it becomes the reference (a key that was not raised is 0: no entry's)
                for (u32 j = 0; j < cnt; j++) {
                    const u32 w0 = s_e0[j][tid], w1 = s_e1[j][tid], kind = w1 & E_KIND_MASK, i = (w1 >> E_IDX_SHIFT) & E_IDX_MASK;
                    const u32 rest = w1 >> E_REST_SHIFT;
                    if (i == E_NO_RECORD) continue;
                    if (kind == E_SVC) {
                        if (s_vkey[slot][i] == key0 + j) s_sval[slot][i] = SEEN | rest;
                    } else if (kind == E_LABEL) {
                        if (s_lkey[slot][i] == key0 + j)
                            for (u32 k = 0; k < LAB_WORDS; k++)
                                s_lab[slot][k][i] = label_word(row8 + (rest & R_OFF_MASK), k, rest >> R_CHARSET_SHIFT);
                    } else if (kind == E_COMP) {
                        if (s_pkey[slot][i] == key0 + j) {
                            s_cfl[slot][i] = SEEN | rest >> R_PS_SHIFT;
                            s_csid[slot][i] = w0;
                        }
                    } else if (kind == E_LOC) {
                        if (s_okey[slot][i] == key0 + j) s_loc[slot][i] = SEEN | w0;
                    } else if (s_ekey[slot] == key0 + j) {
                        s_eid[slot] = SEEN | w0;
                        for (u32 k = 0; k < LAB_WORDS; k++)
                            s_elab[slot][k] = label_word(row8 + (rest & R_OFF_MASK), k, rest >> R_CHARSET_SHIFT);
                    }
                }
                __syncthreads();
                // round 3: every entry against the reference; the keys are cleared for the next tile
                for (u32 j = 0; j < cnt; j++) {
                    const u32 w0 = s_e0[j][tid], w1 = s_e1[j][tid], kind = w1 & E_KIND_MASK, i = (w1 >> E_IDX_SHIFT) & E_IDX_MASK;
                    const u32 rest = w1 >> E_REST_SHIFT;
                    if (i == E_NO_RECORD) continue;
                    if (kind == E_SVC) {
                        atomicAdd((SEEN | rest) == s_sval[slot][i] ? &s_nv[slot][i] : &s_nv_o[slot][i], 1u);
                    } else if (kind == E_LABEL) {
                        bool eq = true;
                        for (u32 k = 0; k < LAB_WORDS; k++)
                            eq = eq && s_lab[slot][k][i] == label_word(row8 + (rest & R_OFF_MASK), k, rest >> R_CHARSET_SHIFT);
                        atomicAdd(eq ? &s_nl[slot][i] : &s_nl_o[slot][i], 1u);
                    } else if (kind == E_COMP) {
                        const bool eq = (SEEN | rest >> R_PS_SHIFT) == s_cfl[slot][i] && w0 == s_csid[slot][i];
                        atomicAdd(eq ? &s_np[slot][i] : &s_np_o[slot][i], 1u);
                    } else if (kind == E_LOC) {
                        atomicAdd((SEEN | w0) == s_loc[slot][i] ? &s_no[slot][i] : &s_no_o[slot][i], 1u);
                    } else {
                        bool eq = (SEEN | w0) == s_eid[slot];
                        for (u32 k = 0; k < LAB_WORDS; k++)
                            eq = eq && s_elab[slot][k] == label_word(row8 + (rest & R_OFF_MASK), k, rest >> R_CHARSET_SHIFT);
                        atomicAdd(eq ? &s_ne[slot] : &s_ne_o[slot], 1u);
                    }
                }
                s_vkey[os][oc] = s_lkey[os][oc] = s_pkey[os][oc] = s_okey[os][oc] = 0;
                if (oc == 0) s_ekey[os] = 0;
            }
            __syncthreads();
        }
        const long long g = P.g0 + os;
        if (os < gpp && g < ngroups) {  // (whole wavefronts: os is the wavefront)
            const ull ks = s_sk[os][oc], kc = s_ck[os][oc];
            const u32 nsvc = (u32)__popcll(__ballot(ks != NONE)), npkt = (u32)__popcll(__ballot(kc != NONE));
            u32* o = svc + 8u * ((u64)g * DIR_MAX + oc);
            const u32 sval = s_sval[os][oc], l4 = s_lab[os][LAB_WORDS - 1u][oc];
            const u32 sflags = ((l4 & SEEN) ? SVC_LABEL | ((l4 >> 16) & 15u) << SVC_CHARSET_SHIFT : 0u) |
                               ((sval & SEEN) ? SVC_LISTED | (sval & 1u) << SVC_PD_SHIFT : 0u);
            o[0] = ks != NONE ? (u32)ks : 0u;
#pragma unroll
            for (u32 k = 0; k < 4u; k++) o[1u + k] = s_lab[os][k][oc];
            o[5] = (l4 & 0xFFFFu) | sflags << 16 | ((sval >> R_COUNT_SHIFT) & 255u) << 24;
            o[6] = (s_nl[os][oc] & 0xFFFFu) | s_nl_o[os][oc] << 16;
            o[7] = (s_nv[os][oc] & 0xFFFFu) | s_nv_o[os][oc] << 16;
            u32* c = pkt + 5u * ((u64)g * DIR_MAX + oc);
            const u32 loc = s_loc[os][oc], cfl = s_cfl[os][oc];
            const u32 pflags = ((loc & SEEN) ? PKT_LOC : 0u) | ((cfl & SEEN) ? PKT_COMP | (cfl & 3u) << PKT_PS_SHIFT : 0u);
            c[0] = (kc != NONE ? (u32)kc : 0u) | pflags << 16;
            c[1] = loc & ~SEEN;
            c[2] = s_csid[os][oc];
            c[3] = (s_no[os][oc] & 0xFFFFu) | s_no_o[os][oc] << 16;
            c[4] = (s_np[os][oc] & 0xFFFFu) | s_np_o[os][oc] << 16;
            if (oc < 10u) {
                const u32 eid = s_eid[os], e4 = s_elab[os][LAB_WORDS - 1u];
                const u32 dflags = ((eid & SEEN) ? DIR_LABEL : 0u) | s_ovf[os];
                const u32 v = oc == 0u   ? (eid & 0xFFFFu) | (e4 & 0xFFFFu) << 16
                              : oc <= 4u ? s_elab[os][oc - 1u]
                              : oc == 5u ? dflags | ((e4 >> 16) & 15u) << 8 | s_ne[os] << 16
                              : oc == 6u ? (s_ne_o[os] & 0xFFFFu) | nsvc << 16
                              : oc == 7u ? npkt | s_used[os] << 16
                              : oc == 8u ? (s_malf[os] & 0xFFFFu) | s_next[os] << 16
                                         : 0u;
                dir[10u * (u64)g + oc] = v;
            }
        }
        // (the next pass clears what this lane's wavefront has just read, and nothing else, before its first barrier)
    }
}

struct HostEntry {
    u32 kind, w0, rest;
    uint8_t lab[LABEL_VALUE_BYTES];
};

inline u32 ent_scid(const HostEntry& e) { return e.rest & R_SCID_MASK; }

// the first 64 of the distinct keys in ascending order; true if there were more
bool first_keys(std::vector<u32>& keys) {
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    const bool over = keys.size() > DIR_MAX;
    if (over) keys.resize(DIR_MAX);
    return over;
}

inline int key_index(const std::vector<u32>& keys, u32 k) {
    const auto it = std::lower_bound(keys.begin(), keys.end(), k);
    return it != keys.end() && *it == k ? (int)(it - keys.begin()) : -1;
}

}  // namespace

void vit_mci_dir_host_impl(const uint8_t* h_fibs, const uint8_t* h_fib_ok, int64_t nfibs, uint32_t G, vit_mci_service* h_svc,
                           vit_mci_pktcomp* h_pkt, vit_mci_dir* h_dir, uint8_t* h_status) {
    const int64_t ngroups = fib_ngroups(nfibs, G);
    std::vector<HostEntry> ent;
    std::vector<u32> sids, scids;
    for (int64_t g = 0; g < ngroups; g++) {
        ent.clear();
        sids.clear();
        scids.clear();
        const FibCounts n = fib_group_host(h_fibs, h_fib_ok, nfibs, G, g, h_status, [&](const uint8_t* b, u32& next) {
            return dir_walk(b, next, [&](u32 kind, u32 w0, u32 rest) {
                HostEntry e = {kind, w0, rest, {}};
                if (kind == E_LABEL || kind == E_ELABEL) memcpy(e.lab, b + (rest & R_OFF_MASK), LABEL_VALUE_BYTES);
                if (kind == E_SVC || kind == E_LABEL) sids.push_back(w0);
                if (kind == E_COMP || kind == E_LOC) scids.push_back(ent_scid(e));
                ent.push_back(e);
            });
        });
        vit_mci_service* S = h_svc + DIR_MAX * (u64)g;
        vit_mci_pktcomp* P = h_pkt + DIR_MAX * (u64)g;
        memset(S, 0, DIR_MAX * sizeof(*S));
        memset(P, 0, DIR_MAX * sizeof(*P));
        vit_mci_dir D;
        memset(&D, 0, sizeof(D));
        if (first_keys(sids)) D.flags |= DIR_SVC_OVERFLOW;
        if (first_keys(scids)) D.flags |= DIR_PKT_OVERFLOW;
        for (size_t i = 0; i < sids.size(); i++) S[i].sid = sids[i];
        for (size_t i = 0; i < scids.size(); i++) P[i].scid = (uint16_t)scids[i];
        u32 svc_pd[DIR_MAX] = {}, comp_rest[DIR_MAX] = {}, ens_charset = 0;
        for (size_t k = ent.size(); k-- > 0;) {  // from the last entry back: the first one met is the one that wins
            const HostEntry& e = ent[k];
            const u32 charset = e.rest >> R_CHARSET_SHIFT;
            const uint16_t chars = (uint16_t)(e.lab[LABEL_BYTES] << 8 | e.lab[LABEL_BYTES + 1u]);
            if (e.kind == E_SVC || e.kind == E_LABEL) {
                const int i = key_index(sids, e.w0);
                if (i < 0) continue;
                vit_mci_service& s = S[i];
                if (e.kind == E_SVC) {
                    const u32 pd = e.rest & 1u, count = (e.rest >> R_COUNT_SHIFT) & 255u;
                    if (!(s.flags & SVC_LISTED)) {
                        s.flags |= (uint8_t)(SVC_LISTED | pd << SVC_PD_SHIFT);
                        s.count = (uint8_t)count;
                        svc_pd[i] = pd;
                    }
                    if (svc_pd[i] == pd && s.count == count) s.n_listed++;
                    else s.n_listed_other++;
                } else {
                    if (!(s.flags & SVC_LABEL)) {
                        s.flags |= (uint8_t)(SVC_LABEL | charset << SVC_CHARSET_SHIFT);
                        memcpy(s.label, e.lab, LABEL_BYTES);
                        s.chars = chars;
                    }
                    if (!memcmp(s.label, e.lab, LABEL_BYTES) && s.chars == chars && (u32)(s.flags >> SVC_CHARSET_SHIFT) == charset) s.n_label++;
                    else s.n_label_other++;
                }
            } else if (e.kind == E_COMP || e.kind == E_LOC) {
                const int i = key_index(scids, ent_scid(e));
                if (i < 0) continue;
                vit_mci_pktcomp& c = P[i];
                if (e.kind == E_COMP) {
                    const u32 psca = e.rest >> R_PS_SHIFT;
                    if (!(c.flags & PKT_COMP)) {
                        c.flags |= (uint16_t)(PKT_COMP | psca << PKT_PS_SHIFT);
                        c.sid = e.w0;
                        comp_rest[i] = psca;
                    }
                    if (comp_rest[i] == psca && c.sid == e.w0) c.n_comp++;
                    else c.n_comp_other++;
                } else {
                    if (!(c.flags & PKT_LOC)) {
                        c.flags |= PKT_LOC;
                        c.loc = e.w0;
                    }
                    if (c.loc == e.w0) c.n_loc++;
                    else c.n_loc_other++;
                }
            } else {
                if (!(D.flags & DIR_LABEL)) {
                    D.flags |= DIR_LABEL;
                    D.eid = (uint16_t)e.w0;
                    D.chars = chars;
                    D.charset = (uint8_t)charset;
                    ens_charset = charset;
                    memcpy(D.label, e.lab, LABEL_BYTES);
                }
                if (D.eid == e.w0 && !memcmp(D.label, e.lab, LABEL_BYTES) && D.chars == chars && ens_charset == charset) D.n_label++;
                else D.n_label_other++;
            }
        }
        D.nsvc = (uint16_t)sids.size();
        D.npkt = (uint16_t)scids.size();
        D.nfib_used = (uint16_t)n.used;
        D.nfib_malformed = (uint16_t)n.malf;
        D.n_next = (uint16_t)n.next;
        h_dir[g] = D;
    }
}

hipError_t vit_launch_mci_dir(const uint8_t* d_fibs, const uint8_t* d_fib_ok, int64_t nfibs, uint32_t G, vit_mci_service* d_svc,
                              vit_mci_pktcomp* d_pkt, vit_mci_dir* d_dir, uint8_t* d_status, hipStream_t stream) {
    if (nfibs <= 0) return hipSuccess;
    const long long ngroups = fib_ngroups(nfibs, G);
    hipLaunchKernelGGL(vit_mci_dir_kernel, fib_grid(ngroups, G), dim3(TPB), 0, stream, d_fibs, d_fib_ok, (long long)nfibs, G,
                       ngroups, reinterpret_cast<u32*>(d_svc), reinterpret_cast<u32*>(d_pkt), reinterpret_cast<u32*>(d_dir), d_status);
    return hipGetLastError();
}
