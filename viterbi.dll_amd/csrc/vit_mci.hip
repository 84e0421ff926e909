// vit_mci.hip -- the multiplex configuration from the FIBs on the device: FIG 0/0 (ensemble), FIG 0/1 (sub-channel
// organisation) and FIG 0/2 (service components) of every group of G FIBs, resolved to 64 sub-channel records and one
// group record (vit_mci_kernel), and its host twin (vit_mci_fibs_host_impl) over the same walk.  The definition is written
// out in include/viterbi_amd.h ("Multiplex configuration"); every constant of the format is in vit_fig_fmt.h.
//
// Shape: passes, tiles, a lane per FIB and the FIB's row in LDS are written out in vit_fib_group_dev.h, which this
// kernel shares with vit_mci_dir_kernel.  Here a lane leaves at most 12 entries (mci_walk), and last wins, without depending on scheduling:
// three rounds between barriers - every entry raises its SubChId's key with an LDS atomic maximum, the entry whose
// key came out on top writes its value as the SubChId's reference, every entry compares itself with the reference and
// adds to the equal or the other count.  Maximum and sums do not depend on the order of their operands.  A group of more
// than one tile is taken from its last tile to its first: a SubChId whose reference is set by a later tile no longer raises
// a key, and its earlier entries are only counted.  The 64 records stay in LDS across the tiles and are written once.
//
// Resources (hipcc -O3, gfx950, the compiler's report in profiles/r28_fib_group_resource_usage.txt): 81 VGPRs, 51,344
// bytes of LDS, no scratch, no spills; the LDS sets three workgroups per CU.  The stores are vector stores of plain C++.
// With G = 4096 a call of 49152 FIBs runs on 12 workgroups.
#include <vector>

#include "vit_fib_group_dev.h"
#include "vit_internal.h"

namespace {

// an entry as two words: w0 = the value (org; SId; EId << 16 | cif), w1 = SubChId | kind << 6 | rest << 8 (comp's low ten
// bits; change flags | Al << 2)
enum : u32 { E_ORG = 1, E_COMP = 2, E_ENS = 3 };
constexpr u32 E_KIND_SHIFT = 6, E_REST_SHIFT = 8;

// The walk of one used FIB, b[0 ... 29]: emit(kind, SubChId, w0, rest) for every entry in the order of their byte
// offsets; n_next counts the FIGs passed over for C/N or OE; returns the status byte.  The FIG iteration and the FIG 0/2
// list are this walk's own text of what fib_walk and fig02_services (vit_fib_group_dev.h) state for dir_walk: through them
// vit_mci_kernel ran 0.9 % (G = 12) and 1.2 % (G = 4096) slower on random FIBs, outside the timing rule
// (profiles/HISTORY.md, round 28).  A change to the end marker, the overrun rule or the list's two exits goes into both.
template <class Emit>
__host__ __device__ __forceinline__ u32 mci_walk(const uint8_t* b, u32& n_next, Emit&& emit) {
    u32 st = ST_USED, p = 0;
    while (p < FIB_DATA) {
        const u32 h = b[p];
        if (h == END_MARKER) break;
        const u32 type = h >> FIG_TYPE_SHIFT, len = h & FIG_LEN_MASK;
        if (p + 1u + len > FIB_DATA) {
            st |= ST_MALFORMED;
            break;
        }
        if (type == 0 && len >= 1u) {
            const u32 t = b[p + 1u], ext = t & FIG0_EXT_MASK;
            if (ext <= EXT_SERVICE) {
                u32 q = p + 2u;
                const u32 e = p + 1u + len;
                if (t & (FIG0_CN | FIG0_OE)) {
                    n_next++;
                } else if (ext == EXT_ENSEMBLE) {
                    st |= ST_FIG00;
                    if (e - q < 4u) {
                        st |= ST_MALFORMED;
                    } else {
                        const u32 b2 = b[q + 2u];
                        emit(E_ENS, 0u, (u32)b[q] << 24 | (u32)b[q + 1u] << 16 | (b2 & 31u) << 8 | b[q + 3u],
                             b2 >> 6 | ((b2 >> 5) & 1u) << 2);
                    }
                } else if (ext == EXT_SUBCH) {
                    st |= ST_FIG01;
                    while (q < e) {
                        if (e - q < 3u) {
                            st |= ST_MALFORMED;
                            break;
                        }
                        const u32 b0 = b[q], b2 = b[q + 2u];
                        const u32 start = (b0 & 3u) << 8 | b[q + 1u];
                        if (!(b2 >> 7)) {
                            emit(E_ORG, b0 >> 2, ORG_PRESENT | start | (b2 & ORG_INDEX_MASK) << ORG_INDEX_SHIFT |
                                                     ((b2 >> 6) & 1u) << ORG_SWITCH_SHIFT, 0u);
                            q += 3u;
                        } else {
                            if (e - q < 4u) {
                                st |= ST_MALFORMED;
                                break;
                            }
                            emit(E_ORG, b0 >> 2, ORG_PRESENT | ORG_LONG | start | ((b2 & 3u) << 8 | b[q + 3u]) << ORG_SIZE_SHIFT |
                                                     ((b2 >> 2) & ORG_LEVEL_MASK) << ORG_LEVEL_SHIFT |
                                                     ((b2 >> 4) & ORG_OPTION_MASK) << ORG_OPTION_SHIFT, 0u);
                            q += 4u;
                        }
                    }
                } else {
                    st |= ST_FIG02;
                    const u32 sidlen = (t & FIG0_PD) ? 4u : 2u;
                    bool fits = true;
                    while (fits && q < e) {
                        if (e - q < sidlen + 1u) {
                            st |= ST_MALFORMED;
                            break;
                        }
                        u32 sid = (u32)b[q] << 8 | b[q + 1u];
                        if (sidlen == 4u) sid = sid << 16 | (u32)b[q + 2u] << 8 | b[q + 3u];
                        const u32 nc = b[q + sidlen] & 15u;
                        q += sidlen + 1u;
                        for (u32 c = 0; c < nc; c++) {
                            if (e - q < 2u) {
                                st |= ST_MALFORMED;
                                fits = false;
                                break;
                            }
                            const u32 c0 = b[q], c1 = b[q + 1u], tmid = c0 >> 6;
                            if (tmid <= 1u)
                                emit(E_COMP, c1 >> 2, sid, tmid | (c0 & COMP_TYPE_MASK) << COMP_TYPE_SHIFT |
                                                               ((c1 >> 1) & 1u) << COMP_PS_SHIFT | (c1 & 1u) << COMP_CA_SHIFT);
                            q += 2u;
                        }
                    }
                }
            }
        }
        p += 1u + len;
    }
    return st;
}

__global__ __launch_bounds__(TPB) void vit_mci_kernel(const uint8_t* __restrict__ fibs, const uint8_t* __restrict__ fib_ok,
                                                      long long nfibs, u32 G, long long ngroups, u32* __restrict__ sub,
                                                      u32* __restrict__ grp, uint8_t* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) uint8_t s_img[IMG_BYTES];
    __shared__ u32 s_row[TPB * ROW_DWORDS];
    __shared__ u32 s_e0[MAX_ENTRIES][TPB], s_e1[MAX_ENTRIES][TPB];
    // per group of the pass and SubChId: the keys of the tile, the references, the counts
    __shared__ u32 s_okey[SLOTS][NSUBCH], s_ckey[SLOTS][NSUBCH];
    __shared__ u32 s_org[SLOTS][NSUBCH], s_comp[SLOTS][NSUBCH], s_sid[SLOTS][NSUBCH];
    __shared__ u32 s_norg[SLOTS][NSUBCH], s_norg_o[SLOTS][NSUBCH], s_ncomp[SLOTS][NSUBCH], s_ncomp_o[SLOTS][NSUBCH];
    // per group: FIG 0/0 (s_ens1 = 1 << 31 | change flags | Al << 2 once one is seen) and the FIB counts
    __shared__ u32 s_ekey[SLOTS], s_ens0[SLOTS], s_ens1[SLOTS], s_nens_o[SLOTS], s_used[SLOTS], s_malf[SLOTS], s_next[SLOTS];

    const FibLanes L = fib_lanes(G, ngroups);
    const u32 tid = L.tid, slot = L.slot, os = L.wave, oc = L.lane;  // (os, oc): the group of the pass and the SubChId to write out
    for (long long pass = blockIdx.x; pass < L.npasses; pass += gridDim.x) {
        s_okey[os][oc] = s_ckey[os][oc] = s_org[os][oc] = s_comp[os][oc] = s_sid[os][oc] = 0;
        s_norg[os][oc] = s_norg_o[os][oc] = s_ncomp[os][oc] = s_ncomp_o[os][oc] = 0;
        if (oc == 0) s_ekey[os] = s_ens0[os] = s_ens1[os] = s_nens_o[os] = s_used[os] = s_malf[os] = s_next[os] = 0;
        const FibPass P = fib_pass(L, pass, G, nfibs);
        for (u32 tile = P.ntiles; tile-- > 0;) {
            const FibTile T = fib_tile(L, P, tile, G, fibs);
            load_image(T.p, T.tn * FIB_BYTES, s_img, tid, TPB);
            __syncthreads();  // (also: the cleared records, and the previous tile's last round)
            u32 cnt = 0, st = 0, nnext = 0;
            if (fib_in_use(T, fib_ok)) {
                u32* row = s_row + ROW_DWORDS * tid;
                image_row<ROW_DWORDS>(s_img, T.base, row);
                st = mci_walk(reinterpret_cast<const uint8_t*>(row), nnext, [&](u32 kind, u32 c, u32 w0, u32 rest) {
                    if (cnt < MAX_ENTRIES) {
                        s_e0[cnt][tid] = w0;
                        s_e1[cnt][tid] = c | kind << E_KIND_SHIFT | rest << E_REST_SHIFT;
                        cnt++;
                    }
                });
                fib_count(st, nnext, &s_used[slot], &s_malf[slot], &s_next[slot]);
            }
            fib_status(T, st, status);
            const u32 key0 = T.key0;
            // round 1: the last entry of the tile for every SubChId that has no reference yet
            for (u32 j = 0; j < cnt; j++) {
                const u32 w1 = s_e1[j][tid], kind = (w1 >> E_KIND_SHIFT) & 3u, c = w1 & (NSUBCH - 1u);
                if (kind == E_ORG) {
                    if (!(s_org[slot][c] & ORG_PRESENT)) atomicMax(&s_okey[slot][c], key0 + j);
                } else if (kind == E_COMP) {
                    if (!(s_comp[slot][c] & COMP_PRESENT)) atomicMax(&s_ckey[slot][c], key0 + j);
                } else {
                    if (!(s_ens1[slot] >> 31)) atomicMax(&s_ekey[slot], key0 + j);
                }
            }
            __syncthreads();
            // round 2: it becomes the reference (a key that was not raised is 0: no entry's)
            for (u32 j = 0; j < cnt; j++) {
                const u32 w0 = s_e0[j][tid], w1 = s_e1[j][tid], kind = (w1 >> E_KIND_SHIFT) & 3u, c = w1 & (NSUBCH - 1u);
                const u32 rest = w1 >> E_REST_SHIFT;
                if (kind == E_ORG) {
                    if (s_okey[slot][c] == key0 + j) s_org[slot][c] = w0;
                } else if (kind == E_COMP) {
                    if (s_ckey[slot][c] == key0 + j) {
                        s_comp[slot][c] = COMP_PRESENT | rest;
                        s_sid[slot][c] = w0;
                    }
                } else if (s_ekey[slot] == key0 + j) {
                    s_ens0[slot] = w0;
                    s_ens1[slot] = 1u << 31 | rest;
                }
            }
            __syncthreads();
            // round 3: every entry against the reference; the keys are cleared for the next tile
            for (u32 j = 0; j < cnt; j++) {
                const u32 w0 = s_e0[j][tid], w1 = s_e1[j][tid], kind = (w1 >> E_KIND_SHIFT) & 3u, c = w1 & (NSUBCH - 1u);
                const u32 rest = w1 >> E_REST_SHIFT;
                if (kind == E_ORG) {
                    atomicAdd(w0 == s_org[slot][c] ? &s_norg[slot][c] : &s_norg_o[slot][c], 1u);
                } else if (kind == E_COMP) {
                    const bool eq = (COMP_PRESENT | rest) == s_comp[slot][c] && w0 == s_sid[slot][c];
                    atomicAdd(eq ? &s_ncomp[slot][c] : &s_ncomp_o[slot][c], 1u);
                } else if ((w0 >> 16) != (s_ens0[slot] >> 16) || rest != (s_ens1[slot] & 7u)) {
                    atomicAdd(&s_nens_o[slot], 1u);
                }
            }
            s_okey[os][oc] = s_ckey[os][oc] = 0;
            if (oc == 0) s_ekey[os] = 0;
            __syncthreads();
        }
        const long long g = P.g0 + os;
        if (os < L.gpp && g < ngroups) {
            u32* o = sub + 5u * ((u64)g * NSUBCH + oc);
            o[0] = s_org[os][oc];
            o[1] = s_comp[os][oc];
            o[2] = s_sid[os][oc];
            o[3] = (s_norg[os][oc] & 0xFFFFu) | s_norg_o[os][oc] << 16;
            o[4] = (s_ncomp[os][oc] & 0xFFFFu) | s_ncomp_o[os][oc] << 16;
            if (oc < 4u) {
                const u32 e0 = s_ens0[os], e1 = s_ens1[os];
                const u32 flags = (e1 >> 31) ? GRP_SEEN | (e1 & 7u) << GRP_CHANGE_SHIFT : 0u;
                const u32 v = oc == 0u   ? (e0 >> 16) | (e0 & 0xFFFFu) << 16
                              : oc == 1u ? flags | s_used[os] << 16
                              : oc == 2u ? (s_malf[os] & 0xFFFFu) | s_nens_o[os] << 16
                                         : (s_next[os] & 0xFFFFu);
                grp[4u * (u64)g + oc] = v;
            }
        }
        // (the next pass clears what this lane has just read, and nothing else, before its first barrier)
    }
}

struct HostEntry {
    u32 kind, c, w0, rest;
};

}  // namespace

void vit_mci_fibs_host_impl(const uint8_t* h_fibs, const uint8_t* h_fib_ok, int64_t nfibs, uint32_t G, vit_mci_subch* h_sub,
                            vit_mci_group* h_grp, uint8_t* h_status) {
    const int64_t ngroups = fib_ngroups(nfibs, G);
    std::vector<HostEntry> ent;
    for (int64_t g = 0; g < ngroups; g++) {
        ent.clear();
        const FibCounts n = fib_group_host(h_fibs, h_fib_ok, nfibs, G, g, h_status, [&](const uint8_t* b, u32& next) {
            return mci_walk(b, next, [&](u32 kind, u32 c, u32 w0, u32 rest) { ent.push_back(HostEntry{kind, c, w0, rest}); });
        });
        vit_mci_subch* S = h_sub + NSUBCH * (u64)g;
        for (u32 c = 0; c < NSUBCH; c++) S[c] = vit_mci_subch{};
        vit_mci_group R = {};
        u32 nens_o = 0;
        bool have_ens = false;
        u32 ens_eid = 0, ens_rest = 0;
        for (size_t k = ent.size(); k-- > 0;) {  // from the last entry back: the first one met is the one that wins
            const HostEntry& e = ent[k];
            vit_mci_subch& s = S[e.c];
            if (e.kind == E_ORG) {
                if (!s.org) s.org = e.w0;
                if (s.org == e.w0) s.n_org++;
                else s.n_org_other++;
            } else if (e.kind == E_COMP) {
                const u32 comp = COMP_PRESENT | e.rest;
                if (!s.comp) {
                    s.comp = comp;
                    s.sid = e.w0;
                }
                if (s.comp == comp && s.sid == e.w0) s.n_comp++;
                else s.n_comp_other++;
            } else {
                if (!have_ens) {
                    have_ens = true;
                    ens_eid = e.w0 >> 16;
                    ens_rest = e.rest;
                    R.eid = (uint16_t)ens_eid;
                    R.cif = (uint16_t)(e.w0 & 0xFFFFu);
                    R.flags = (uint8_t)(GRP_SEEN | e.rest << GRP_CHANGE_SHIFT);
                }
                if ((e.w0 >> 16) != ens_eid || e.rest != ens_rest) nens_o++;
            }
        }
        R.nfib_used = (uint16_t)n.used;
        R.nfib_malformed = (uint16_t)n.malf;
        R.n_ens_other = (uint16_t)nens_o;
        R.n_next = (uint16_t)n.next;
        h_grp[g] = R;
    }
}

hipError_t vit_launch_mci(const uint8_t* d_fibs, const uint8_t* d_fib_ok, int64_t nfibs, uint32_t G, vit_mci_subch* d_sub,
                          vit_mci_group* d_grp, uint8_t* d_status, hipStream_t stream) {
    if (nfibs <= 0) return hipSuccess;
    const long long ngroups = fib_ngroups(nfibs, G);
    hipLaunchKernelGGL(vit_mci_kernel, fib_grid(ngroups, G), dim3(TPB), 0, stream, d_fibs, d_fib_ok, (long long)nfibs, G,
                       ngroups, reinterpret_cast<u32*>(d_sub), reinterpret_cast<u32*>(d_grp), d_status);
    return hipGetLastError();
}
