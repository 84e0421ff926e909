// vit_api_ens.hip -- the C ABI for a whole ensemble (include/viterbi_amd.h, vit_ens_subch): the layout rule, the table
// forms of RS and the access units, and the chain from the CIF ring.  Argument rules and launches only; the kernels are
// in rs_kernels.hip and vit_dab.hip, the launch plan in vit_internal.h.
#include <algorithm>

#include "vit_host.h"

namespace {

inline uint64_t align16(uint64_t x) { return (x + 15u) & ~(uint64_t)15u; }

// The table's rules and its layout (h_out optional); false, with the error text naming the entry, if one is broken.
bool ens_layout(const char* who, const vit_ens_subch* h_sub, uint32_t nsub, vit_ens_layout* h_out) {
    if (!h_sub || nsub < 1u || nsub > VIT_ENS_MAX_SUBCH) {
        set_err("%s: bad arguments (nsub=%u, 1 ... %u; h_sub)", who, nsub, (unsigned)VIT_ENS_MAX_SUBCH);
        return false;
    }
    vit_ens_layout lay = {};
    uint64_t rows = 0;
    for (uint32_t k = 0; k < nsub; k++) {
        const vit_ens_subch& s = h_sub[k];
        const char* why = nullptr;
        if (s.framebits == 0 || s.framebits > VIT_MAX_FRAMEBITS || (s.framebits & 7u)) why = "framebits must be a multiple of 8 in 8 ... 9216";
        else if (s.RSDims > 48u) why = "RSDims must be 0 (not DAB+) or 1 ... 48";
        else if (s.RSDims && s.framebits != 192u * s.RSDims) why = "a DAB+ entry's framebits must be 192*RSDims";
        else if (s.nframes == 0) why = "nframes must be at least 1";
        else if (s.RSDims && s.nframes % 5u) why = "a DAB+ entry's nframes must be a multiple of 5";
        else if ((uint64_t)s.phase + s.nframes + 15u > 0xFFFFFFFFull) why = "phase + nframes + 15 must fit 32 bits";
        else if (s.reserved) why = "reserved must be 0";
        if (why) {
            set_err("%s: bad arguments (entry %u: %s; framebits=%u RSDims=%u phase=%u nframes=%u reserved=%u)", who, k, why,
                    s.framebits, s.RSDims, s.phase, s.nframes, s.reserved);
            return false;
        }
        lay.work_offset[k] = align16(lay.work_bytes);
        lay.rs_offset[k] = align16(lay.rs_bytes);
        lay.rec_index[k] = lay.nrec;
        lay.work_bytes = lay.work_offset[k] + (uint64_t)s.nframes * (s.framebits / 8u);
        lay.rs_bytes = lay.rs_offset[k] + (s.RSDims ? (uint64_t)(s.nframes / 5u) * 110u * s.RSDims : 0u);
        lay.nrec += s.RSDims ? s.nframes / 5u : 0u;
        rows = std::max(rows, (uint64_t)s.phase + s.nframes + 15u);
        lay.max_framebits = std::max(lay.max_framebits, s.framebits);
    }
    lay.rows_needed = (uint32_t)rows;
    if (h_out) *h_out = lay;
    return true;
}

// The table as the kernels read it; false (error text set) if its frames, records or RS passes do not fit the kernels'
// 32-bit indices (2^31 frames).
bool ens_device_table(const char* who, const vit_ens_subch* h_sub, uint32_t nsub, const vit_ens_layout& lay, VitEnsTable* tab) {
    *tab = VitEnsTable{};
    uint64_t frames = 0, passes = 0;
    for (uint32_t k = 0; k < nsub; k++) {
        const vit_ens_subch& s = h_sub[k];
        if (frames + s.nframes > 0x7FFFFFFFull) {
            set_err("%s: bad arguments (the table holds more than 2^31 - 1 frames)", who);
            return false;
        }
        VitEnsEntry& e = tab->e[k];
        e.work_off = lay.work_offset[k];
        e.rs_off = lay.rs_offset[k];
        e.rec0 = (uint32_t)lay.rec_index[k];
        e.frame0 = (uint32_t)frames;
        e.pass0 = (uint32_t)passes;
        e.framebits = (uint16_t)s.framebits;
        e.rsdims = (uint16_t)s.RSDims;
        frames += s.nframes;
        if (s.RSDims) {
            const uint32_t spb = 256u / s.RSDims, nsf = s.nframes / 5u;
            passes += (nsf + spb - 1u) / spb;
            tab->max_rsdims = std::max(tab->max_rsdims, s.RSDims);
        }
    }
    tab->nsub = nsub;
    tab->nframes = (uint32_t)frames;
    tab->nrec = (uint32_t)lay.nrec;
    tab->npass = (uint32_t)passes;
    return true;
}

}  // namespace

extern "C" {

int vit_ensemble_layout(const vit_ens_subch* h_sub, uint32_t nsub, vit_ens_layout* h_out) {
    if (!h_out) return bad_arg("vit_ensemble_layout: bad arguments (h_out)");
    return ens_layout("vit_ensemble_layout", h_sub, nsub, h_out) ? VIT_OK : VIT_ERR_ARG;
}

int vit_rs_table_dev(const uint8_t* d_work, uint8_t* d_rs_out, int32_t* d_ret, const vit_ens_subch* h_sub, uint32_t nsub,
                     void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    vit_ens_layout lay;
    VitEnsTable tab;
    if (!ens_layout("vit_rs_table_dev", h_sub, nsub, &lay) || !ens_device_table("vit_rs_table_dev", h_sub, nsub, lay, &tab))
        return VIT_ERR_ARG;
    if (tab.nrec > 0 && (!d_work || !d_rs_out || !d_ret)) return bad_arg("vit_rs_table_dev: bad arguments (NULL pointer)");
    LAUNCHCHK("rs table launch failed: %s", rs_table_launch(d_work, d_rs_out, d_ret, tab, (hipStream_t)stream));
    return VIT_OK;
}

int vit_dabplus_aus_table_dev(const uint8_t* d_sf, int from_work, const vit_ens_subch* h_sub, uint32_t nsub,
                              const int32_t* d_ret, vit_au_table* d_au, void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    vit_ens_layout lay;
    VitEnsTable tab;
    if (!ens_layout("vit_dabplus_aus_table_dev", h_sub, nsub, &lay) ||
        !ens_device_table("vit_dabplus_aus_table_dev", h_sub, nsub, lay, &tab))
        return VIT_ERR_ARG;
    if ((from_work != 0 && from_work != 1) || (tab.nrec > 0 && (!d_sf || !d_au || (reinterpret_cast<uintptr_t>(d_au) & 3u))))
        return bad_arg("vit_dabplus_aus_table_dev: bad arguments (from_work=%d, 0 or 1; d_sf; d_au 4-byte aligned)", from_work);
    LAUNCHCHK("access unit table launch failed: %s",
              vit_launch_aus_table(d_sf, from_work != 0, tab, d_ret, d_au, (hipStream_t)stream));
    return VIT_OK;
}

int vit_ensemble_dev(const vit_cif_ring* ring, uint64_t msc_col, const vit_ens_subch* h_sub, uint32_t nsub,
                     const vit_punct_profile* d_profiles, uint32_t nprofiles, uint8_t erasure, uint8_t* d_work, uint8_t* d_rs_out,
                     int32_t* d_ret, uint8_t* d_fire_ok, vit_au_table* d_au, void* stream) {
    static const char* const who = "vit_ensemble_dev";
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    vit_ens_layout lay;
    VitEnsTable tab;
    if (!ens_layout(who, h_sub, nsub, &lay) || !ens_device_table(who, h_sub, nsub, lay, &tab)) return VIT_ERR_ARG;
    if (!d_work || !d_profiles || (tab.nrec > 0 && (!d_rs_out || !d_ret)) || (reinterpret_cast<uintptr_t>(d_au) & 3u))
        return bad_arg("%s: bad arguments (d_work, d_profiles, d_rs_out, d_ret; d_au 4-byte aligned)", who);
    if (!ring_check_base(who, ring, "%s: bad arguments (NULL ring or d_base)")) return VIT_ERR_ARG;
    if (lay.rows_needed > ring->nrows)
        return bad_arg("%s: bad arguments (the table needs %u distinct rows, the ring has %u)", who, lay.rows_needed, ring->nrows);
    // the span of columns the table uses, relative to msc_col
    uint64_t lo = ~0ull, hi = 0;
    for (uint32_t k = 0; k < nsub; k++) {
        const vit_ens_subch& s = h_sub[k];
        if (s.col & 15u) return bad_arg("%s: bad arguments (entry %u: col=%u is not a multiple of 16)", who, k, s.col);
        if (s.profile >= nprofiles) return bad_arg("%s: bad arguments (entry %u: profile %u >= nprofiles %u)", who, k, s.profile, nprofiles);
        if (msc_col > ring->row_bytes || !ring_check_cols(who, ring, msc_col + s.col, s.nsym)) {
            set_err("%s: bad arguments (entry %u: columns [%llu + %u, + %u) outside row_bytes %llu)", who, k, (unsigned long long)msc_col,
                    s.col, s.nsym, (unsigned long long)ring->row_bytes);
            return VIT_ERR_ARG;
        }
        lo = std::min<uint64_t>(lo, s.col);
        hi = std::max<uint64_t>(hi, (uint64_t)s.col + s.nsym);
    }
    const uint64_t span = hi - lo;  // < 2^33; the de-interleave takes 32 bits
    if (span > 0xFFFFFFFFull) return bad_arg("%s: bad arguments (the table spans %llu columns)", who, (unsigned long long)span);
    VitEnsSource src = {};
    for (uint32_t k = 0; k < nsub; k++) {
        src.sym0[k] = (uint32_t)(h_sub[k].col - lo);
        src.phase[k] = h_sub[k].phase;
        src.profile[k] = h_sub[k].profile;
    }
    const hipStream_t s = (hipStream_t)stream;
    const int64_t nspan = (int64_t)lay.rows_needed - 15;  // logical frames of the call
    // one lease: the de-interleaved span, then the expansion slots; the table's descriptors, then the checked ones
    const size_t deint_bytes = (size_t)align16((uint64_t)nspan * span), slot = 4u * ((size_t)lay.max_framebits + VIT_TAIL);
    ScratchLease scratch;
    int rc = scratch.begin(deint_bytes + (size_t)tab.nframes * slot, 2u * (size_t)tab.nframes * sizeof(vit_frame_desc), s);
    if (rc != VIT_OK) return rc;
    uint8_t* d_deint = scratch.sym<uint8_t>();
    uint8_t* d_slots = d_deint + deint_bytes;
    vit_frame_desc* d_desc = scratch.desc();
    vit_frame_desc* d_idesc = d_desc + tab.nframes;
    LAUNCHCHK("time de-interleave launch failed: %s",
              vit_launch_time_deinterleave(*ring, msc_col + lo, (uint32_t)span, d_deint, nspan, s));
    LAUNCHCHK("ensemble descriptor launch failed: %s", vit_launch_ens_descs(tab, src, span, d_desc, s));
    LAUNCHCHK("depuncture launch failed: %s",
              vit_launch_depunct_varlen(d_deint, (uint64_t)nspan * span, lay.work_bytes, d_desc, tab.nframes, lay.max_framebits,
                                        d_profiles, nprofiles, erasure, d_slots, d_idesc, s));
    rc = launch_decode(decode_mode(), d_slots, false, d_work, d_idesc, 0, lay.max_framebits, tab.nframes, s);
    if (rc != VIT_OK) return rc;
    LAUNCHCHK("ensemble post-pass launch failed: %s", vit_launch_ens_post(d_work, tab, d_idesc, d_fire_ok, s));
    LAUNCHCHK("rs table launch failed: %s", rs_table_launch(d_work, d_rs_out, d_ret, tab, s));
    if (d_au) LAUNCHCHK("access unit table launch failed: %s", vit_launch_aus_table(d_rs_out, false, tab, d_ret, d_au, s));
    return scratch.end();
}

}  // extern "C"
