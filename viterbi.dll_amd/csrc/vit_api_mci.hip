// vit_api_mci.hip -- the C ABI of the multiplex configuration (include/viterbi_amd.h, "Multiplex configuration"): the
// argument rules and the launch of vit_mci_fibs_dev, and the two host-only steps behind it - the EEP profile of a
// sub-channel and the table for vit_ensemble_dev.  The kernel and the host twin are in vit_mci.hip, the format's constants
// and the EEP rule in vit_fig_fmt.h.  Behind them the service directory ("Service directory"): vit_mci_dir_dev and its
// host twin (vit_mci_dir.hip), and the two host-only steps that lead from it to the table of vit_packet_table_dev.
#include <string.h>
#include <initializer_list>

#include "vit_fig_fmt.h"
#include "vit_host.h"

using namespace figfmt;

namespace {

// The rule every FIB call shares, host and device form: VIT_OK, or bad_arg.  `outs` are the call's record pointers and
// `names` says how the messages call them; the device forms (`device`) also want them 4-byte aligned.
struct FibOutNames { const char *null, *misaligned; };
constexpr FibOutNames MCI_OUTS = {"NULL fibs, sub or grp", "d_sub and d_grp must be 4-byte aligned"};
constexpr FibOutNames DIR_OUTS = {"NULL fibs, svc, pkt or dir", "d_svc, d_pkt and d_dir must be 4-byte aligned"};

int fib_args(const char* who, bool device, const void* fibs, int64_t nfibs, uint32_t G, std::initializer_list<const void*> outs,
             const FibOutNames& names) {
    bool null = !fibs, misaligned = false;
    for (const void* p : outs) {
        null = null || !p;
        misaligned = misaligned || (reinterpret_cast<uintptr_t>(p) & 3u) != 0;
    }
    const char* why = nullptr;
    if (nfibs < 0) why = "nfibs must not be negative";
    else if (G < 1u || G > MAX_G) why = "G must be 1 ... 4096";
    else if (nfibs > 0 && null) why = names.null;
    else if (nfibs > 0 && device && misaligned) why = names.misaligned;
    return why ? bad_arg("%s: bad arguments (%s; nfibs=%lld G=%u)", who, why, (long long)nfibs, G) : VIT_OK;
}

bool vectors_ok(const uint32_t* keep_pi, uint32_t keep_tail) {
    if (!keep_pi) return false;
    for (uint32_t i = 0; i < EEP_NPI; i++)
        if ((uint32_t)__builtin_popcount(keep_pi[i]) != 8u + i + 1u) return false;
    return (keep_tail >> 24) == 0 && (uint32_t)__builtin_popcount(keep_tail) == EEP_TAIL_KEPT;
}

// the rule alone (vectors checked by the caller); false: no such profile
bool eep_build(uint32_t option, uint32_t level, uint32_t size_cu, const uint32_t* keep_pi, uint32_t keep_tail,
               vit_punct_profile* out, uint32_t* framebits) {
    if (option >= EEP_OPTIONS || level >= EEP_LEVELS) return false;
    const uint32_t unit = EEP_UNIT[option][level];
    if (size_cu == 0 || size_cu % unit) return false;
    const uint32_t n = size_cu / unit, fb = EEP_BITS[option] * n;
    if (fb > VIT_MAX_FRAMEBITS) return false;
    const EepRule& r = option == 1u ? EEP_B[level] : (level == 1u && n == 1u) ? EEP_A_2A_N1 : EEP_A[level];
    const uint32_t l1 = (uint32_t)(r.l1n * (int)n + r.l1c), l2 = (uint32_t)(r.l2n * (int)n + r.l2c);
    memset(out, 0, sizeof(*out));
    out->nsegs = 3;
    out->seg[0] = vit_punct_seg{EEP_STEPS_PER_BLOCK * l1, keep_pi[r.pi1 - 1u]};
    out->seg[1] = vit_punct_seg{EEP_STEPS_PER_BLOCK * l2, keep_pi[r.pi2 - 1u]};
    out->seg[2] = vit_punct_seg{VIT_TAIL, keep_tail};
    *framebits = fb;
    return true;
}

}  // namespace

int vit_mci_fibs_dev(const uint8_t* d_fibs, const uint8_t* d_fib_ok, int64_t nfibs, uint32_t G, vit_mci_subch* d_sub,
                     vit_mci_group* d_grp, uint8_t* d_status, void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (int rc = fib_args("vit_mci_fibs_dev", true, d_fibs, nfibs, G, {d_sub, d_grp}, MCI_OUTS)) return rc;
    LAUNCHCHK("multiplex configuration launch failed: %s",
              vit_launch_mci(d_fibs, d_fib_ok, nfibs, G, d_sub, d_grp, d_status, (hipStream_t)stream));
    return VIT_OK;
}

int vit_mci_fibs_host(const uint8_t* h_fibs, const uint8_t* h_fib_ok, int64_t nfibs, uint32_t G, vit_mci_subch* h_sub,
                      vit_mci_group* h_grp, uint8_t* h_status) {
    if (int rc = fib_args("vit_mci_fibs_host", false, h_fibs, nfibs, G, {h_sub, h_grp}, MCI_OUTS)) return rc;
    if (nfibs > 0) vit_mci_fibs_host_impl(h_fibs, h_fib_ok, nfibs, G, h_sub, h_grp, h_status);
    return VIT_OK;
}

int vit_eep_profile(uint32_t option, uint32_t level, uint32_t size_cu, const uint32_t keep_pi[24], uint32_t keep_tail,
                    vit_punct_profile* out, uint32_t* framebits) {
    if (!out || !framebits) return bad_arg("vit_eep_profile: bad arguments (NULL pointer)");
    if (!vectors_ok(keep_pi, keep_tail))
        return bad_arg("vit_eep_profile: bad arguments (keep_pi[i] must have 8+i+1 one bits, keep_tail 12 in its low 24)");
    if (!eep_build(option, level, size_cu, keep_pi, keep_tail, out, framebits))
        return bad_arg("vit_eep_profile: bad arguments (option=%u, 0 ... 1; level=%u, 0 ... 3; size_cu=%u, a positive multiple "
                       "of the level's unit with framebits <= 9216)", option, level, size_cu);
    return VIT_OK;
}

namespace {

// vit_mci_ens_table (packet = 0, packet_rows = nullptr) and vit_mci_dir_ens_table: `packet` is the mask of the SubChIds
// that a FIG 0/3 entry names; one of them without a component gives a row where the first call skips it
int ens_table(const char* who, const vit_mci_subch* h_sub, uint64_t packet, const uint32_t* keep_pi, uint32_t keep_tail,
              vit_ens_subch* h_out, uint32_t* nsub, vit_punct_profile* h_profiles, uint32_t* nprofiles, uint64_t* skipped,
              uint64_t* packet_rows) {
    if (!vectors_ok(keep_pi, keep_tail))
        return bad_arg("%s: bad arguments (keep_pi[i] must have 8+i+1 one bits, keep_tail 12 in its low 24)", who);
    const uint32_t cap = *nprofiles;
    uint32_t rows = 0, nprof = 0;
    uint64_t skip = 0, marked = 0;
    for (uint32_t c = 0; c < NSUBCH; c++) {
        const uint32_t org = h_sub[c].org, comp = h_sub[c].comp;
        if (!(org & ORG_PRESENT)) continue;
        vit_punct_profile prof;
        uint32_t fb = 0;
        const uint32_t size = (org >> ORG_SIZE_SHIFT) & ORG_SIZE_MASK;
        const bool has_comp = (comp & COMP_PRESENT) != 0, named = !has_comp && ((packet >> c) & 1u);
        if (!(org & ORG_LONG) || !(has_comp || named) ||
            !eep_build((org >> ORG_OPTION_SHIFT) & ORG_OPTION_MASK, (org >> ORG_LEVEL_SHIFT) & ORG_LEVEL_MASK, size, keep_pi,
                       keep_tail, &prof, &fb)) {
            skip |= 1ull << c;
            continue;
        }
        uint32_t k = 0;
        while (k < nprof && memcmp(&h_profiles[k], &prof, sizeof(prof)) != 0) k++;
        if (k == nprof) {
            if (nprof == cap) return bad_arg("%s: bad arguments (h_profiles holds %u profiles, SubChId %u needs one more)", who, cap, c);
            h_profiles[nprof++] = prof;
        }
        const bool dabplus = has_comp && (comp & COMP_TMID_MASK) == 0 && ((comp >> COMP_TYPE_SHIFT) & COMP_TYPE_MASK) == COMP_TYPE_DABPLUS;
        vit_ens_subch row = {};
        row.col = CU_SYMBOLS * (org & ORG_START_MASK);
        row.profile = k;
        row.framebits = fb;
        row.RSDims = dabplus ? fb / DABPLUS_BITS : 0u;
        row.nsym = CU_SYMBOLS * size;
        if (named) marked |= 1ull << rows;
        h_out[rows++] = row;
    }
    *nsub = rows;
    *nprofiles = nprof;
    *skipped = skip;
    if (packet_rows) *packet_rows = marked;
    return VIT_OK;
}

static_assert(sizeof(vit_mci_service) == 32 && sizeof(vit_mci_pktcomp) == 20 && sizeof(vit_mci_dir) == 40, "record sizes");

}  // namespace

int vit_mci_ens_table(const vit_mci_subch h_sub[64], const uint32_t keep_pi[24], uint32_t keep_tail, vit_ens_subch* h_out,
                      uint32_t* nsub, vit_punct_profile* h_profiles, uint32_t* nprofiles, uint64_t* skipped) {
    if (!h_sub || !h_out || !nsub || !h_profiles || !nprofiles || !skipped)
        return bad_arg("vit_mci_ens_table: bad arguments (NULL pointer)");
    return ens_table("vit_mci_ens_table", h_sub, 0, keep_pi, keep_tail, h_out, nsub, h_profiles, nprofiles, skipped, nullptr);
}

int vit_mci_dir_dev(const uint8_t* d_fibs, const uint8_t* d_fib_ok, int64_t nfibs, uint32_t G, vit_mci_service* d_svc,
                    vit_mci_pktcomp* d_pkt, vit_mci_dir* d_dir, uint8_t* d_status, void* stream) {
    if (hip_device_ready() != VIT_OK) return VIT_ERR_NO_DEVICE;
    if (int rc = fib_args("vit_mci_dir_dev", true, d_fibs, nfibs, G, {d_svc, d_pkt, d_dir}, DIR_OUTS)) return rc;
    LAUNCHCHK("service directory launch failed: %s",
              vit_launch_mci_dir(d_fibs, d_fib_ok, nfibs, G, d_svc, d_pkt, d_dir, d_status, (hipStream_t)stream));
    return VIT_OK;
}

int vit_mci_dir_host(const uint8_t* h_fibs, const uint8_t* h_fib_ok, int64_t nfibs, uint32_t G, vit_mci_service* h_svc,
                     vit_mci_pktcomp* h_pkt, vit_mci_dir* h_dir, uint8_t* h_status) {
    if (int rc = fib_args("vit_mci_dir_host", false, h_fibs, nfibs, G, {h_svc, h_pkt, h_dir}, DIR_OUTS)) return rc;
    if (nfibs > 0) vit_mci_dir_host_impl(h_fibs, h_fib_ok, nfibs, G, h_svc, h_pkt, h_dir, h_status);
    return VIT_OK;
}

int vit_mci_dir_ens_table(const vit_mci_subch h_sub[64], const vit_mci_pktcomp* h_pkt, uint32_t npkt, const uint32_t keep_pi[24],
                          uint32_t keep_tail, vit_ens_subch* h_out, uint32_t* nsub, vit_punct_profile* h_profiles,
                          uint32_t* nprofiles, uint64_t* skipped, uint64_t* packet_rows) {
    if (!h_sub || !h_out || !nsub || !h_profiles || !nprofiles || !skipped || !packet_rows || (npkt > 0 && !h_pkt))
        return bad_arg("vit_mci_dir_ens_table: bad arguments (NULL pointer)");
    if (npkt > DIR_MAX) return bad_arg("vit_mci_dir_ens_table: bad arguments (npkt=%u, at most 64)", npkt);
    uint64_t packet = 0;
    for (uint32_t i = 0; i < npkt; i++)
        if (h_pkt[i].flags & PKT_LOC) packet |= 1ull << (h_pkt[i].loc & LOC_SUBCH_MASK);
    return ens_table("vit_mci_dir_ens_table", h_sub, packet, keep_pi, keep_tail, h_out, nsub, h_profiles, nprofiles, skipped,
                     packet_rows);
}

int vit_mci_pkt_table(const vit_ens_subch* h_rows, uint32_t nsub, const vit_ens_layout* h_layout, uint64_t packet_rows,
                      uint32_t fec, uint32_t min_score, vit_pkt_stream h_out[64], uint32_t* nstreams, uint32_t* h_row_of_stream) {
    if (!h_rows || !h_layout || !h_out || !nstreams) return bad_arg("vit_mci_pkt_table: bad arguments (NULL pointer)");
    if (nsub < 1u || nsub > VIT_ENS_MAX_SUBCH) return bad_arg("vit_mci_pkt_table: bad arguments (nsub=%u, 1 ... 64)", nsub);
    if (nsub < 64u && (packet_rows >> nsub)) return bad_arg("vit_mci_pkt_table: bad arguments (packet_rows marks a row at or above nsub=%u)", nsub);
    if (fec != VIT_PKT_FEC_NONE && fec != VIT_PKT_FEC_SEARCH)
        return bad_arg("vit_mci_pkt_table: bad arguments (fec=%u: VIT_PKT_FEC_NONE or VIT_PKT_FEC_SEARCH; one phase does not fit several streams)", fec);
    if (fec == VIT_PKT_FEC_NONE && min_score) return bad_arg("vit_mci_pkt_table: bad arguments (min_score=%u without a search)", min_score);
    for (uint32_t k = 0; k < nsub; k++) {
        if (!((packet_rows >> k) & 1u)) continue;
        const uint32_t fbytes = h_rows[k].framebits / 8u;
        if (h_rows[k].RSDims || !h_rows[k].nframes || (h_rows[k].framebits & 7u) || fbytes % 24u || fbytes < 24u || fbytes > 1152u)
            return bad_arg("vit_mci_pkt_table: bad arguments (row %u: RSDims=%u, 0; nframes=%u, >= 1; framebits=%u, framebits/8 a "
                           "multiple of 24 in 24 ... 1152)", k, h_rows[k].RSDims, h_rows[k].nframes, h_rows[k].framebits);
    }
    uint32_t n = 0;
    for (uint32_t k = 0; k < nsub; k++) {
        if (!((packet_rows >> k) & 1u)) continue;
        vit_pkt_stream s = {};
        s.offset = h_layout->work_offset[k];
        s.framebytes = h_rows[k].framebits / 8u;
        s.nframes = h_rows[k].nframes;
        s.fec = fec;
        s.min_score = min_score;
        if (h_row_of_stream) h_row_of_stream[n] = k;
        h_out[n++] = s;
    }
    *nstreams = n;
    return VIT_OK;
}
