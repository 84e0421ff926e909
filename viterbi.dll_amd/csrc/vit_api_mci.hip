// vit_api_mci.hip -- the C ABI of the multiplex configuration (include/viterbi_amd.h, "Multiplex configuration"): the
// argument rules and the launch of vit_mci_fibs_dev, and the two host-only steps behind it - the EEP profile of a
// sub-channel and the table for vit_ensemble_dev.  The kernel and the host twin are in vit_mci.hip, the format's constants
// and the EEP rule in vit_fig_fmt.h.
#include <string.h>

#include "vit_fig_fmt.h"
#include "vit_host.h"

using namespace figfmt;

namespace {

inline bool misaligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; }

// the rule every form of the FIB call shares; nullptr if the arguments are fine
const char* mci_args_wrong(const void* fibs, int64_t nfibs, uint32_t G, const void* sub, const void* grp) {
    if (nfibs < 0) return "nfibs must not be negative";
    if (G < 1u || G > MAX_G) return "G must be 1 ... 4096";
    if (nfibs > 0 && (!fibs || !sub || !grp)) return "NULL fibs, sub or grp";
    return nullptr;
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
    const char* why = mci_args_wrong(d_fibs, nfibs, G, d_sub, d_grp);
    if (!why && nfibs > 0 && (misaligned4(d_sub) || misaligned4(d_grp))) why = "d_sub and d_grp must be 4-byte aligned";
    if (why) return bad_arg("vit_mci_fibs_dev: bad arguments (%s; nfibs=%lld G=%u)", why, (long long)nfibs, G);
    LAUNCHCHK("multiplex configuration launch failed: %s",
              vit_launch_mci(d_fibs, d_fib_ok, nfibs, G, d_sub, d_grp, d_status, (hipStream_t)stream));
    return VIT_OK;
}

int vit_mci_fibs_host(const uint8_t* h_fibs, const uint8_t* h_fib_ok, int64_t nfibs, uint32_t G, vit_mci_subch* h_sub,
                      vit_mci_group* h_grp, uint8_t* h_status) {
    const char* why = mci_args_wrong(h_fibs, nfibs, G, h_sub, h_grp);
    if (why) return bad_arg("vit_mci_fibs_host: bad arguments (%s; nfibs=%lld G=%u)", why, (long long)nfibs, G);
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

int vit_mci_ens_table(const vit_mci_subch h_sub[64], const uint32_t keep_pi[24], uint32_t keep_tail, vit_ens_subch* h_out,
                      uint32_t* nsub, vit_punct_profile* h_profiles, uint32_t* nprofiles, uint64_t* skipped) {
    if (!h_sub || !h_out || !nsub || !h_profiles || !nprofiles || !skipped)
        return bad_arg("vit_mci_ens_table: bad arguments (NULL pointer)");
    if (!vectors_ok(keep_pi, keep_tail))
        return bad_arg("vit_mci_ens_table: bad arguments (keep_pi[i] must have 8+i+1 one bits, keep_tail 12 in its low 24)");
    const uint32_t cap = *nprofiles;
    uint32_t rows = 0, nprof = 0;
    uint64_t skip = 0;
    for (uint32_t c = 0; c < NSUBCH; c++) {
        const uint32_t org = h_sub[c].org, comp = h_sub[c].comp;
        if (!(org & ORG_PRESENT)) continue;
        vit_punct_profile prof;
        uint32_t fb = 0;
        const uint32_t size = (org >> ORG_SIZE_SHIFT) & ORG_SIZE_MASK;
        if (!(org & ORG_LONG) || !(comp & COMP_PRESENT) ||
            !eep_build((org >> ORG_OPTION_SHIFT) & ORG_OPTION_MASK, (org >> ORG_LEVEL_SHIFT) & ORG_LEVEL_MASK, size, keep_pi,
                       keep_tail, &prof, &fb)) {
            skip |= 1ull << c;
            continue;
        }
        uint32_t k = 0;
        while (k < nprof && memcmp(&h_profiles[k], &prof, sizeof(prof)) != 0) k++;
        if (k == nprof) {
            if (nprof == cap)
                return bad_arg("vit_mci_ens_table: bad arguments (h_profiles holds %u profiles, SubChId %u needs one more)", cap, c);
            h_profiles[nprof++] = prof;
        }
        const bool dabplus = (comp & COMP_TMID_MASK) == 0 && ((comp >> COMP_TYPE_SHIFT) & COMP_TYPE_MASK) == COMP_TYPE_DABPLUS;
        vit_ens_subch row = {};
        row.col = CU_SYMBOLS * (org & ORG_START_MASK);
        row.profile = k;
        row.framebits = fb;
        row.RSDims = dabplus ? fb / DABPLUS_BITS : 0u;
        row.nsym = CU_SYMBOLS * size;
        h_out[rows++] = row;
    }
    *nsub = rows;
    *nprofiles = nprof;
    *skipped = skip;
    return VIT_OK;
}
