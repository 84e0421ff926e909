// vit_fig_fmt.h -- every constant of the multiplex configuration (FIG 0/0, 0/1, 0/2 of EN 300 401 clause 6, the EEP rule
// of clause 11.3.2) that the library restates, in one place: vit_fib_group_dev.h (the walk over a FIB's FIGs, the FIG 0/2
// service list), vit_mci.hip and vit_mci_dir.hip (kernels, host twins) and vit_api_mci.hip (argument rule, profiles, the
// sub-channel table) take them from here, and include/viterbi_amd.h writes the same
// definitions out in words ("Multiplex configuration").  They were written down without the standard's text at hand; a
// correction against it is a change here plus the same change in the tests' model (tests/test_mci_host.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace figfmt {

constexpr uint32_t FIB_BYTES = 32;         // 30 bytes of FIGs and the CRC
constexpr uint32_t FIB_DATA = 30;          // only these are parsed
constexpr uint32_t END_MARKER = 0xFF;      // a FIG header of this value ends the FIB
constexpr uint32_t MAX_G = 4096;           // FIBs per group
constexpr uint32_t NSUBCH = 64;            // SubChId 0 ... 63
// Entries (a FIG 0/0, a sub-channel of a FIG 0/1, a component with TMId 0 or 1 of a FIG 0/2) one FIB can hold: the
// cheapest is a component, 2 bytes, behind 2 bytes of FIG header and 3 of service header - (30 - 5) / 2 = 12; a
// sub-channel costs 3 bytes and a FIG 0/0 six.  MAX_G * 12 = 49152 < 65536 keeps every count inside 16 bits; FIGs
// passed over cost 2 bytes at least: MAX_G * 15 = 61440.
constexpr uint32_t MAX_ENTRIES = 12;
static_assert(MAX_G * MAX_ENTRIES < 65536u && MAX_G * (FIB_DATA / 2u) < 65536u, "counts are 16 bits");

// FIG header: type(3) length(5); FIG type 0 body byte 0: C/N(1) OE(1) P/D(1) extension(5)
constexpr uint32_t FIG_LEN_MASK = 31, FIG_TYPE_SHIFT = 5;
constexpr uint32_t FIG0_CN = 0x80, FIG0_OE = 0x40, FIG0_PD = 0x20, FIG0_EXT_MASK = 31;
constexpr uint32_t EXT_ENSEMBLE = 0, EXT_SUBCH = 1, EXT_SERVICE = 2;
constexpr uint32_t FIG02_NCOMP_MASK = 15;    // FIG 0/2, a service's count byte: the number of components that follow

// vit_mci_subch.org
constexpr uint32_t ORG_PRESENT = 1u << 31, ORG_LONG = 1u << 30;
constexpr uint32_t ORG_START_MASK = 0x3FF;                 // bits 9..0
constexpr uint32_t ORG_SIZE_SHIFT = 10, ORG_SIZE_MASK = 0x3FF;   // long: bits 19..10
constexpr uint32_t ORG_LEVEL_SHIFT = 20, ORG_LEVEL_MASK = 3;     // long: bits 21..20
constexpr uint32_t ORG_OPTION_SHIFT = 22, ORG_OPTION_MASK = 7;   // long: bits 24..22
constexpr uint32_t ORG_INDEX_SHIFT = 10, ORG_INDEX_MASK = 63;    // short: bits 15..10
constexpr uint32_t ORG_SWITCH_SHIFT = 16;                        // short: bit 16
// vit_mci_subch.comp
constexpr uint32_t COMP_PRESENT = 1u << 31;
constexpr uint32_t COMP_TMID_MASK = 3;                     // bits 1..0
constexpr uint32_t COMP_TYPE_SHIFT = 2, COMP_TYPE_MASK = 63;     // bits 7..2
constexpr uint32_t COMP_PS_SHIFT = 8, COMP_CA_SHIFT = 9;
constexpr uint32_t COMP_TYPE_DABPLUS = 63;                 // audio service component type of DAB+ (with TMId 0)
// vit_mci_group.flags
constexpr uint32_t GRP_SEEN = 1, GRP_CHANGE_SHIFT = 1, GRP_AL_SHIFT = 3;
// d_status
constexpr uint32_t ST_USED = 1, ST_MALFORMED = 2, ST_FIG00 = 4, ST_FIG01 = 8, ST_FIG02 = 16;

// EEP (long form) profiles: a sub-channel of size_cu capacity units carries framebits = BITS * n per logical frame with
// n = size_cu / UNIT[level]; its L1 + L2 = framebits / 32 blocks of 32 trellis steps go under PI1 and PI2
constexpr uint32_t EEP_OPTIONS = 2, EEP_LEVELS = 4, EEP_NPI = 24, EEP_STEPS_PER_BLOCK = 32, EEP_TAIL_KEPT = 12;
constexpr uint32_t EEP_BITS[EEP_OPTIONS] = {192, 768};
constexpr uint32_t EEP_UNIT[EEP_OPTIONS][EEP_LEVELS] = {{12, 8, 6, 4}, {27, 21, 18, 15}};
struct EepRule {
    int l1n, l1c, l2n, l2c;  // L1 = l1n * n + l1c, L2 = l2n * n + l2c
    uint32_t pi1, pi2;
};
constexpr EepRule EEP_A[EEP_LEVELS] = {{6, -3, 0, 3, 24, 23}, {2, -3, 4, 3, 14, 13}, {6, -3, 0, 3, 8, 7}, {4, -3, 2, 3, 3, 2}};
constexpr EepRule EEP_A_2A_N1 = {0, 5, 0, 1, 13, 12};  // option A, level 1, n = 1
constexpr EepRule EEP_B[EEP_LEVELS] = {{24, -3, 0, 3, 10, 9}, {24, -3, 0, 3, 6, 5}, {24, -3, 0, 3, 4, 3}, {24, -3, 0, 3, 2, 1}};
constexpr uint32_t CU_SYMBOLS = 64;        // transmitted symbols (bits) of one capacity unit
constexpr uint32_t DABPLUS_BITS = 192;     // framebits = 192 * RSDims

// ---- the service directory (vit_mci_dir.hip; include/viterbi_amd.h, "Service directory"; the model is in
// tests/test_mci_dir_host.py): FIG 0/2 (services, TMId-3 components), FIG 0/3 (packet-mode components), FIG 1/0, 1/1, 1/5
constexpr uint32_t DIR_MAX = 64;           // records per group and table (VIT_DIR_MAX)
constexpr uint32_t EXT_PACKET = 3;         // FIG 0/3
constexpr uint32_t FIG1_EXT_MASK = 7, FIG1_OE = 0x08, FIG1_CHARSET_SHIFT = 4;
constexpr uint32_t EXT_LABEL_ENS = 0, EXT_LABEL_SVC16 = 1, EXT_LABEL_SVC32 = 5;
constexpr uint32_t LABEL_BYTES = 16, LABEL_VALUE_BYTES = 18;   // the label, and with its character flag field
constexpr uint32_t TMID_PACKET = 3;
constexpr uint32_t LOC_BYTES = 5, LOC_CAORG_BYTES = 2;
// Entries one FIB can hold.  A FIG 0/2 costs 2 bytes of header; a service entry 3 at least (16-bit SId, count byte), a
// component entry 2 behind its service's: 2 + 3k + 2(n - k) <= 30 gives n <= 13 with k = 1 (one service, 12 components),
// and k <= 9 alone.  A location entry costs 5 bytes, (30 - 2) / 5 = 5.  A label costs 1 + 1 + 2 + 18 = 22 bytes: one, and
// the 8 bytes beside it hold two more entries at most.  A FIG passed over costs 2 bytes at least, as above.
constexpr uint32_t DIR_MAX_ENTRIES = 13, DIR_MAX_SVC_ENTRIES = 9, DIR_MAX_LOC_ENTRIES = 5, DIR_MAX_LABELS = 1;
static_assert(2u + 3u + 2u * (DIR_MAX_ENTRIES - 1u) <= FIB_DATA && 2u + 3u + 2u * DIR_MAX_ENTRIES > FIB_DATA, "13 entries");
static_assert(2u + 3u * DIR_MAX_SVC_ENTRIES <= FIB_DATA && 2u + 3u * (DIR_MAX_SVC_ENTRIES + 1u) > FIB_DATA, "9 services");
static_assert(2u + LOC_BYTES * DIR_MAX_LOC_ENTRIES <= FIB_DATA && 2u + LOC_BYTES * (DIR_MAX_LOC_ENTRIES + 1u) > FIB_DATA, "5 locations");
static_assert(2u + 2u + LABEL_VALUE_BYTES <= FIB_DATA && 2u * (2u + 2u + LABEL_VALUE_BYTES) > FIB_DATA, "1 label");
static_assert(MAX_G * DIR_MAX_ENTRIES < 65536u && MAX_G * DIR_MAX_SVC_ENTRIES < 65536u && MAX_G * DIR_MAX_LOC_ENTRIES < 65536u &&
              MAX_G * DIR_MAX_LABELS < 65536u, "counts are 16 bits");
// vit_mci_service.flags, vit_mci_pktcomp.flags, vit_mci_pktcomp.loc, vit_mci_dir.flags
constexpr uint32_t SVC_LABEL = 1, SVC_LISTED = 2, SVC_PD_SHIFT = 2, SVC_CHARSET_SHIFT = 4;
constexpr uint32_t PKT_LOC = 1, PKT_COMP = 2, PKT_PS_SHIFT = 2, PKT_CA_SHIFT = 3;
constexpr uint32_t LOC_SUBCH_MASK = 63, LOC_ADDR_SHIFT = 6, LOC_DSCTY_SHIFT = 16, LOC_DG_SHIFT = 22, LOC_CAORG_SHIFT = 23;
constexpr uint32_t DIR_LABEL = 1, DIR_SVC_OVERFLOW = 2, DIR_PKT_OVERFLOW = 4;
// d_status of vit_mci_dir_dev
constexpr uint32_t ST_DIR_FIG02 = 4, ST_DIR_FIG03 = 8, ST_DIR_FIG1 = 16;

}  // namespace figfmt
