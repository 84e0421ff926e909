// vit_packet_fmt.h -- every constant of packet mode and its FEC (EN 300 401 clause 5.3) that the library restates, in
// one place: vit_packet.hip (kernels, host twin) and vit_api_packet.hip (argument rules) take them from here, and
// include/viterbi_amd.h writes the same definitions out in words.  They were written down without the standard's text at
// hand; a correction against it is a change here plus the same change in the tests' model (tests/test_packet_host.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pktfmt {

constexpr uint32_t SLOT = 24;               // bytes of the shortest packet; every packet is 1 ... 4 slots
constexpr uint32_t MAX_FRAMEBYTES = 1152;   // 9216 bits: the longest logical frame
constexpr uint32_t MAX_SLOTS = MAX_FRAMEBYTES / SLOT;  // 48

// packet header: byte 0 = length(2) continuity(2) first/last(2) address(9..8), byte 1 = address(7..0),
// byte 2 = command(1) useful data length(7)
constexpr uint32_t LEN_SHIFT = 6;           // byte 0 bits 7..6: (slots - 1)
constexpr uint32_t CONT_SHIFT = 4;          // byte 0 bits 5..4
constexpr uint32_t FL_SHIFT = 2;            // byte 0 bits 3..2
constexpr uint32_t ADDR_HI_MASK = 3;        // byte 0 bits 1..0
constexpr uint32_t CMD_MASK = 0x80;         // byte 2 bit 7
constexpr uint32_t USEFUL_MASK = 0x7F;      // byte 2 bits 6..0
constexpr uint32_t ADDR_PADDING = 0;
constexpr uint32_t ADDR_FEC = 1022;
constexpr uint32_t NADDR = 1024;            // the address field's range; 1 ... 1021 and 1023 carry data
constexpr uint32_t PKT_DATA_OFFSET = 3;     // a packet's useful data follows its three header bytes
constexpr uint32_t PKT_OVERHEAD = 5;        // header and CRC: useful <= 24 * slots - 5
constexpr uint32_t MAX_USEFUL = 4 * SLOT - PKT_OVERHEAD;   // 91

// MSC data group (clause 5.3.3), the bytes D[0..L) of a run of packets: byte 0 = extension(1) crc(1) segment(1)
// user access(1) type(4), byte 1 = continuity(4) repetition(4); then 2 bytes of extension field, 2 bytes of segment
// field, and the user access field: one byte transport-id flag (bit 4) and length indicator (bits 3..0), then
// `length indicator` bytes, the first two of them the transport id if the flag is set; the group's CRC is its last 2 bytes
constexpr uint32_t DG_EXT = 0x80, DG_CRC = 0x40, DG_SEG = 0x20, DG_UA = 0x10, DG_TYPE_MASK = 15;
constexpr uint32_t DG_FIXED_BYTES = 2, DG_EXT_BYTES = 2, DG_SEG_BYTES = 2, DG_CRC_BYTES = 2;
constexpr uint32_t DG_UA_TIDF = 0x10, DG_UA_LI_MASK = 15, DG_TID_BYTES = 2;
constexpr uint32_t DG_HDR_PEEK = 9;         // no field of the header is read at or behind D[9]
constexpr uint32_t DG_ALIGN = 16;           // a group's bytes start at a multiple of it in d_data
// vit_dgroup_rec.flags
constexpr uint32_t DGF_WELLFORMED = 1, DGF_CRCF = 2, DGF_CRC_OK = 4, DGF_SEG = 8, DGF_UA = 16, DGF_TIDF = 32, DGF_EXT = 64;
constexpr int64_t DG_MAX_SLOTS = 1 << 24;   // of one call: lengths and offsets stay inside 31 bits (91 + 15 bytes a slot)

// FEC frame: application data slots, then FEC packets; FEC packet c starts with {c << 2 | ADDR_FEC >> 8, ADDR_FEC & 255}
constexpr uint32_t FEC_DATA_SLOTS = 94;
constexpr uint32_t FEC_PACKETS = 9;
constexpr uint32_t FEC_SLOTS = FEC_DATA_SLOTS + FEC_PACKETS;   // 103
constexpr uint32_t FEC_FRAME_BYTES = FEC_SLOTS * SLOT;         // 2472
constexpr uint32_t FEC_DATA_BYTES = FEC_DATA_SLOTS * SLOT;     // 2256
constexpr uint32_t FEC_HDR_BYTES = 2;                          // of each FEC packet
constexpr uint32_t FEC_PARITY_PER_PACKET = 22;
constexpr uint32_t FEC_CNT_SHIFT = 2;                          // the counter sits in byte 0 bits 5..2
constexpr uint32_t FEC_HDR1 = ADDR_FEC & 0xFFu;                // 0xFE
__host__ __device__ constexpr uint32_t fec_hdr0(uint32_t c) { return c << FEC_CNT_SHIFT | ADDR_FEC >> 8; }

// the interleaver table and its code: column-wise fill, one RS(204,188) codeword per row
constexpr uint32_t ROWS = 12;
constexpr uint32_t COLS = FEC_DATA_BYTES / ROWS;   // 188
constexpr uint32_t NPAR = 16;                      // g(x) = prod_{i=0..15} (x + alpha^i)
constexpr uint32_t NCODE = COLS + NPAR;            // 204, shortened from 255 by 51 leading zeros
constexpr uint32_t TCORR = NPAR / 2;               // 8
static_assert(ROWS * COLS == FEC_DATA_BYTES && ROWS * NPAR <= FEC_PACKETS * FEC_PARITY_PER_PACKET, "table");
static_assert(FEC_HDR_BYTES + FEC_PARITY_PER_PACKET == SLOT, "FEC packet");

// frame byte of codeword position k of row r (k = 0 ... 187 data column, 188 ... 203 parity byte k - 188)
__host__ __device__ constexpr uint32_t fec_byte(uint32_t r, uint32_t k) {
    return k < COLS ? ROWS * k + r
                    : FEC_DATA_BYTES + SLOT * ((ROWS * (k - COLS) + r) / FEC_PARITY_PER_PACKET) + FEC_HDR_BYTES +
                          (ROWS * (k - COLS) + r) % FEC_PARITY_PER_PACKET;
}

}  // namespace pktfmt
