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
