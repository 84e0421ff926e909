// vit_crc_dev.h -- the byte step of the FIB CRC-16 (0x1021, MSB first), shared by the units that run it without a table:
// the access units (vit_dab.hip) and the packets (vit_packet.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// CRC-16 0x1021 over one byte without a table: crc * x^8 + b * x^16 mod g
__host__ __device__ constexpr uint32_t crc16_step(uint32_t crc, uint32_t b) {
    uint32_t x = ((crc >> 8) ^ b) & 0xFFu;
    x ^= x >> 4;
    return ((crc << 8) ^ (x << 12) ^ (x << 5) ^ x) & 0xFFFFu;
}
