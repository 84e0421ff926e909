// vit_crc_dev.h -- the FIB CRC-16 (0x1021, MSB first) for the units that run it without a table: its byte step (the access
// units of vit_dab.hip, the packets of vit_packet.hip, the data groups of vit_dgroup.hip) and the arithmetic mod g that
// combines remainders of pieces (packets and data groups).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// CRC-16 0x1021 over one byte without a table: crc * x^8 + b * x^16 mod g
__host__ __device__ constexpr uint32_t crc16_step(uint32_t crc, uint32_t b) {
    uint32_t x = ((crc >> 8) ^ b) & 0xFFu;
    x ^= x >> 4;
    return ((crc << 8) ^ (x << 12) ^ (x << 5) ^ x) & 0xFFFFu;
}

// r * x^(8e) mod g
constexpr uint32_t crc_xpow(uint32_t e, uint32_t r) {
    for (uint32_t k = 0; k < e; k++) r = crc16_step(r, 0);
    return r;
}

// r * x mod g for the constant x: the 31-bit carry-less product, its upper half taken through two zero bytes
template <uint32_t X>
__device__ __forceinline__ uint32_t crc_mul(uint32_t r) {
    uint32_t prod = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16u; j++)
        if ((X >> j) & 1u) prod ^= r << j;
    return (prod & 0xFFFFu) ^ crc16_step(crc16_step(prod >> 16, 0), 0);
}

// a * b mod g for two 16-bit values, neither a constant
__host__ __device__ inline uint32_t crc_mulg(uint32_t a, uint32_t b) {
    uint32_t prod = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16u; j++) prod ^= (b >> j) & 1u ? a << j : 0u;
    return (prod & 0xFFFFu) ^ crc16_step(crc16_step(prod >> 16, 0), 0);
}
