// vit_iq_dev.h -- the integer sample formats of include/viterbi_amd.h ("Integer sample formats"): the one loader that
// vit_ofdm_td.hip, vit_ofdm_sync.hip and vit_iq_convert.hip share.  Device code only; a TU that includes it turns
// contraction off, so nothing downstream fuses with the multiplication by the scale.
//
// A sample travels in two steps.  iq_load_raw fetches it as it lies in memory into one dword - a 2-byte load for the two
// 8-bit formats (the pair (I, Q) in bits 0 ... 15; any sample position is 2-byte aligned because d_iq is 4-byte aligned),
// a 4-byte load for CS16 - and reads no byte of any other sample.  iq_convert turns the dword into the float2 of the
// definition: one exact conversion per component and one multiplication, the only rounding.  The kernels keep prefetched
// samples raw (a dword instead of a float2) and convert where they consume them.  The format is uniform over a launch:
// the switches below are scalar branches, written around the loops over a thread's samples.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "viterbi_amd.h"

namespace vit_iq {

typedef uint32_t u32;
typedef uint64_t u64;

// bytes of one complex sample
__host__ __device__ constexpr u32 sample_bytes(u32 fmt) { return fmt == VIT_IQ_F32 ? 8u : fmt == VIT_IQ_CS16 ? 4u : 2u; }

// NS samples at the sample indices idx(j) behind s0, as they lie in memory
template <u32 NS, class Idx>
__device__ __forceinline__ void iq_load_raw(const void* s0, u32 fmt, u32 (&raw)[NS], Idx idx) {
    if (fmt == VIT_IQ_CS16) {
#pragma unroll
        for (u32 j = 0; j < NS; j++) raw[j] = reinterpret_cast<const u32*>(s0)[idx(j)];
    } else {
#pragma unroll
        for (u32 j = 0; j < NS; j++) raw[j] = reinterpret_cast<const uint16_t*>(s0)[idx(j)];
    }
}

// CU8: 2b - 255 is formed in binary32 from the exact (float)b - every step is an integer of magnitude <= 255, so the
// fused multiply-add rounds nothing - and meets the scale in the definition's one rounding
__device__ __forceinline__ float cu8(u32 b, float scale) { return __builtin_fmaf((float)b, 2.0f, -255.0f) * scale; }

template <u32 NS>
__device__ __forceinline__ void iq_convert(const u32 (&raw)[NS], u32 fmt, float scale, float2 (&x)[NS]) {
    if (fmt == VIT_IQ_CU8) {
#pragma unroll
        for (u32 j = 0; j < NS; j++) x[j] = make_float2(cu8(raw[j] & 0xFFu, scale), cu8(raw[j] >> 8 & 0xFFu, scale));
    } else if (fmt == VIT_IQ_CS8) {
#pragma unroll
        for (u32 j = 0; j < NS; j++)
            x[j] = make_float2((float)(int)(int8_t)raw[j] * scale, (float)(int)(int8_t)(raw[j] >> 8) * scale);
    } else {
#pragma unroll
        for (u32 j = 0; j < NS; j++)
            x[j] = make_float2((float)(int)(int16_t)raw[j] * scale, (float)((int)raw[j] >> 16) * scale);
    }
}

}  // namespace vit_iq
