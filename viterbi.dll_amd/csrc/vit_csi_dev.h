// vit_csi_dev.h -- the per-symbol soft-decision rule of include/viterbi_amd.h ("Channel-state weighting",
// VIT_SOFT_PER_SYMBOL), shared by the two demappers: vit_ofdm.hip and vit_ofdm_td.hip.  Device code only; a TU that
// includes it turns contraction off.
//
// A symbol's level S is a long sum of the synchroniser's shape: A = max(64, nfft/8) accumulators, one per thread, each
// the sum of its groups of 4 carriers, meet in the tree of adjacent pairs (vit_wave_dev.h): vit_wave::wave_sum inside a
// wavefront, then the wavefronts' totals through CSI_PARTS words of LDS, where every thread reads them all (broadcast
// reads) and finishes the tree itself with vit_wave::pair_tree<TPB / 64>, so the scale needs no second exchange.  A
// wavefront that holds no accumulator (the demapper's workgroup may be larger than A) leaves the +0 its word starts
// with: x + 0 = x for the non-negative totals, so the tree over the workgroup's wavefronts is the tree over A/64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cfloat>

#include "vit_wave_dev.h"

namespace vit_csi {

typedef uint32_t u32;
constexpr u32 CSI_PARTS = 16;  // wavefronts of the largest workgroup (nfft 8192: 1024 accumulators)

// a carrier's term of the sum: nrm, or +0 for an erasure (no signal, NaN, Inf)
__device__ __forceinline__ float csi_term(float nrm) {
    return (nrm >= 0x1p-64f && nrm <= FLT_MAX) ? nrm : 0.0f;  // false for NaN
}

// q[g] of the header: the group's four terms in adjacent pairs
__device__ __forceinline__ float csi_group(float v0, float v1, float v2, float v3) { return (v0 + v1) + (v2 + v3); }

// s of the header, or 0 for a symbol that is all erasures (S outside [2^-64, 2^96], Inf included; S is never NaN)
__device__ __forceinline__ float csi_scale(float S, float gain, u32 K) {
    return (S >= 0x1p-64f && S <= 0x1p96f) ? (gain * (float)K) / S : 0.0f;
}

// The two soft bytes of a carrier (low byte: bit n).  An erased carrier arrives with re = im = 0 and an erased symbol
// with s = 0: both give 128 - rint(+-0) = 128 (re and im of a carrier that is no erasure are finite).
__device__ __forceinline__ u32 csi_pair(float re, float im, float s) {
    const float q0 = __builtin_fminf(__builtin_fmaxf(128.0f - __builtin_rintf(re * s), 0.0f), 255.0f);
    const float q1 = __builtin_fminf(__builtin_fmaxf(128.0f - __builtin_rintf(im * s), 0.0f), 255.0f);
    return (u32)q0 | (u32)q1 << 8;
}

}  // namespace vit_csi
