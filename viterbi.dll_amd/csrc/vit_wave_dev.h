// vit_wave_dev.h -- the tree of adjacent pairs, the grouping of every long binary32 sum of include/viterbi_amd.h, for the
// kernels that take it across a wavefront's lanes or over a few registers or LDS words: the demappers' symbol level
// (vit_csi_dev.h), the synchroniser's sums (vit_ofdm_sync.hip) and the block powers (vit_ofdm_acq.hip).  Device code
// only; a TU that includes it turns contraction off.
//
// Across lanes the tree is the butterfly over lane distances 1 ... 32: binary32 addition commutes, so lane L's
// v[L] + v[L ^ h] is the tree's node bit for bit, and after level k every lane of an aligned group of 2 << k holds the
// group's sum.  Distances 1 ... 8 are DPP operands of the addition - the mirrors fetch what lane ^ 4 and lane ^ 8 hold
// because the levels below have made the lanes of a group alike; 16 and 32 cross DPP rows and go through the LDS
// crossbar (ds_bpermute).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vit_wave {

template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
    return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}

// v + the value of the lane `1 << level` away, level 0 ... 5, the levels below it taken before; every lane of the
// wavefront must be active
__device__ __forceinline__ float xor_add(float v, uint32_t level) {
    switch (level) {
        case 0: return dpp_add<0xB1>(v);   // quad_perm [1, 0, 3, 2]
        case 1: return dpp_add<0x4E>(v);   // quad_perm [2, 3, 0, 1]
        case 2: return dpp_add<0x141>(v);  // row_half_mirror
        case 3: return dpp_add<0x140>(v);  // row_mirror
        case 4: return v + __shfl_xor(v, 16);
        default: return v + __shfl_xor(v, 32);
    }
}

// the tree over the 64 lanes' values: every lane ends with the wavefront's total
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (uint32_t level = 0; level < 6u; level++) v = xor_add(v, level);
    return v;
}

// the tree over the N values p[0], p[stride], ... (registers or LDS words)
template <uint32_t N>
__device__ __forceinline__ float pair_tree(const float* p, uint32_t stride = 1u) {
    static_assert(N >= 1 && (N & (N - 1u)) == 0, "a power of two");
    float u[N];
#pragma unroll
    for (uint32_t i = 0; i < N; i++) u[i] = p[i * stride];
#pragma unroll
    for (uint32_t h = 1; h < N; h *= 2)
#pragma unroll
        for (uint32_t i = 0; i < N; i += 2u * h) u[i] = u[i] + u[i + h];
    return u[0];
}

}  // namespace vit_wave
