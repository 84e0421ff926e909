// vit_punct_dev.h -- device helpers of the depuncturing expansion, shared by vit_punct.hip and vit_ti.hip: a profile's
// segment table, the step -> (first transmitted byte, keep nibble) lookup and the v_perm_b32 selector of a keep nibble.
#pragma once
#include "vit_internal.h"

namespace {

// Segment table of one profile: first step and first transmitted byte of every segment.  The uniform call computes it
// on the host and passes it by value; the varlen kernel builds it per frame from the caller's device profile.
struct SegTab {
    uint32_t nsegs;
    uint32_t start[VIT_PUNCT_MAX_SEGS];
    uint32_t base[VIT_PUNCT_MAX_SEGS];
    uint32_t keep[VIT_PUNCT_MAX_SEGS];
};

// v_perm_b32 selector that expands the packed transmitted bytes of a step with keep nibble `nib`: byte j takes packed
// byte popc(nib & ((1 << j) - 1)) if symbol j is transmitted, else selector 4 = byte 0 of the erasure word (src0)
__device__ __forceinline__ uint32_t expand_sel(uint32_t nib) {
    uint32_t sel = 0, r = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        const uint32_t bit = (nib >> j) & 1u;
        sel |= (bit ? r : 4u) << (8u * j);
        r += bit;
    }
    return sel;
}

// Segment lookup of frame-local step t: first transmitted byte and keep nibble
__device__ __forceinline__ void locate(uint32_t t, const SegTab& tab, uint32_t& off, uint32_t& nib) {
    uint32_t s0 = tab.start[0], b0 = tab.base[0], keep = tab.keep[0];
#pragma unroll
    for (uint32_t k = 1; k < VIT_PUNCT_MAX_SEGS; k++) {  // segments start in increasing order: the last one at or below t
        if (k < tab.nsegs && t >= tab.start[k]) {
            s0 = tab.start[k];
            b0 = tab.base[k];
            keep = tab.keep[k];
        }
    }
    const uint32_t k = t - s0, ph = 4u * (k & 7u);
    off = b0 + (k >> 3) * __builtin_popcount(keep) + __builtin_popcount(keep & ((1u << ph) - 1u));
    nib = (keep >> ph) & 15u;
}

}  // namespace
