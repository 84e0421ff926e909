// vit_image_dev.h -- a run of bytes at any address into LDS with aligned 16-byte loads: the staging step that
// vit_packet.hip (logical frames, FEC frames) and vit_mci.hip (FIBs) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// n bytes at p into an LDS image that keeps p's phase in 16 bytes: byte k at s[(p & 15) + k].  `nthreads` threads call
// it with t = 0 ... nthreads-1.  Whole aligned windows inside [p, p + n) are one 16-byte load each; the two edge windows
// go byte by byte, so nothing outside the n bytes is read.  s is 16-byte aligned and holds ((p & 15) + n + 15) & ~15 bytes.
__device__ __forceinline__ void load_image(const uint8_t* p, uint32_t n, uint8_t* s, uint32_t t, uint32_t nthreads) {
    const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u);
    const uint32_t nwin = (a + n + 15u) >> 4;
    for (uint32_t w = t; w < nwin; w += nthreads) {
        const int o = (int)(16u * w) - (int)a;
        if (o >= 0 && (uint32_t)o + 16u <= n) {
            *reinterpret_cast<uint4*>(s + 16u * w) = *reinterpret_cast<const uint4*>(p + o);
        } else {
            for (uint32_t j = 0; j < 16u; j++) {
                const int k = o + (int)j;
                if (k >= 0 && (uint32_t)k < n) s[16u * w + j] = p[k];
            }
        }
    }
}
