// vit_image_dev.h -- a run of bytes at any address into LDS with aligned 16-byte loads, and a lane's bytes out of that
// image: the staging steps that the packet units (vit_packet_dev.h: logical frames, FEC frames) and the FIB group units
// (vit_fib_group_dev.h: FIBs) share.
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

// The 4 * (NDW - 1) bytes at byte `base` of an LDS image into row[0 ... NDW-2]: NDW aligned dwords, one v_alignbyte per
// dword, so the image holds a dword past the last byte taken.  (pkt_wave_records in vit_packet_dev.h keeps a sibling of
// these lines, seven dwords into registers: through this routine its two kernels' instructions came out in another order.)
template <uint32_t NDW>
__device__ __forceinline__ void image_row(const uint8_t* s, uint32_t base, uint32_t* row) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(s + (base & ~3u));
    uint32_t d[NDW];
#pragma unroll
    for (uint32_t k = 0; k < NDW; k++) d[k] = q[k];
#pragma unroll
    for (uint32_t k = 0; k < NDW - 1u; k++) row[k] = __builtin_amdgcn_alignbyte(d[k + 1u], d[k], base & 3u);
}
