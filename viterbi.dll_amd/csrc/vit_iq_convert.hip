// vit_iq_convert.hip -- integer samples to the floats of the definition (include/viterbi_amd.h, "Integer sample formats"),
// for callers who need the floats themselves.  A streaming kernel: a thread owns one 16-byte aligned chunk of the input
// (8 samples of an 8-bit format, 4 of CS16), loads it whole and stores its 16 or 8 floats in 16-byte pieces where the
// output lies that way (d_out is 8-byte aligned: whether a chunk's floats start on 16 bytes is the same for every whole
// chunk of a call), in 8-byte pieces otherwise.  The chunks at the two ends that the samples fill only in part go sample
// by sample through the loader of vit_iq_dev.h, so no byte outside the samples is read.
#pragma clang fp contract(off)
#include "vit_internal.h"
#include "vit_iq_dev.h"

namespace {

using vit_iq::u32;
using vit_iq::u64;

constexpr u32 CONVERT_TPB = 256u;

template <u32 FMT>
__device__ __forceinline__ void convert_chunk(const char* iq, u64 nsamples, u64 head, u64 chunk, float scale, float* out) {
    constexpr u32 SB = vit_iq::sample_bytes(FMT), SPC = 16u / SB;  // samples per chunk
    // chunk q holds the samples q*SPC - head ... + SPC - 1; head < SPC samples of chunk 0 lie in front of d_iq
    const u64 first = chunk * SPC;
    const u64 lo = first < head ? 0 : first - head;
    const u64 hi = first + SPC - head < nsamples ? first + SPC - head : nsamples;
    if (hi - lo == SPC) {
        const uint4 v = *reinterpret_cast<const uint4*>(iq + lo * SB);
        const u32 d[4] = {v.x, v.y, v.z, v.w};
        u32 raw[SPC];
#pragma unroll
        for (u32 j = 0; j < SPC; j++) {
            const u32 w = d[SB == 4u ? j : j / 2u];
            raw[j] = SB == 4u ? w : (w >> (16u * (j & 1u))) & 0xFFFFu;
        }
        float2 x[SPC];
        vit_iq::iq_convert<SPC>(raw, FMT, scale, x);
        float* o = out + 2u * lo;
        if ((reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
#pragma unroll
            for (u32 j = 0; j < SPC; j += 2) reinterpret_cast<float4*>(o)[j / 2u] = make_float4(x[j].x, x[j].y, x[j + 1].x, x[j + 1].y);
        } else {
#pragma unroll
            for (u32 j = 0; j < SPC; j++) reinterpret_cast<float2*>(o)[j] = x[j];
        }
        return;
    }
    for (u64 s = lo; s < hi; s++) {
        u32 raw[1];
        float2 x[1];
        vit_iq::iq_load_raw<1>(iq, FMT, raw, [s](u32) { return s; });
        vit_iq::iq_convert<1>(raw, FMT, scale, x);
        reinterpret_cast<float2*>(out)[s] = x[0];
    }
}

__global__ __launch_bounds__(CONVERT_TPB) void vit_iq_convert_kernel(const char* iq, u32 fmt, float scale, u64 nsamples, u64 head,
                                                                     u64 chunks, float* out) {
    const u64 chunk = (u64)blockIdx.x * CONVERT_TPB + threadIdx.x;
    if (chunk >= chunks) return;
    if (fmt == VIT_IQ_CU8) convert_chunk<VIT_IQ_CU8>(iq, nsamples, head, chunk, scale, out);
    else if (fmt == VIT_IQ_CS8) convert_chunk<VIT_IQ_CS8>(iq, nsamples, head, chunk, scale, out);
    else convert_chunk<VIT_IQ_CS16>(iq, nsamples, head, chunk, scale, out);
}

}  // namespace

hipError_t vit_launch_iq_convert(const void* d_iq, const vit_iq_format& fmt, uint64_t nsamples, float* d_out, hipStream_t stream) {
    if (nsamples == 0) return hipSuccess;
    const u32 sb = vit_iq::sample_bytes(fmt.format), spc = 16u / sb;
    const u64 head = (u64)(reinterpret_cast<uintptr_t>(d_iq) & 15u) / sb;  // d_iq is 4-byte aligned: whole samples
    if (nsamples > UINT64_MAX - head - spc) return hipErrorInvalidValue;
    const u64 chunks = (head + nsamples + spc - 1u) / spc;
    const u64 grid = (chunks + CONVERT_TPB - 1u) / CONVERT_TPB;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vit_iq_convert_kernel, dim3((unsigned)grid), dim3(CONVERT_TPB), 0, stream,
                       static_cast<const char*>(d_iq), fmt.format, fmt.scale, nsamples, head, chunks, d_out);
    return hipGetLastError();
}
