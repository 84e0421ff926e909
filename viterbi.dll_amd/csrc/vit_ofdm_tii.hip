// vit_ofdm_tii.hip -- transmitter identification from the null symbol (include/viterbi_amd.h, "Transmitter
// identification"): per frame the spectrum of one window, the power of the table's carrier pairs summed over the
// repetitions; per group of navg frames the sum over the frames, the lower median as the noise level, a mask and a strength
// per comb.  Defined bit for bit: every float operation is one IEEE binary32 operation (contraction off, plain operators),
// the transform is the passes of vit_fft_dev.h, every sum is serial in the header's order, the median is a selection.
// Nothing here depends on the launch: no atomics, no scan over the grid.
//
// Two kernels, not one workgroup walking a group's frames.  The spectrum stage is one workgroup's chain per frame (load,
// rotate, log2 nfft stages with their barriers) and wants every frame on a CU of its own: at navg 16 a batch of 512 frames
// would be 32 workgroups on 256 CUs if a workgroup owned a group.  Between the kernels lie Gp*C floats per frame (mode I:
// 768 bytes against the 16 KiB of samples the frame's window holds), in the calling thread's scratch as
// vit_ofdm_acquire_dev keeps its powers.  Both kernels decide by the same function whether a frame is skipped, so the
// second never reads a row the first did not write.
//
//   spectrum  One workgroup per frame, nfft/8 threads (at least 64): step B of vit_ofdm_sync.hip - the thread's 8 samples
//             through the loader of vit_iq_dev.h, the rotation fused into the first pass, twiddles in LDS at twpad().  Then
//             thread T takes the slots (b, c) = T, T + TPB, ...: the 2R points of its pairs from LDS at pad(bin), f in
//             ascending r.  No spectrum reaches memory.
//   group     One workgroup of 256 per group, slots over lanes (at most 4 per lane).  The frames that count are flagged in
//             LDS by the first navg threads; a lane sums its slots over them in ascending t.  The median by rank counting:
//             every lane reads every value (a broadcast read) and the lane whose rank is the wanted one publishes its
//             value.  Then a lane per comb walks its Gp slots in ascending b: mask and strength, no atomics.
#pragma clang fp contract(off)
#include "vit_fft_dev.h"
#include "vit_internal.h"
#include "vit_iq_dev.h"

namespace {

using namespace vit_fft;

// (both stand again in viterbi.dll_amd/__init__.py, TII_GEOMETRY, with the caps of the argument rules - Gp <= 32, navg <= 256,
// R <= 8: the tests take their edges from it)
constexpr u32 GROUP_TPB = 256u;    // navg <= 256: one thread per frame of a group; TII_GEOMETRY["group_threads"]
constexpr u32 SLOTS_MAX = 1024u;   // Gp * C at most: TII_GEOMETRY["slots_max"]

struct TiiArgs {
    const float2* iq;
    u64 nsamples, frame_stride;
    const long long* start;
    long long offset, nframes;
    const float2* tw;
    const float2* nco;
    const uint2* rot;
    u32 nco_shift;  // 32 - nco_bits
    const uint16_t* pairs;
    u32 nfft, Gp, C, R, navg;
    float thr;
    float* slots;  // scratch: row t holds f_t, Gp*C floats
    u32* tii;
    float* energy;
    // integer sample formats: iq then points at samples of iq_fmt (VIT_IQ_CU8 ... VIT_IQ_CS16)
    u32 iq_fmt;
    float iq_scale;
};

// the first sample of frame t's window, or false: the frame is skipped unless start >= 0 and the window is inside
// [0, nsamples).  No sum below can wrap: start >= 0, and offset is added as the two's-complement value it is.
__device__ __forceinline__ bool window_of(const TiiArgs& A, u64 t, u64& w0) {
    const long long s = A.start ? A.start[t] : (long long)(t * A.frame_stride);
    if (s < 0) return false;
    if (A.offset < 0 && (u64)s < 0ull - (u64)A.offset) return false;
    w0 = (u64)s + (u64)A.offset;
    return A.nsamples >= A.nfft && w0 <= A.nsamples - A.nfft;
}

template <u32 M_, bool INT>
__global__ __launch_bounds__(Cfg<M_>::TPB) void vit_tii_spectrum_kernel(TiiArgs A) {
    typedef Cfg<M_> C;
    constexpr u32 N = C::N, TA = C::TA, TPB = C::TPB;
    extern __shared__ float2 lds_tii[];
    static_assert(pad_is_affine(M_), "pad() must skew every thread's group alike");
    float2* tw_lds = lds_tii + C::PADN;
    const u32 T = threadIdx.x;
    const bool active = TPB == TA || T < TA;
    const u64 t = blockIdx.x;
    u64 w0 = 0;
    if (!window_of(A, t, w0)) return;  // uniform over the workgroup
    float2 e1, e3;
    fft_twiddles_to_lds<M_>(tw_lds, A.tw, T, e1, e3);
    if (active) {
        float2 x[8];
        if constexpr (INT) {
            u32 raw[8];
            const char* wi = reinterpret_cast<const char*>(A.iq) + w0 * vit_iq::sample_bytes(A.iq_fmt);
            vit_iq::iq_load_raw<8>(wi, A.iq_fmt, raw, [T](u32 j) { return input_index<M_>(T, j); });
            vit_iq::iq_convert<8>(raw, A.iq_fmt, A.iq_scale, x);
        } else {
            const float2* win = A.iq + w0;
#pragma unroll
            for (u32 j = 0; j < 8; j++) x[j] = win[input_index<M_>(T, j)];
        }
        if (A.rot) {
            const uint2 r = A.rot[t];
            const u32 n0 = (u32)(u64)A.offset;  // n = offset + i mod 2^32, like the phase
#pragma unroll
            for (u32 j = 0; j < 8; j++) {
                const float2 v = x[j];
                const float2 w = A.nco[(r.x + (n0 + input_index<M_>(T, j)) * r.y) >> A.nco_shift];
                x[j] = make_float2(v.x * w.x - v.y * w.y, v.x * w.y + v.y * w.x);
            }
        }
        fft_first_pass<M_>(lds_tii, T, x, e1, e3);
    }
    __syncthreads();  // and the twiddles are in LDS
    fft_radix8_passes<M_>(lds_tii, tw_lds, T, active);

    const u32 GC = A.Gp * A.C;
    float* row = A.slots + t * GC;
    for (u32 sl = T; sl < GC; sl += TPB) {
        float f = 0.f;
        for (u32 r = 0; r < A.R; r++) {
            u32 k = A.pairs[r * GC + sl];
            k = k < N - 2u ? k : N - 2u;
            const float2 a = lds_tii[pad(k)], b = lds_tii[pad(k + 1u)];
            f = f + ((a.x * a.x + a.y * a.y) + (b.x * b.x + b.y * b.y));
        }
        row[sl] = f;
    }
}

__global__ __launch_bounds__(GROUP_TPB) void vit_tii_group_kernel(TiiArgs A) {
    __shared__ float E[SLOTS_MAX];
    __shared__ u32 used[GROUP_TPB];
    __shared__ float noise_lds;
    const u32 T = threadIdx.x;
    const u64 g = blockIdx.x;
    const u32 GC = A.Gp * A.C;
    const u64 t0 = g * A.navg;
    const u32 nt = (u64)A.nframes - t0 < A.navg ? (u32)((u64)A.nframes - t0) : A.navg;
    u64 w0;
    used[T] = T < nt && window_of(A, t0 + T, w0) ? 1u : 0u;
    if (T == 0) noise_lds = 0.f;  // what a group outside the domain (no value of the wanted rank: NaN) decides with
    __syncthreads();
    u32 nused = 0;
    for (u32 i = 0; i < nt; i++) nused += used[i];
    // C: the group's energies, frames in ascending t
    for (u32 sl = T; sl < GC; sl += GROUP_TPB) {
        float acc = 0.f;
        for (u32 i = 0; i < nt; i++)
            if (used[i]) acc = acc + A.slots[(t0 + i) * GC + sl];
        E[sl] = acc;
        if (A.energy) A.energy[g * GC + sl] = acc;
    }
    __syncthreads();
    // D: the lower median.  rank = the values smaller + the equal values of a lower index: a permutation of 0 ... GC-1
    const u32 want = (GC - 1u) / 2u;
    for (u32 sl = T; sl < GC; sl += GROUP_TPB) {
        const float v = E[sl];
        u32 rank = 0;
        for (u32 j = 0; j < GC; j++) {
            const float o = E[j];
            rank += (o < v || (o == v && j < sl)) ? 1u : 0u;
        }
        if (rank == want) noise_lds = v;
    }
    __syncthreads();
    const float noise = noise_lds;
    const float tau = A.thr * noise;
    u32* out = A.tii + g * (2u + 2u * (u64)A.C);
    if (T == 0) {
        out[0] = nused;
        out[1] = __float_as_uint(noise);
    }
    for (u32 c = T; c < A.C; c += GROUP_TPB) {
        u32 mask = 0;
        float strength = 0.f;
        for (u32 b = 0; b < A.Gp; b++) {
            const float v = E[b * A.C + c];
            if (v > 0.f && v >= tau) {
                mask |= 1u << b;
                strength = strength + v;
            }
        }
        out[2u + 2u * c] = mask;
        out[3u + 2u * c] = __float_as_uint(strength);
    }
}

template <u32 M_, bool INT>
hipError_t launch_tii2(const TiiArgs& A, hipStream_t stream) {
    typedef Cfg<M_> C;
    hipError_t e = vit_launch_dynamic_lds<&vit_tii_spectrum_kernel<M_, INT>>((unsigned)A.nframes, C::TPB, C::LDS_BYTES, stream, A);
    if (e != hipSuccess) return e;
    const long long ngrp = (A.nframes + A.navg - 1) / A.navg;
    hipLaunchKernelGGL(vit_tii_group_kernel, dim3((unsigned)ngrp), dim3(GROUP_TPB), 0, stream, A);
    return hipGetLastError();
}

template <u32 M_>
hipError_t launch_tii(const TiiArgs& A, hipStream_t stream) {
    return A.iq_fmt == VIT_IQ_F32 ? launch_tii2<M_, false>(A, stream) : launch_tii2<M_, true>(A, stream);
}

}  // namespace

hipError_t vit_launch_ofdm_tii(const vit_iq_input& in, const vit_iq_format& fmt, const vit_tii_params& p, const uint16_t* d_pairs,
                               int64_t nframes, float* d_slots, uint32_t* d_tii, float* d_energy, hipStream_t stream) {
    if (nframes <= 0) return hipSuccess;
    if (nframes > 0x7FFFFFFFll) return hipErrorInvalidValue;
    static_assert(SLOTS_MAX * 4u + GROUP_TPB * 4u + 64u <= 64u * 1024u, "static LDS");
    TiiArgs A = {};
    A.iq = reinterpret_cast<const float2*>(in.d_iq);
    A.nsamples = in.nsamples;
    A.frame_stride = in.frame_stride;
    A.start = reinterpret_cast<const long long*>(in.d_start);
    A.offset = p.offset;
    A.nframes = nframes;
    A.tw = reinterpret_cast<const float2*>(in.d_tw);
    A.nco = reinterpret_cast<const float2*>(in.d_nco);
    A.rot = reinterpret_cast<const uint2*>(in.d_rot);
    A.nco_shift = in.d_rot ? 32u - in.nco_bits : 0u;
    A.pairs = d_pairs;
    A.nfft = p.nfft;
    A.Gp = p.ngroups;
    A.C = p.ncombs;
    A.R = p.nrep;
    A.navg = p.navg;
    A.thr = p.thr;
    A.slots = d_slots;
    A.tii = d_tii;
    A.energy = d_energy;
    A.iq_fmt = fmt.format;
    A.iq_scale = fmt.scale;
    return for_nfft(p.nfft, [&](auto m) { return launch_tii<decltype(m)::value>(A, stream); });
}
