// vit_fft_dev.h -- the in-LDS FFT of include/viterbi_amd.h ("From the samples", step 2), shared by the kernels that
// transform a symbol inside a workgroup: vit_ofdm_td.hip (every symbol of a frame), vit_ofdm_sync.hip (the phase
// reference symbol and the channel impulse response) and vit_ofdm_tii.hip (the null symbol).  Device code, and the hosts'
// choice of the instantiation (for_nfft); a TU that includes it turns contraction off.
//
// A symbol's FFT lives in LDS as nfft padded float2.  A thread owns 8 points of every pass (nfft/8 threads work on a
// symbol; at nfft < 512 the rest of the 64 idle in the FFT).  The stages are grouped into passes of 3 (radix-8 in
// registers), preceded by one pass of m mod 3 stages:
//   first pass   straight from registers: thread T holds inputs T + c*nfft/R, which bit reversal makes the R consecutive
//                points of group bitrev(T); stages 1 ... log2 R, one LDS store per point (fft_first_pass);
//   other passes 8 LDS loads at stride 2^s, 3 stages, 8 LDS stores in place, a barrier (fft_radix8_passes).
// The butterflies are the header's radix-2 decimation-in-time graph with the header's twiddles; only the multiplications
// by the exact twiddles 1 and -j of stages 1 and 2 are skipped (the header's domain makes that free).
// vit_ofdm_td.hip keeps both pass loops written out in its kernel, with the rotation fused into the first
// (profiles/r19_front_isa_same.txt).  As a call, fft_radix8_passes costs six of its 96 instantiations scratch at their
// 128 VGPRs - mode I's own (nfft 2048, float32, no rotation, per-carrier rule) 0 -> 12 bytes and 114 -> 128 VGPRs, the
// per-symbol rule's at nfft 1024 ... 4096 12 -> 20, two at nfft 8192 124 -> 132 and 100 -> 108.  fft_first_pass on the
// rotated samples keeps every instantiation's resources, but together with the soft bytes' destination as a function the
// per-symbol kernel of the integer formats took 0.2 - 0.3 % longer, and half of the instantiations are the parent's code
// instruction for instruction with the two written out.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace vit_fft {

typedef uint32_t u32;
typedef uint64_t u64;

// LDS index of point i.  Rows of 32 points are skewed by 4, rows of 256 by 1 more: the strided loads of the passes
// (stride 2^s points between a thread's own, consecutive or 8 << s apart between lanes) and the bit-reversed stores of
// the first pass (2^(m-5) apart between lanes) then spread over the 32 eight-byte bank pairs.
constexpr u32 pad(u32 i) { return i + ((i >> 5) << 2) + (i >> 8); }
// Point q of a thread's group in the pass behind s stages is base + (q << s), base = pass_base(T, s).  Its LDS index is
// pad(base) + pad(q << s): the skew of a group's points does not depend on the thread, so one address register and
// immediate offsets serve a pass (pad_is_affine checks it for every thread at compile time).
constexpr u32 pass_base(u32 T, u32 s) { return ((T >> s) << (s + 3u)) + (T & ((1u << s) - 1u)); }
constexpr bool pad_is_affine(u32 M) {
    const u32 R1 = M % 3u ? M % 3u : 3u;
    for (u32 s = R1; s < M; s += 3u)
        for (u32 T = 0; T < (1u << M) / 8u; T++)
            for (u32 q = 0; q < 8u; q++)
                if (pad(pass_base(T, s) + (q << s)) != pad(pass_base(T, s)) + pad(q << s)) return false;
    for (u32 i = 0; i < (1u << M); i++)  // the first pass stores aligned groups of at most 8 consecutive points
        if (pad(i) != pad(i & ~7u) + (i & 7u)) return false;
    return true;
}

template <u32 M>
struct Cfg {
    static constexpr u32 N = 1u << M;
    static constexpr u32 TA = N / 8u;                  // threads that work on a symbol
    static constexpr u32 TPB = TA < 64u ? 64u : TA;
    static constexpr u32 R1 = M % 3u ? M % 3u : 3u;    // stages of the first pass
    static constexpr u32 NP = (M - R1) / 3u;           // radix-8 passes behind it
    // wavefronts per SIMD the registers are budgeted for: with rotation the prefetched phasors take 16 more (a workgroup
    // of 1024 needs 4 in any case)
    static constexpr u32 waves(bool rot) { return TPB == 1024u ? 4u : rot ? 3u : 4u; }
    static constexpr u32 PADN = pad(N - 1u) + 1u;       // float2 of LDS for a symbol, then twpad(N/2 - 1) + 1 twiddles
    static constexpr u32 LDS_BYTES = (PADN + N / 2u + N / 64u) * 8u;
    static constexpr u32 CG = 2u;                      // groups of 4 carriers per thread: K <= N = 8 TA
};

__device__ __forceinline__ void bfly(float2& u, float2& v, float2 w) {
    const float tr = w.x * v.x - w.y * v.y;
    const float ti = w.x * v.y + w.y * v.x;
    const float2 a = u;
    u = make_float2(a.x + tr, a.y + ti);
    v = make_float2(a.x - tr, a.y - ti);
}
__device__ __forceinline__ void bfly_one(float2& u, float2& v) {  // w = 1
    const float2 a = u, t = v;
    u = make_float2(a.x + t.x, a.y + t.y);
    v = make_float2(a.x - t.x, a.y - t.y);
}
__device__ __forceinline__ void bfly_mj(float2& u, float2& v) {  // w = -j: t = (v.im, -v.re)
    const float2 a = u, t = v;
    u = make_float2(a.x + t.y, a.y - t.x);
    v = make_float2(a.x - t.y, a.y + t.x);
}

// 3 stages on 8 points; w[h - 1 + jq]: the twiddle of stage h = 1, 2, 4 for the points q with q mod h = jq
__device__ __forceinline__ void radix8(float2 (&v)[8], const float2 (&w)[7]) {
#pragma unroll
    for (u32 h = 1; h < 8; h *= 2)
#pragma unroll
        for (u32 q = 0; q < 8; q++)
            if (!(q & h)) bfly(v[q], v[q + h], w[h - 1 + (q & (h - 1))]);
}

// stages 1 ... R1 on the 2^R1 points of one group of the first pass; e1, e3: the twiddles at 1/8 and 3/8 of a half turn
template <u32 R1>
__device__ __forceinline__ void first_stages(float2* v, float2 e1, float2 e3) {
#pragma unroll
    for (u32 q = 0; q < (1u << R1); q += 2) bfly_one(v[q], v[q + 1]);
    if (R1 >= 2) {
#pragma unroll
        for (u32 q = 0; q < (1u << R1); q += 4) {
            bfly_one(v[q], v[q + 2]);
            bfly_mj(v[q + 1], v[q + 3]);
        }
    }
    if (R1 >= 3) {
        bfly_one(v[0], v[4]);
        bfly(v[1], v[5], e1);
        bfly_mj(v[2], v[6]);
        bfly(v[3], v[7], e3);
    }
}

constexpr u32 bitrev(u32 x, u32 bits) {
    u32 r = 0;
    for (u32 b = 0; b < bits; b++) r |= (x >> b & 1u) << (bits - 1u - b);
    return r;
}

// LDS index of twiddle k: the lanes of a pass read twiddles a power of two apart
constexpr u32 twpad(u32 k) { return k + (k >> 5); }

// The workgroup's copy of the table tw (N/2 twiddles) to tw_lds at twpad() - the caller puts a barrier in front of the
// radix-8 passes - and the two twiddles first_stages needs, e1 and e3, for thread T of Cfg<M>::TPB.  A thread's 7
// twiddles per pass are the same for every symbol, but 21 or 28 float2 of registers cost more occupancy than their loads
// cost LDS cycles.
template <u32 M>
__device__ __forceinline__ void fft_twiddles_to_lds(float2* tw_lds, const float2* tw, u32 T, float2& e1, float2& e3) {
    typedef Cfg<M> C;
    for (u32 i = T; i < C::N / 2u; i += C::TPB) tw_lds[twpad(i)] = tw[i];
    e1 = e3 = make_float2(1.f, 0.f);
    if (C::R1 == 3) {
        e1 = tw[C::N / 8u];
        e3 = tw[3u * C::N / 8u];
    }
}

// the 7 twiddles of thread T's group in the pass behind s stages, in radix8's order, from the LDS copy of the table
template <u32 M>
__device__ __forceinline__ void load_twiddles(const float2* tw, u32 T, u32 s, float2 (&w)[7]) {
    const u32 j0 = T & ((1u << s) - 1u);
#pragma unroll
    for (u32 a = 0; a < 3; a++)
#pragma unroll
        for (u32 jq = 0; jq < (1u << a); jq++) w[(1u << a) - 1u + jq] = tw[twpad((j0 + (jq << s)) * ((1u << M) >> (s + a + 1u)))];
}

// input i of the transform that thread T (< TA) holds in slot j of its 8: group k = j / R of the first pass is
// T + k*TA, its point c = j % R is input gid + c*N/R
template <u32 M>
constexpr u32 input_index(u32 T, u32 j) {
    constexpr u32 R = 1u << Cfg<M>::R1;
    return T + (j / R) * Cfg<M>::TA + (j % R) * (Cfg<M>::N / R);
}

// The first pass of thread T (< TA) from its 8 inputs x[j] = input input_index(T, j): stages 1 ... R1, stored to the
// symbol's LDS.  The caller puts a barrier behind it.
template <u32 M>
__device__ __forceinline__ void fft_first_pass(float2* lds, u32 T, const float2 (&x)[8], float2 e1, float2 e3) {
    typedef Cfg<M> C;
    constexpr u32 R1 = C::R1, R = 1u << R1;
#pragma unroll
    for (u32 k = 0; k < 8u / R; k++) {
        float2 v[R];
#pragma unroll
        for (u32 c = 0; c < R; c++) v[bitrev(c, R1)] = x[k * R + c];
        first_stages<R1>(v, e1, e3);
        float2* g = lds + pad(R * (__builtin_bitreverse32(T + k * C::TA) >> (32u - (M - R1))));
#pragma unroll
        for (u32 q = 0; q < R; q++) g[q] = v[q];
    }
}

// The radix-8 passes behind the first one, each followed by a barrier: every thread of the workgroup calls it, those
// with `active` (T < TA) work.  tw_lds: the twiddle table at twpad().
template <u32 M>
__device__ __forceinline__ void fft_radix8_passes(float2* lds, const float2* tw_lds, u32 T, bool active) {
    typedef Cfg<M> C;
#pragma unroll
    for (u32 p = 0; p < C::NP; p++) {
        if (active) {
            const u32 s = C::R1 + 3u * p;
            float2* g = lds + pad(pass_base(T, s));
            float2 v[8];
#pragma unroll
            for (u32 q = 0; q < 8; q++) v[q] = g[pad(q << s)];
            float2 w[7];
            load_twiddles<M>(tw_lds, T, s, w);
            radix8(v, w);
#pragma unroll
            for (u32 q = 0; q < 8; q++) g[pad(q << s)] = v[q];
        }
        __syncthreads();
    }
}

// Host side: f(std::integral_constant<u32, M>()) for the transform length nfft = 2^M that has a Cfg<M>
template <typename F>
hipError_t for_nfft(u32 nfft, F&& f) {
    switch (nfft) {
        case 64: return f(std::integral_constant<u32, 6>());
        case 128: return f(std::integral_constant<u32, 7>());
        case 256: return f(std::integral_constant<u32, 8>());
        case 512: return f(std::integral_constant<u32, 9>());
        case 1024: return f(std::integral_constant<u32, 10>());
        case 2048: return f(std::integral_constant<u32, 11>());
        case 4096: return f(std::integral_constant<u32, 12>());
        case 8192: return f(std::integral_constant<u32, 13>());
    }
    return hipErrorInvalidValue;
}

}  // namespace vit_fft
