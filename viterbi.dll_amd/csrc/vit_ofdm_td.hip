// vit_ofdm_td.hip -- from the samples to soft bytes (include/viterbi_amd.h, "From the samples"): fine-frequency rotation,
// the FFT of every OFDM symbol and, fused behind it, exactly the demapping of vit_ofdm.hip - no spectrum goes through
// memory (vit_ofdm_demod_dev) - or the spectra themselves in the layout vit_ofdm_demap_dev reads (vit_ofdm_fft_dev).
//
// The result is defined bit for bit: every float operation is one IEEE binary32 operation (contraction off, plain
// operators), the butterflies are the header's radix-2 decimation-in-time graph with the header's twiddles.  Only the
// multiplications by the exact twiddles 1 and -j of stages 1 and 2 are skipped (the header's domain makes that free).
//
// One workgroup owns one frame and a run of consecutive symbols; a symbol's FFT lives in LDS as nfft padded float2.
// A thread owns 8 points of every pass (nfft/8 threads work on a symbol; at nfft < 512 the rest of the 64 idle in the
// FFT).  The stages are grouped into passes of 3 (radix-8 in registers), preceded by one pass of m mod 3 stages:
//   first pass   straight from the sample registers: thread T holds samples T + c*nfft/R, which bit reversal makes the
//                R consecutive points of group bitrev(T); rotation, stages 1 ... log2 R, one LDS store per point;
//   other passes 8 LDS loads at stride 2^s, 3 stages, 8 LDS stores in place, a barrier.
// Both pass loops are written out here, with the rotation fused into the first: vit_fft_dev.h has them as functions
// and the measured reason.
// The twiddle table is copied to LDS behind the symbol once per workgroup and a thread loads its 7 twiddles per radix-8
// pass from there: they are the same for every symbol, but kept in registers (21 float2 at nfft 2048) they cost a
// wavefront per SIMD, which costs more than the loads.  The next symbol's samples (and phasors) are loaded right after
// the first pass has consumed this symbol's: they are in flight during the other passes, the barriers and the outputs.
// Demapping: carrier n reads bin d_bins[n] of the LDS spectrum; a thread owns fixed groups of 4 consecutive n, keeps
// their bins and the previous symbol's values in registers and stores 4 + 4 soft bytes per group (any alignment).  A run
// starts by transforming the symbol before it: 1/run of redundant work.
// Integer sample formats (vit_iq_dev.h): one template flag apart from the float32 instantiations, which pay nothing for
// them.  The prefetched samples are then kept raw, 8 dwords instead of 16, and converted where the first pass consumes
// them; the three formats share an instantiation and part in two scalar branches of the loader.
// The per-symbol soft-decision rule (VIT_SOFT_PER_SYMBOL, vit_csi_dev.h): one more template flag, of which the other
// instantiations hold no code.  The thread's groups T + j*TPB are the header's groups of accumulator T (TPB = max(64, nfft/8)), so
// it keeps re and im of its 8 carriers, sums their terms, the workgroup reduces (DPP inside a wavefront, one LDS exchange
// and one barrier across them, CSI_PARTS floats behind the twiddles) and every thread quantises with the symbol's scale.
#pragma clang fp contract(off)
#include <cmath>

#include "vit_demap_dev.h"
#include "vit_fft_dev.h"
#include "vit_iq_dev.h"

namespace {

using namespace vit_fft;
using namespace vit_demap;

struct TdArgs {
    const float2* iq;
    u64 nsamples, sym_stride, frame_stride, extent;  // extent: samples from a frame's start to its last read, + 1
    const long long* start;
    const float2* tw;
    const float2* nco;
    const uint2* rot;
    u32 nco_shift;  // 32 - nco_bits
    u32 lo, hi;     // the symbols (FFT) or data symbols (demod) [lo, hi) of every frame are produced
    u32 run, runs;  // of them per workgroup, workgroups per frame
    // spectra out
    float2* out;
    u64 out_sym_stride, out_frame_stride;
    // demapping
    const uint16_t* bins;
    u32 K, fic_syms, cifs, per;
    float gain;
    uint8_t* fic;
    uint8_t* ring;
    u64 row_bytes, nrows, first_row, col;
    // integer sample formats: iq then points at samples of iq_fmt (VIT_IQ_CU8 ... VIT_IQ_CS16)
    u32 iq_fmt;
    float iq_scale;
    // the per-symbol rule: d_level or nullptr, its words per frame (nsyms - 1)
    float* level;
    u32 nlev, csi;  // csi: host side only, picks the instantiation
};

template <u32 M, bool ROT, bool INT>
struct Samples {
    float2 x[INT ? 1 : 8];
    u32 raw[INT ? 8 : 1];  // integer formats: as they lie in memory, converted by the first pass
    float2 w[ROT ? 8 : 1];
};

// symbol l's samples of thread T: group k of the first pass is T + k*TA, its point c is sample gid + c*N/R
template <u32 M, bool ROT, bool INT>
__device__ __forceinline__ void load_samples(const TdArgs& A, const void* frame, u32 l, u32 ph0, u32 step, u32 T,
                                             Samples<M, ROT, INT>& s) {
    typedef Cfg<M> C;
    constexpr u32 R = 1u << C::R1, NG = C::N / R;
    const u32 n0 = (u32)((u64)l * A.sym_stride);  // mod 2^32, like the phase
    if constexpr (INT) {
        const char* sym = static_cast<const char*>(frame) + (u64)l * A.sym_stride * vit_iq::sample_bytes(A.iq_fmt);
        vit_iq::iq_load_raw<8>(sym, A.iq_fmt, s.raw, [T](u32 j) { return input_index<M>(T, j); });
        if (ROT) {
#pragma unroll
            for (u32 j = 0; j < 8; j++) s.w[j] = A.nco[(ph0 + (n0 + input_index<M>(T, j)) * step) >> A.nco_shift];
        }
        return;
    }
    const float2* sym = static_cast<const float2*>(frame) + (u64)l * A.sym_stride;
#pragma unroll
    for (u32 k = 0; k < 8u / R; k++)
#pragma unroll
        for (u32 c = 0; c < R; c++) {
            const u32 i = T + k * C::TA + c * NG;
            s.x[k * R + c] = sym[i];
            if (ROT) s.w[k * R + c] = A.nco[(ph0 + (n0 + i) * step) >> A.nco_shift];
        }
}

template <u32 M, bool ROT, bool DEMAP, bool INT, bool CSI = false>
__global__ __launch_bounds__(Cfg<M>::TPB) __attribute__((amdgpu_waves_per_eu(Cfg<M>::waves(ROT), Cfg<M>::waves(ROT)))) void vit_ofdm_td_kernel(TdArgs A) {
    typedef Cfg<M> C;
    constexpr u32 N = C::N, TA = C::TA, R1 = C::R1, R = 1u << R1, NP = C::NP;
    extern __shared__ float2 lds_td[];
    const u32 T = threadIdx.x;
    const bool active = C::TPB == TA || T < TA;
    const u64 t = blockIdx.x / A.runs;
    long long st = (long long)(t * A.frame_stride);
    if (A.start) {  // the frame is skipped unless all its reads are inside [0, nsamples)
        st = A.start[t];
        if (st < 0 || (u64)st > A.nsamples || A.extent > A.nsamples - (u64)st) return;
    }
    const void* frame = INT ? static_cast<const void*>(reinterpret_cast<const char*>(A.iq) + st * (long long)vit_iq::sample_bytes(A.iq_fmt))
                            : static_cast<const void*>(A.iq + st);
    const u32 s0 = A.lo + (u32)(blockIdx.x % A.runs) * A.run, s1 = s0 + A.run < A.hi ? s0 + A.run : A.hi;
    const u32 l1 = DEMAP ? s1 : s1 - 1u;  // the symbols s0 ... l1 are transformed
    u32 ph0 = 0, step = 0;
    if (ROT) {
        const uint2 r = A.rot[t];
        ph0 = r.x;
        step = r.y;
    }

    static_assert(pad_is_affine(M), "pad() must skew every thread's group alike");
    float2* tw_lds = lds_td + Cfg<M>::PADN;  // the twiddles live in LDS behind the symbol
    float2 e1, e3;
    fft_twiddles_to_lds<M>(tw_lds, A.tw, T, e1, e3);
    float* part = reinterpret_cast<float*>(lds_td) + C::LDS_BYTES / 4u;  // CSI: the wavefronts' totals, +0 behind the last
    if (CSI && T < vit_csi::CSI_PARTS) part[T] = 0.0f;
    __syncthreads();
    // the thread's carriers: groups T + j*TPB of 4 consecutive n
    u32 bin[C::CG][4];
    float2 prev[C::CG][4];
    if (DEMAP) {
#pragma unroll
        for (u32 j = 0; j < C::CG; j++)
#pragma unroll
            for (u32 c = 0; c < 4; c++) {
                const u32 n = 4u * (T + j * C::TPB) + c;
                bin[j][c] = n < A.K ? (u32)A.bins[n] : N;  // >= N: no carrier, erasures
                prev[j][c] = make_float2(0.f, 0.f);
            }
    }

    Samples<M, ROT, INT> smp;
    if (active) load_samples<M, ROT, INT>(A, frame, s0, ph0, step, T, smp);
    for (u32 l = s0; l <= l1; l++) {
        if (active) {
            float2 xi[INT ? 8 : 1];
            if constexpr (INT) vit_iq::iq_convert<8>(smp.raw, A.iq_fmt, A.iq_scale, xi);
#pragma unroll
            for (u32 k = 0; k < 8u / R; k++) {
                float2 v[R];
#pragma unroll
                for (u32 c = 0; c < R; c++) {
                    float2 x = INT ? xi[INT ? k * R + c : 0] : smp.x[INT ? 0 : k * R + c];
                    if (ROT) {
                        const float2 ww = smp.w[k * R + c];
                        x = make_float2(x.x * ww.x - x.y * ww.y, x.x * ww.y + x.y * ww.x);
                    }
                    v[bitrev(c, R1)] = x;
                }
                first_stages<R1>(v, e1, e3);
                float2* g = lds_td + pad(R * (__builtin_bitreverse32(T + k * TA) >> (32u - (M - R1))));
#pragma unroll
                for (u32 q = 0; q < R; q++) g[q] = v[q];
            }
            if (l < l1) load_samples<M, ROT, INT>(A, frame, l + 1u, ph0, step, T, smp);
        }
        __syncthreads();
#pragma unroll
        for (u32 p = 0; p < NP; p++) {  // fft_radix8_passes' loop, written out: vit_fft_dev.h has the measured reason
            if (active) {
                const u32 s = R1 + 3u * p;
                float2* g = lds_td + pad(pass_base(T, s));
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
        if (DEMAP) {
            const u32 s = l - 1u;  // the data symbol this transform completes (none at l = s0)
            // soft_dst(A, t, s) written out: through the function the integer formats' per-symbol kernel at nfft 2048 took
            // 0.2 - 0.3 % longer (0.2122 -> 0.2127 ms for 512 frames, profiles/r19_front_isa_same.txt)
            uint8_t* dst = nullptr;
            if (l > s0) {
                if (s < A.fic_syms) {
                    dst = A.fic + (t * A.fic_syms + s) * 2u * A.K;
                } else {
                    const u32 m = s - A.fic_syms, c = m / A.per;
                    u64 row = A.first_row + t * A.cifs + c;
                    if (row >= A.nrows) row -= A.nrows;
                    dst = A.ring + row * A.row_bytes + A.col + (u64)(m - c * A.per) * 2u * A.K;
                }
            }
            float yre[CSI ? C::CG : 1][4], yim[CSI ? C::CG : 1][4], sc = 0.0f;
            if constexpr (CSI) {
                // re, im of the thread's carriers (0 for an erasure) and accumulator T of the symbol's level
                float acc = 0.0f;
#pragma unroll
                for (u32 j = 0; j < C::CG; j++) {
                    float v[4];
#pragma unroll
                    for (u32 c = 0; c < 4; c++) {
                        const bool named = bin[j][c] < N;
                        const float2 a = named ? lds_td[pad(bin[j][c])] : make_float2(0.f, 0.f);
                        const float2 b = prev[j][c];
                        const float re = a.x * b.x + a.y * b.y;
                        const float im = a.y * b.x - a.x * b.y;
                        v[c] = named ? vit_csi::csi_term(__builtin_fabsf(re) + __builtin_fabsf(im)) : 0.0f;
                        yre[j][c] = v[c] != 0.0f ? re : 0.0f;
                        yim[j][c] = v[c] != 0.0f ? im : 0.0f;
                        prev[j][c] = a;
                    }
                    const float q = vit_csi::csi_group(v[0], v[1], v[2], v[3]);
                    acc = j ? acc + q : q;  // a group at or beyond K adds +0
                }
                if (dst) {  // uniform: every symbol of the run but the one before it
                    acc = vit_wave::wave_sum(acc);
                    if ((T & 63u) == 0) part[T >> 6] = acc;
                    __syncthreads();
                    const float S = vit_wave::pair_tree<C::TPB / 64u>(part);
                    sc = vit_csi::csi_scale(S, A.gain, A.K);
                    if (T == 0 && A.level) A.level[t * A.nlev + s] = S;
                }
            }
#pragma unroll
            for (u32 j = 0; j < C::CG; j++) {
                const u32 n0 = 4u * (T + j * C::TPB);
                if (n0 >= A.K) continue;
                u32 lo4 = 0, hi4 = 0;
                if constexpr (CSI) {
#pragma unroll
                    for (u32 c = 0; c < 4; c++) {
                        const u32 q = vit_csi::csi_pair(yre[j][c], yim[j][c], sc);
                        lo4 |= (q & 0xFFu) << (8u * c);
                        hi4 |= (q >> 8) << (8u * c);
                    }
                } else {
#pragma unroll
                    for (u32 c = 0; c < 4; c++) {
                        const bool named = bin[j][c] < N;
                        const float2 a = named ? lds_td[pad(bin[j][c])] : make_float2(0.f, 0.f);
                        const u32 q = named && dst ? soft_pair(a.x, a.y, prev[j][c].x, prev[j][c].y, A.gain) : 0x8080u;
                        lo4 |= (q & 0xFFu) << (8u * c);
                        hi4 |= (q >> 8) << (8u * c);
                        prev[j][c] = a;
                    }
                }
                if (!dst) continue;
                if (n0 + 4u <= A.K) {
                    __builtin_memcpy(dst + n0, &lo4, 4);  // unaligned global_store_dword
                    __builtin_memcpy(dst + A.K + n0, &hi4, 4);
                } else {
                    for (u32 c = 0; n0 + c < A.K; c++) {
                        dst[n0 + c] = (uint8_t)(lo4 >> (8u * c));
                        dst[A.K + n0 + c] = (uint8_t)(hi4 >> (8u * c));
                    }
                }
            }
        } else {
            float2* o = A.out + t * A.out_frame_stride + (u64)l * A.out_sym_stride;
            for (u32 i = T; i < N; i += C::TPB) o[i] = lds_td[pad(i)];
        }
        __syncthreads();  // the spectrum has been read: the next symbol's first pass may overwrite it
    }
}

template <u32 M, bool ROT, bool DEMAP, bool INT, bool CSI = false>
hipError_t launch3(const TdArgs& A, u64 grid, hipStream_t stream) {
    const size_t lds = Cfg<M>::LDS_BYTES + (CSI ? 4u * vit_csi::CSI_PARTS : 0u);
    return vit_launch_dynamic_lds<&vit_ofdm_td_kernel<M, ROT, DEMAP, INT, CSI>>((unsigned)grid, Cfg<M>::TPB, lds, stream, A);
}

template <u32 M, bool INT>
hipError_t launch2i(const TdArgs& A, bool demap, u64 grid, hipStream_t stream) {
    if (demap && A.csi) return A.rot ? launch3<M, true, true, INT, true>(A, grid, stream) : launch3<M, false, true, INT, true>(A, grid, stream);
    if (A.rot) return demap ? launch3<M, true, true, INT>(A, grid, stream) : launch3<M, true, false, INT>(A, grid, stream);
    return demap ? launch3<M, false, true, INT>(A, grid, stream) : launch3<M, false, false, INT>(A, grid, stream);
}

template <u32 M>
hipError_t launch2(const TdArgs& A, bool demap, u64 grid, hipStream_t stream) {
    return A.iq_fmt == VIT_IQ_F32 ? launch2i<M, false>(A, demap, grid, stream) : launch2i<M, true>(A, demap, grid, stream);
}

// the symbols [lo, hi) of every frame, split into runs (vit_demap_dev.h), by the instantiation for nfft
hipError_t launch(TdArgs& A, u32 nfft, bool demap, int64_t nframes, hipStream_t stream) {
    const u64 grid = split_runs(A, nframes);
    if (grid == 0) return hipSuccess;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    return for_nfft(nfft, [&](auto m) { return launch2<decltype(m)::value>(A, demap, grid, stream); });
}

TdArgs input_args(const vit_iq_input& in, const vit_iq_format& fmt, u32 nfft, u32 nsyms) {
    TdArgs A = {};
    A.iq = reinterpret_cast<const float2*>(in.d_iq);
    A.iq_fmt = fmt.format;
    A.iq_scale = fmt.scale;
    A.nsamples = in.nsamples;
    A.sym_stride = in.sym_stride;
    A.frame_stride = in.frame_stride;
    A.extent = (u64)(nsyms - 1u) * in.sym_stride + nfft;  // the caller has checked that it does not overflow
    A.start = reinterpret_cast<const long long*>(in.d_start);
    A.tw = reinterpret_cast<const float2*>(in.d_tw);
    if (in.d_rot) {
        A.nco = reinterpret_cast<const float2*>(in.d_nco);
        A.rot = reinterpret_cast<const uint2*>(in.d_rot);
        A.nco_shift = 32u - in.nco_bits;
    }
    return A;
}

// exact at multiples of an eighth of a turn, binary64 cos / sin rounded to binary32 elsewhere: (cos, sgn * sin)(2 pi k / n)
void unit_pair(u64 k, u64 n, double sgn, float* out) {
    static const double PI = 3.14159265358979323846;
    if ((8u * k) % n == 0) {
        const float r = (float)std::sqrt(0.5);
        const float c[8] = {1.f, r, 0.f, -r, -1.f, -r, 0.f, r}, s[8] = {0.f, r, 1.f, r, 0.f, -r, -1.f, -r};
        const u32 e = (u32)(8u * k / n) & 7u;
        out[0] = c[e];
        out[1] = s[e] == 0.f ? 0.f : (float)(sgn * (double)s[e]);
        return;
    }
    const double a = 2.0 * PI * (double)k / (double)n;
    out[0] = (float)std::cos(a);
    out[1] = (float)(sgn * std::sin(a));
}

}  // namespace

int64_t vit_fft_twiddles_host(uint32_t nfft, float* h_tw) {
    if (!h_tw || nfft < 64u || nfft > 8192u || (nfft & (nfft - 1u)) != 0) return -1;
    for (u32 k = 0; k < nfft / 2u; k++) unit_pair(k, nfft, -1.0, h_tw + 2u * k);
    return nfft / 2u;
}

int64_t vit_nco_table_host(uint32_t nco_bits, float* h_nco) {
    if (!h_nco || nco_bits < 1u || nco_bits > 20u) return -1;
    const u64 n = 1ull << nco_bits;
    for (u64 k = 0; k < n; k++) unit_pair(k, n, 1.0, h_nco + 2u * k);
    return (int64_t)n;
}

hipError_t vit_launch_ofdm_fft(const vit_iq_input& in, const vit_iq_format& fmt, uint32_t nfft, uint32_t nsyms, int64_t nframes, float* d_fft,
                               uint64_t out_sym_stride, uint64_t out_frame_stride, hipStream_t stream) {
    TdArgs A = input_args(in, fmt, nfft, nsyms);
    A.lo = 0;
    A.hi = nsyms;
    A.out = reinterpret_cast<float2*>(d_fft);
    A.out_sym_stride = out_sym_stride;
    A.out_frame_stride = out_frame_stride;
    return launch(A, nfft, false, nframes, stream);
}

hipError_t vit_launch_ofdm_demod(const vit_iq_input& in, const vit_iq_format& fmt, const uint16_t* d_bins, const vit_ofdm_shape& shape, float gain,
                                 int64_t nframes, uint8_t* d_fic, const vit_cif_ring* ring, uint64_t col, uint32_t rule, float* d_level,
                                 hipStream_t stream) {
    TdArgs A = input_args(in, fmt, shape.nfft, shape.nsyms);
    A.bins = d_bins;
    set_outputs(A, shape, gain, d_fic, ring, col);
    A.csi = rule == VIT_SOFT_PER_SYMBOL;
    A.level = d_level;
    A.nlev = shape.nsyms - 1u;
    return launch(A, shape.nfft, true, nframes, stream);
}
