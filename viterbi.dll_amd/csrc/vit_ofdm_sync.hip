// vit_ofdm_sync.hip -- from the coarse start to the two tables vit_ofdm_demod_dev reads (include/viterbi_amd.h, "From
// the coarse start"): per frame the fractional carrier offset from the guard intervals, the integer offset and the first
// path from the phase reference symbol.  Defined bit for bit: every float operation is one IEEE binary32 operation
// (contraction off, plain operators), the two transforms are the passes of vit_fft_dev.h, and every long sum has the
// header's grouping - element e goes to accumulator e mod NACC in ascending order, NACC = the workgroup's size
// max(64, nfft/8), and the accumulators meet in the tree of adjacent pairs.
//
// One workgroup owns one frame; thread T is accumulator T.
//   A  streams the guard pairs (x[n], x[n + nfft]) of the cp_symbols guards: consecutive threads read consecutive
//      samples, four pairs in flight per thread; gamma and E meet in one block reduction.
//   B  rotates the window at c - W by the fractional step and transforms it in LDS: Y.
//   C  the shifts m = -M ... M, four accumulators at a time.  D[k] = Y[k] conj(Y[k-1]) is not stored: a thread reads the
//      5 neighbouring Y of its k from LDS for 4 shifts and forms the 4 D from them, the same operations on the same
//      values whenever it is done.  A second padded array would not fit beside Y and the twiddles at nfft 8192, and at the
//      other lengths it would halve the workgroups a CU holds.  R[k] = P[k] conj(P[k-1]) of the thread's k stays in
//      registers.  Wavefront totals go to LDS; one barrier serves all shifts.
//   D  Z[k] = Y[k + m^] conj(P[k]) is read into registers, a barrier, and conj Z is transformed in place of Y; the
//      powers |h|^2 are reduced from LDS (sum, maximum over 0 ... 2W, first index over the threshold).
// Thread 0 writes the frame's 1 + 2 + 8 words.
// Integer sample formats (vit_iq_dev.h): one template flag apart from the float32 instantiations.  Only the loads of A
// and B change - the pairs in flight stay raw until they are accumulated - and A's loop is written once per format.
#pragma clang fp contract(off)
#include "vit_fft_dev.h"
#include "vit_internal.h"
#include "vit_iq_dev.h"
#include "vit_wave_dev.h"

namespace {

using namespace vit_fft;
using vit_wave::pair_tree;

constexpr u32 MMAX = 64u;              // integer offsets searched at most: -64 ... 64
constexpr u32 NSHIFT_MAX = 2u * MMAX + 1u;
constexpr u32 SHIFT_GROUP = 4u;        // shifts a thread accumulates at a time
constexpr u32 PAIRS_IN_FLIGHT = 4u;    // guard pairs a thread loads before it accumulates them

struct SyncArgs {
    const float2* iq;
    u64 nsamples, sym_stride, frame_stride;
    u64 span;  // samples from c - W to the frame's last read, + 1
    const long long* start;
    long long first_start;
    const float2* tw;
    const float2* nco;
    const float2* prs;
    u32 nco_shift;  // 32 - nco_bits
    u32 cp, W, M, G;
    float thr;
    int backoff;
    long long* start_out;
    uint2* rot_out;
    u32* info;
    // integer sample formats: iq then points at samples of iq_fmt (VIT_IQ_CU8 ... VIT_IQ_CS16)
    u32 iq_fmt;
    float iq_scale;
};

// LDS behind the symbol and the twiddles, in floats; J wavefronts
template <u32 J>
struct Scratch {
    static constexpr u32 GUARDS = 0u;                       // 3 sums x J
    static constexpr u32 SHIFTS = GUARDS + 3u * J;           // NSHIFT_MAX x J x (re, im)
    static constexpr u32 METRIC = SHIFTS + NSHIFT_MAX * J * 2u;
    static constexpr u32 POWER = METRIC + NSHIFT_MAX + 3u;  // sum, maximum, first index: J each
    static constexpr u32 FLOATS = POWER + 3u * J;
};

// The tree of adjacent pairs over the 64 lanes: every lane ends with the wavefront's total.  vit_wave::wave_sum's bits by six
// ds_bpermute exchanges instead of four DPP additions and two: with the DPP form the nfft 8192 instantiations, which sit at
// their 128 VGPRs, spill 28 bytes more (scratch 192 -> 220, profiles/r19_front_isa_same.txt), so this kernel keeps its own.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (u32 h = 1; h < 64u; h *= 2) v = v + __shfl_xor(v, (int)h);
    return v;
}

// atan2(im, re) / 2 pi in [-1/2, 1/2]: the header's graph
__device__ __forceinline__ float turn_of(float re, float im) {
    const float ax = __builtin_fabsf(re), ay = __builtin_fabsf(im);
    const float mx = ax > ay ? ax : ay, mn = ax > ay ? ay : ax;
    if (!(mx > 0.0f)) return 0.0f;
    const float q = mn / mx;
    const float s = q * q;
    float p = VIT_SYNC_ATAN_C6;
    p = p * s + VIT_SYNC_ATAN_C5;
    p = p * s + VIT_SYNC_ATAN_C4;
    p = p * s + VIT_SYNC_ATAN_C3;
    p = p * s + VIT_SYNC_ATAN_C2;
    p = p * s + VIT_SYNC_ATAN_C1;
    p = p * s + VIT_SYNC_ATAN_C0;
    float r = p * q;
    if (ay > ax) r = 0.25f - r;
    if (re < 0.0f) r = 0.5f - r;
    if (im < 0.0f) r = -r;
    return r;
}

// step A on an integer format FMT: the loop of the float32 kernel with the pairs in flight kept raw
template <u32 FMT, u32 N, u32 TPB>
__device__ __forceinline__ void guard_sums_int(const SyncArgs& A, long long c, u32 T, float& gr, float& gi, float& en) {
    constexpr u32 SB = vit_iq::sample_bytes(FMT);
    const u32 Gw = A.G - 2u * A.W;
    const u64 total = (u64)A.cp * Gw;
    const char* guard0 = reinterpret_cast<const char*>(A.iq) + (c + N + A.W) * (long long)SB;
    const u32 dq = TPB / Gw, dr = TPB % Gw;
    u32 l = T / Gw, k = T % Gw;
    for (u64 e = T; e < total; e += (u64)PAIRS_IN_FLIGHT * TPB) {
        u32 ra[PAIRS_IN_FLIGHT], rb[PAIRS_IN_FLIGHT];
#pragma unroll
        for (u32 u = 0; u < PAIRS_IN_FLIGHT; u++) {
            ra[u] = rb[u] = 0u;
            if (e + (u64)u * TPB < total) {
                const char* p = guard0 + ((u64)l * A.sym_stride + k) * SB;
                u32 two[2];
                vit_iq::iq_load_raw<2>(p, FMT, two, [](u32 j) { return j * N; });
                ra[u] = two[0];
                rb[u] = two[1];
            }
            k += dr;
            l += dq;
            if (k >= Gw) {
                k -= Gw;
                l++;
            }
        }
        float2 a[PAIRS_IN_FLIGHT], b[PAIRS_IN_FLIGHT];
        vit_iq::iq_convert<PAIRS_IN_FLIGHT>(ra, FMT, A.iq_scale, a);
        vit_iq::iq_convert<PAIRS_IN_FLIGHT>(rb, FMT, A.iq_scale, b);
#pragma unroll
        for (u32 u = 0; u < PAIRS_IN_FLIGHT; u++)
            if (e + (u64)u * TPB < total) {
                gr = gr + (a[u].x * b[u].x + a[u].y * b[u].y);
                gi = gi + (a[u].x * b[u].y - a[u].y * b[u].x);
                en = en + ((a[u].x * a[u].x + a[u].y * a[u].y) + (b[u].x * b[u].x + b[u].y * b[u].y));
            }
    }
}

template <u32 M_, bool INT>
__global__ __launch_bounds__(Cfg<M_>::TPB) void vit_ofdm_sync_kernel(SyncArgs A) {
    typedef Cfg<M_> C;
    constexpr u32 N = C::N, TA = C::TA, TPB = C::TPB, J = TPB / 64u, KPT = N / TPB;
    typedef Scratch<J> S;
    extern __shared__ float2 lds_sync[];
    static_assert(pad_is_affine(M_), "pad() must skew every thread's group alike");
    float2* tw_lds = lds_sync + C::PADN;
    float* scr = reinterpret_cast<float*>(tw_lds + N / 2u + N / 64u);
    const u32 T = threadIdx.x, lane = T & 63u, wave = T >> 6;
    const bool active = TPB == TA || T < TA;
    const u64 t = blockIdx.x;
    const long long c = A.start ? A.start[t] : A.first_start + (long long)(t * A.frame_stride);
    // the frame is skipped unless c - W ... c - W + span - 1 are inside [0, nsamples)
    if (c < (long long)A.W || (u64)(c - A.W) > A.nsamples || A.span > A.nsamples - (u64)(c - A.W)) {
        __syncthreads();  // d_start_out may be d_start: every thread has read its entry
        if (T == 0) {
            A.start_out[t] = -1;
            A.rot_out[t] = make_uint2(0u, 0u);
            if (A.info)
                for (u32 i = 0; i < 8u; i++) A.info[8u * t + i] = 0u;
        }
        return;
    }
    float2 e1, e3;
    fft_twiddles_to_lds<M_>(tw_lds, A.tw, T, e1, e3);

    // ---- A: the guards.  Element e = (l - 1)*Gw + k is the pair at c + l*S - G + W + k = c + nfft + W + (l - 1)*S + k
    const u32 Gw = A.G - 2u * A.W;
    const u64 total = (u64)A.cp * Gw;
    const float2* guard0 = A.iq + c + N + A.W;
    const u32 dq = TPB / Gw, dr = TPB % Gw;
    u32 l = T / Gw, k = T % Gw;
    float gr = 0.f, gi = 0.f, en = 0.f;
    if constexpr (INT) {
        if (A.iq_fmt == VIT_IQ_CU8) guard_sums_int<VIT_IQ_CU8, N, TPB>(A, c, T, gr, gi, en);
        else if (A.iq_fmt == VIT_IQ_CS8) guard_sums_int<VIT_IQ_CS8, N, TPB>(A, c, T, gr, gi, en);
        else guard_sums_int<VIT_IQ_CS16, N, TPB>(A, c, T, gr, gi, en);
    }
    for (u64 e = T; !INT && e < total; e += (u64)PAIRS_IN_FLIGHT * TPB) {
        float2 a[PAIRS_IN_FLIGHT], b[PAIRS_IN_FLIGHT];
#pragma unroll
        for (u32 u = 0; u < PAIRS_IN_FLIGHT; u++) {
            a[u] = b[u] = make_float2(0.f, 0.f);
            if (e + (u64)u * TPB < total) {
                const float2* p = guard0 + (u64)l * A.sym_stride + k;
                a[u] = p[0];
                b[u] = p[N];
            }
            k += dr;
            l += dq;
            if (k >= Gw) {
                k -= Gw;
                l++;
            }
        }
#pragma unroll
        for (u32 u = 0; u < PAIRS_IN_FLIGHT; u++)
            if (e + (u64)u * TPB < total) {
                gr = gr + (a[u].x * b[u].x + a[u].y * b[u].y);
                gi = gi + (a[u].x * b[u].y - a[u].y * b[u].x);
                en = en + ((a[u].x * a[u].x + a[u].y * a[u].y) + (b[u].x * b[u].x + b[u].y * b[u].y));
            }
    }
    gr = wave_sum(gr);
    gi = wave_sum(gi);
    en = wave_sum(en);
    if (lane == 0) {
        scr[S::GUARDS + wave] = gr;
        scr[S::GUARDS + J + wave] = gi;
        scr[S::GUARDS + 2u * J + wave] = en;
    }
    __syncthreads();  // and the twiddles are in LDS
    gr = pair_tree<J>(scr + S::GUARDS);
    gi = pair_tree<J>(scr + S::GUARDS + J);
    en = pair_tree<J>(scr + S::GUARDS + 2u * J);
    const float turn = turn_of(gr, gi);
    const float scale = (float)(1u << (32u - M_));  // 2^32 / nfft
    const u32 step_frac = 0u - (u32)(int)__builtin_rintf(turn * scale);

    // ---- B: the phase reference symbol's window at c - W, rotated by step_frac, transformed
    if (active) {
        const float2* win = A.iq + (c - (long long)A.W);
        float2 xi[INT ? 8 : 1];
        if constexpr (INT) {
            u32 raw[8];
            const char* wi = reinterpret_cast<const char*>(A.iq) + (c - (long long)A.W) * (long long)vit_iq::sample_bytes(A.iq_fmt);
            vit_iq::iq_load_raw<8>(wi, A.iq_fmt, raw, [T](u32 j) { return input_index<M_>(T, j); });
            vit_iq::iq_convert<8>(raw, A.iq_fmt, A.iq_scale, xi);
        }
        float2 x[8];
#pragma unroll
        for (u32 j = 0; j < 8; j++) {
            const u32 i = input_index<M_>(T, j);
            const float2 v = INT ? xi[INT ? j : 0] : win[i];
            const float2 w = A.nco[(i * step_frac) >> A.nco_shift];
            x[j] = make_float2(v.x * w.x - v.y * w.y, v.x * w.y + v.y * w.x);
        }
        fft_first_pass<M_>(lds_sync, T, x, e1, e3);
    }
    __syncthreads();
    fft_radix8_passes<M_>(lds_sync, tw_lds, T, active);

    // ---- C: the integer offset.  k = T + j*TPB: element k of every C[m] goes to accumulator T
    float2 R[KPT];
#pragma unroll
    for (u32 j = 0; j < KPT; j++) {
        const u32 kk = T + j * TPB;
        const float2 a = A.prs[kk], b = A.prs[(kk + N - 1u) & (N - 1u)];
        R[j] = make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
    }
    const u32 nshift = 2u * A.M + 1u;
    for (u32 g0 = 0; g0 < nshift; g0 += SHIFT_GROUP) {
        float2 acc[SHIFT_GROUP];
#pragma unroll
        for (u32 a = 0; a < SHIFT_GROUP; a++) acc[a] = make_float2(0.f, 0.f);
#pragma unroll
        for (u32 j = 0; j < KPT; j++) {
            const u32 i0 = T + j * TPB + N - A.M + g0 - 1u;  // k + m - 1 for the group's first shift m = g0 - M
            float2 y[SHIFT_GROUP + 1u];
#pragma unroll
            for (u32 a = 0; a <= SHIFT_GROUP; a++) y[a] = lds_sync[pad((i0 + a) & (N - 1u))];
#pragma unroll
            for (u32 a = 0; a < SHIFT_GROUP; a++) {
                const float2 u = y[a + 1u], v = y[a];
                const float2 d = make_float2(u.x * v.x + u.y * v.y, u.y * v.x - u.x * v.y);
                acc[a].x = acc[a].x + (d.x * R[j].x + d.y * R[j].y);
                acc[a].y = acc[a].y + (d.y * R[j].x - d.x * R[j].y);
            }
        }
#pragma unroll
        for (u32 a = 0; a < SHIFT_GROUP; a++) {
            const float re = wave_sum(acc[a].x), im = wave_sum(acc[a].y);
            if (lane == 0 && g0 + a < nshift) {
                scr[S::SHIFTS + ((g0 + a) * J + wave) * 2u] = re;
                scr[S::SHIFTS + ((g0 + a) * J + wave) * 2u + 1u] = im;
            }
        }
    }
    __syncthreads();
    for (u32 i = T; i < nshift; i += TPB) {
        const float re = pair_tree<J>(scr + S::SHIFTS + i * J * 2u, 2u);
        const float im = pair_tree<J>(scr + S::SHIFTS + i * J * 2u + 1u, 2u);
        scr[S::METRIC + i] = re * re + im * im;
    }
    __syncthreads();
    float best = scr[S::METRIC];
    u32 besti = 0;
    for (u32 i = 1; i < nshift; i++) {  // the first maximum; every thread scans the same words
        const float v = scr[S::METRIC + i];
        if (v > best) {
            best = v;
            besti = i;
        }
    }
    const int mhat = (int)besti - (int)A.M;

    // ---- D: the impulse response.  conj Z into registers, then its transform in place of Y
    float2 z[8];
    if (active) {
#pragma unroll
        for (u32 j = 0; j < 8; j++) {
            const u32 i = input_index<M_>(T, j);
            const float2 y = lds_sync[pad((i + N + (u32)mhat) & (N - 1u))];
            const float2 p = A.prs[i];
            z[j] = make_float2(y.x * p.x + y.y * p.y, -(y.y * p.x - y.x * p.y));
        }
    }
    __syncthreads();  // Y has been read
    if (active) fft_first_pass<M_>(lds_sync, T, z, e1, e3);
    __syncthreads();
    fft_radix8_passes<M_>(lds_sync, tw_lds, T, active);
    float pw[KPT];
    float psum = 0.f, pmax = 0.f;
#pragma unroll
    for (u32 j = 0; j < KPT; j++) {
        const u32 n = T + j * TPB;
        const float2 h = lds_sync[pad(n)];
        pw[j] = h.x * h.x + h.y * h.y;
        psum = psum + pw[j];
        if (n <= 2u * A.W && pw[j] > pmax) pmax = pw[j];
    }
    psum = wave_sum(psum);
#pragma unroll
    for (u32 h = 1; h < 64u; h *= 2) {
        const float o = __shfl_xor(pmax, (int)h);
        pmax = o > pmax ? o : pmax;
    }
    if (lane == 0) {
        scr[S::POWER + wave] = psum;
        scr[S::POWER + J + wave] = pmax;
    }
    __syncthreads();
    psum = pair_tree<J>(scr + S::POWER);
#pragma unroll
    for (u32 i = 0; i < J; i++) {
        const float o = scr[S::POWER + J + i];
        pmax = o > pmax ? o : pmax;
    }
    const float level = A.thr * pmax;
    u32 tau = 0xFFFFFFFFu;
#pragma unroll
    for (u32 j = KPT; j-- > 0;) {
        const u32 n = T + j * TPB;
        if (n <= 2u * A.W && pw[j] >= level) tau = n;
    }
#pragma unroll
    for (u32 h = 1; h < 64u; h *= 2) {
        const u32 o = (u32)__shfl_xor((int)tau, (int)h);
        tau = o < tau ? o : tau;
    }
    u32* scr_tau = reinterpret_cast<u32*>(scr + S::POWER + 2u * J);
    if (lane == 0) scr_tau[wave] = tau;
    __syncthreads();
    if (T == 0) {
#pragma unroll
        for (u32 i = 0; i < J; i++) tau = scr_tau[i] < tau ? scr_tau[i] : tau;
        if (tau > 2u * A.W) tau = 0u;  // no power reaches the level: NaN, outside the domain
        A.start_out[t] = c - (long long)A.W + (long long)tau - (long long)A.backoff;
        A.rot_out[t] = make_uint2(0u, step_frac - (u32)mhat * (1u << (32u - M_)));
        if (A.info) {
            u32* o = A.info + 8u * t;
            o[0] = (u32)mhat;
            o[1] = tau;
            o[2] = __float_as_uint(gr);
            o[3] = __float_as_uint(gi);
            o[4] = __float_as_uint(en);
            o[5] = __float_as_uint(best);
            o[6] = __float_as_uint(pmax);
            o[7] = __float_as_uint(psum);
        }
    }
}

template <u32 M_, bool INT>
hipError_t launch_sync2(const SyncArgs& A, int64_t nframes, hipStream_t stream) {
    typedef Cfg<M_> C;
    const size_t lds = C::LDS_BYTES + Scratch<C::TPB / 64u>::FLOATS * 4u;
    return vit_launch_dynamic_lds<&vit_ofdm_sync_kernel<M_, INT>>((unsigned)nframes, C::TPB, lds, stream, A);
}

template <u32 M_>
hipError_t launch_sync(const SyncArgs& A, int64_t nframes, hipStream_t stream) {
    return A.iq_fmt == VIT_IQ_F32 ? launch_sync2<M_, false>(A, nframes, stream) : launch_sync2<M_, true>(A, nframes, stream);
}

}  // namespace

hipError_t vit_launch_ofdm_sync(const vit_iq_input& in, const vit_iq_format& fmt, const vit_sync_params& p, const float* d_prs, int64_t nframes,
                                int64_t* d_start_out, uint32_t* d_rot_out, uint32_t* d_info, hipStream_t stream) {
    if (nframes <= 0) return hipSuccess;
    if (nframes > 0x7FFFFFFFll) return hipErrorInvalidValue;
    SyncArgs A = {};
    A.iq = reinterpret_cast<const float2*>(in.d_iq);
    A.nsamples = in.nsamples;
    A.sym_stride = in.sym_stride;
    A.frame_stride = in.frame_stride;
    A.span = (u64)(p.nsyms - 1u) * in.sym_stride + p.nfft + 2u * (u64)p.W;  // the caller has checked that it does not overflow
    A.start = reinterpret_cast<const long long*>(in.d_start);
    A.first_start = p.first_start;
    A.tw = reinterpret_cast<const float2*>(in.d_tw);
    A.nco = reinterpret_cast<const float2*>(in.d_nco);
    A.prs = reinterpret_cast<const float2*>(d_prs);
    A.nco_shift = 32u - in.nco_bits;
    A.cp = p.cp_symbols;
    A.W = p.W;
    A.M = p.M;
    A.G = (u32)(in.sym_stride - p.nfft);
    A.thr = p.thr;
    A.backoff = p.backoff;
    A.start_out = reinterpret_cast<long long*>(d_start_out);
    A.rot_out = reinterpret_cast<uint2*>(d_rot_out);
    A.info = d_info;
    A.iq_fmt = fmt.format;
    A.iq_scale = fmt.scale;
    return for_nfft(p.nfft, [&](auto m) { return launch_sync<decltype(m)::value>(A, nframes, stream); });
}
