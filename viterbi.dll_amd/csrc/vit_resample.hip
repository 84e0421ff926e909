// vit_resample.hip -- before the stream (include/viterbi_amd.h, "Before the stream: rate conversion and channel
// selection"): frequency shift, low-pass and rational rate change L/M of one stream of samples into nchan streams of
// float32 at the chain's rate.  Defined bit for bit: every float operation is one IEEE binary32 operation (contraction off,
// plain operators); an output's T products meet in four accumulators, term k in accumulator k mod 4, ascending.  Nothing
// depends on the launch: an output is formed by one thread from its own T samples and its own row of taps.
//
//   tile    A workgroup of 512 threads owns `tile` consecutive outputs for all channels and reads the tile's input span -
//           ((tile-1)*M + phi) div L + T samples, at most SPAN - once, through the loader of vit_iq_dev.h: thread t holds
//           samples t, t + 512, ... of the span raw in registers (a dword each, a float2 for float32), every load a whole
//           sample and no byte of another.  `tile` is the largest power of two <= 1024 whose span fits (resample_tile below;
//           the Python binding restates the rule for the tests).  The workgroups stride over the tiles.
//   channel The workgroup converts and rotates the span into LDS; thread t then forms outputs t, t + 512 of the tile from
//           it while the next channel's span is rotated into a second buffer.  Barriers per tile: one behind the first
//           rotation, one behind every channel - nchan + 1.  A buffer holds the span twice, the second copy one sample
//           (8 bytes) further on: an output's first sample has any index, and one of the two copies has it at a 16-byte
//           boundary, so a thread reads samples two at a time (ds_read_b128: 4 LDS cycles per 1 KiB, where the 8-byte
//           pairs the compiler would form, ds_read2_b64, take 8).
//   taps    In LDS, VIT_RESAMPLE_TAPS_LDS = 1: the L rows of T floats, each padded by 4 floats.  Consecutive outputs use rows
//           phi, phi + M mod L, ...: the 16 lanes that share an LDS cycle of a 16-byte read hold 16 different rows, and
//           at a row stride of T floats - 8 bank groups of 16 bytes at T 32, of 16 per LDS cycle - they would pile onto 2
//           of the 16; at T + 4 a row moves on by T/4 + 1 groups, odd for the production shapes (T 32, 128), and rows
//           phi ... phi + 15 (in any order) cover all 16.  The table and the spans take up to 80 + 64 KiB of the CU's 160, so one workgroup
//           is resident - which is why it has 512 threads, two wavefronts per SIMD.  = 0 reads the rows through the cache
//           (two workgroups per CU): every lane of a 16-byte load then names another cache line, and the call takes
//           1.34x ... 1.64x as long (tests/tools/bench_resample.py --ab, profiles/r17_resample_bench.json).
//   index   P = pos0 + m*M needs 64 bits once per tile (one division, uniform over the workgroup).  A thread divides
//           once per launch, for t*M; from there it steps by 512*M as (div L, mod L) with a carry, and the tile's phase
//           joins with one more carry: no division per output.
//   gaps    With M > L*T consecutive outputs' samples do not touch, a span would hold samples that no output needs - which
//           must not be read - and nothing is shared.  Then a thread reads its own T samples and its row from memory
//           (DIRECT), tile 512, no LDS.
#pragma clang fp contract(off)
#include "vit_internal.h"
#include "vit_iq_dev.h"

#ifndef VIT_RESAMPLE_TAPS_LDS
#define VIT_RESAMPLE_TAPS_LDS 1
#endif

namespace {

typedef uint32_t u32;
typedef uint64_t u64;

constexpr u32 TPB = 512u;
constexpr u32 SPAN = 2048u;          // samples of one tile's span, at most
constexpr u32 RAW = SPAN / TPB;      // samples a thread holds raw
constexpr u32 COPY = SPAN + 2u;      // float2 of one copy of the span (the second copy starts one sample in)
constexpr u32 TILE_MAX = 1024u;
constexpr u32 TAP_PAD = 4u;          // floats behind every row of taps in LDS
constexpr bool TAPS_LDS = VIT_RESAMPLE_TAPS_LDS != 0;
constexpr u32 MAX_GRID = 1u << 16;

struct ResampleArgs {
    const char* iq;       // sample 0 of d_iq
    const float* taps;
    const float2* nco;
    float2* out;
    u64 out_stride, pos0;
    long long nout;
    u32 L, M, T, nchan;
    u32 tile;             // outputs per tile
    u32 qstep, rstep;     // (TPB*M) div L, (TPB*M) mod L
    u32 nco_shift;        // 32 - nco_bits
    u32 rotate;           // 0: y = x
    float scale;
    u32 rot[2 * VIT_RESAMPLE_MAX_CHAN];  // {phase0, step} per channel
};

// one sample's bytes as they lie in memory, converted where they are consumed
template <u32 FMT> struct RawSample { typedef u32 type; };
template <> struct RawSample<VIT_IQ_F32> { typedef float2 type; };

template <u32 FMT>
__device__ __forceinline__ typename RawSample<FMT>::type load_raw(const char* iq, u64 n) {
    if constexpr (FMT == VIT_IQ_F32) {
        return reinterpret_cast<const float2*>(iq)[n];
    } else {
        u32 raw[1];
        vit_iq::iq_load_raw<1>(iq, FMT, raw, [n](u32) { return n; });
        return raw[0];
    }
}

template <u32 FMT>
__device__ __forceinline__ float2 to_float(const typename RawSample<FMT>::type& raw, float scale) {
    if constexpr (FMT == VIT_IQ_F32) {
        return raw;
    } else {
        const u32 r[1] = {raw};
        float2 x[1];
        vit_iq::iq_convert<1>(r, FMT, scale, x);
        return x[0];
    }
}

// step B: sample n of d_iq (its low 32 bits) for the channel with {phase0, step}
__device__ __forceinline__ float2 rotate(const ResampleArgs& A, float2 x, u32 n, u32 phase0, u32 step) {
    const float2 w = A.nco[(phase0 + n * step) >> A.nco_shift];
    return make_float2(x.x * w.x - x.y * w.y, x.x * w.y + x.y * w.x);
}

struct Acc {
    float re[4], im[4];
    __device__ __forceinline__ Acc() {
#pragma unroll
        for (u32 i = 0; i < 4; i++) re[i] = im[i] = 0.f;
    }
    __device__ __forceinline__ void add(u32 i, float g, float2 y) {
        re[i] = re[i] + g * y.x;
        im[i] = im[i] + g * y.y;
    }
    __device__ __forceinline__ float2 sum() const {
        return make_float2((re[0] + re[1]) + (re[2] + re[3]), (im[0] + im[1]) + (im[2] + im[3]));
    }
};

// the four taps g[k ... k+3] of a row in memory; d_taps is 8-byte aligned and so is every fourth float of a row
__device__ __forceinline__ float4 load_taps(const float* row, u32 k) {
    float4 g;
    __builtin_memcpy(&g, row + k, 16);
    return g;
}

// (q, r) += (dq, dr) in units of (1, 1/L)
__device__ __forceinline__ void step_position(u32& q, u32& r, u32 dq, u32 dr, u32 L) {
    q += dq;
    r += dr;
    if (r >= L) {
        r -= L;
        q++;
    }
}

template <u32 FMT, bool DIRECT>
__global__ __launch_bounds__(TPB) void vit_resample_kernel(ResampleArgs A) {
    typedef typename RawSample<FMT>::type raw_t;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const u32 t = threadIdx.x;
    const u32 L = A.L, T = A.T;
    // thread t's first output of a tile lies t*M behind the tile's position: < 2^9 * 2^12
    const u32 q_t = (t * A.M) / L, r_t = (t * A.M) % L;
    const u64 ntiles = ((u64)A.nout + A.tile - 1u) / A.tile;
    if constexpr (DIRECT) {
        for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
            const u64 m0 = tile * TPB;  // tile = TPB: thread t has output t
            if (m0 + t >= (u64)A.nout) continue;
            const u64 P0 = A.pos0 + m0 * A.M;
            u32 q = 0, r = (u32)(P0 % L);
            step_position(q, r, q_t, r_t, L);
            const u64 n0 = P0 / L + q;
            const float* row = A.taps + (u64)r * T;
            for (u32 c = 0; c < A.nchan; c++) {
                const u32 phase0 = A.rot[2u * c], step = A.rot[2u * c + 1u];
                Acc acc;
                for (u32 k = 0; k < T; k += 4u) {
                    const float4 g4 = load_taps(row, k);
                    const float g[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
                    for (u32 i = 0; i < 4; i++) {
                        float2 y = to_float<FMT>(load_raw<FMT>(A.iq, n0 + k + i), A.scale);
                        if (A.rotate) y = rotate(A, y, (u32)(n0 + k + i), phase0, step);
                        acc.add(i, g[i], y);
                    }
                }
                A.out[c * A.out_stride + m0 + t] = acc.sum();
            }
        }
    } else {
        const u32 row_floats = T + TAP_PAD;
        float* taps_lds = reinterpret_cast<float*>(lds);
        float2* span_lds = reinterpret_cast<float2*>(lds + (TAPS_LDS ? (size_t)L * row_floats * 4u : 0u));
        if constexpr (TAPS_LDS) {
            const u32 T4 = T / 4u;
            for (u32 e = t; e < L * T4; e += TPB)  // the first barrier below is in front of every read
                *reinterpret_cast<float4*>(taps_lds + (e / T4) * row_floats + 4u * (e % T4)) = load_taps(A.taps, 4u * e);
        }
        for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
            const u64 m0 = tile * A.tile;
            const u32 nt = (u64)A.nout - m0 < A.tile ? (u32)((u64)A.nout - m0) : A.tile;  // outputs of this tile
            const u64 P0 = A.pos0 + m0 * A.M;
            const u64 n00 = P0 / L;  // the tile's first sample
            const u32 phi0 = (u32)(P0 % L);
            const u32 span = (u32)(((u64)(nt - 1u) * A.M + phi0) / L) + T;  // <= SPAN by the choice of the tile
            raw_t raw[RAW];
#pragma unroll
            for (u32 j = 0; j < RAW; j++) {
                // beyond the span a thread repeats the span's last sample: no other is touched
                const u32 i = t + TPB * j < span ? t + TPB * j : span - 1u;
                raw[j] = load_raw<FMT>(A.iq, n00 + i);
            }
            auto rotate_span = [&](u32 c) {
                float2* a = span_lds + (c & 1u) * 2u * COPY;
                float2* b = a + COPY + 1u;  // sample i at index i + 1 of the second copy
                const u32 phase0 = A.rot[2u * c], step = A.rot[2u * c + 1u];
#pragma unroll
                for (u32 j = 0; j < RAW; j++) {
                    const u32 i = t + TPB * j;
                    if (i < span) {
                        float2 y = to_float<FMT>(raw[j], A.scale);
                        if (A.rotate) y = rotate(A, y, (u32)n00 + i, phase0, step);
                        a[i] = y;
                        b[i] = y;
                    }
                }
            };
            rotate_span(0);
            __syncthreads();
            for (u32 c = 0; c < A.nchan; c++) {
                if (c + 1u < A.nchan) rotate_span(c + 1u);  // into the buffer channel c-1 was read from, in front of the last barrier
                const float2* a = span_lds + (c & 1u) * 2u * COPY;
                u32 q = 0, r = phi0;
                step_position(q, r, q_t, r_t, L);
                for (u32 j = t; j < nt; j += TPB) {
                    // sample q at a 16-byte boundary: index q of the first copy, or index q + 1 of the second
                    const float4* y4 = reinterpret_cast<const float4*>((q & 1u) ? a + COPY + 1u + q : a + q);
                    const float* row = TAPS_LDS ? taps_lds + r * row_floats : A.taps + (u64)r * T;
                    Acc acc;
#pragma unroll 4  // 12 LDS reads in flight in front of the first product (T = 4, 8: the remainder loop)
                    for (u32 k = 0; k < T; k += 4u) {
                        const float4 g = TAPS_LDS ? *reinterpret_cast<const float4*>(row + k) : load_taps(row, k);
                        const float4 y01 = y4[k / 2u], y23 = y4[k / 2u + 1u];
                        acc.add(0, g.x, make_float2(y01.x, y01.y));
                        acc.add(1, g.y, make_float2(y01.z, y01.w));
                        acc.add(2, g.z, make_float2(y23.x, y23.y));
                        acc.add(3, g.w, make_float2(y23.z, y23.w));
                    }
                    A.out[c * A.out_stride + m0 + j] = acc.sum();
                    step_position(q, r, A.qstep, A.rstep, L);
                }
                __syncthreads();  // channel c is read: its buffer takes channel c+2, or the next tile's first
            }
        }
    }
}

template <u32 FMT>
hipError_t launch(bool direct, unsigned grid, size_t lds, hipStream_t stream, const ResampleArgs& A) {
    if (direct) {
        hipLaunchKernelGGL((vit_resample_kernel<FMT, true>), dim3(grid), dim3(TPB), 0, stream, A);
        return hipGetLastError();
    }
    return vit_launch_dynamic_lds<&vit_resample_kernel<FMT, false>>(grid, TPB, lds, stream, A);
}

}  // namespace

// outputs per tile and whether threads read their samples from memory (gaps between the outputs' samples)
static u32 resample_tile(u32 L, u32 M, u32 T, bool* direct) {
    *direct = (u64)M > (u64)L * T;
    if (*direct) return TPB;
    u32 tile = TILE_MAX;
    while (tile > 1u && ((u64)(tile - 1u) * M + L - 1u) / L + T > SPAN) tile /= 2u;
    return tile;
}

hipError_t vit_launch_resample(const void* d_iq, const vit_iq_format& fmt, const vit_resample_params& p, int64_t nout, float* d_out,
                               uint64_t out_stride, hipStream_t stream) {
    if (nout <= 0) return hipSuccess;
    ResampleArgs A = {};
    bool direct = false;
    A.iq = reinterpret_cast<const char*>(d_iq);
    A.taps = p.d_taps;
    A.nco = reinterpret_cast<const float2*>(p.d_nco);
    A.out = reinterpret_cast<float2*>(d_out);
    A.out_stride = out_stride;
    A.pos0 = p.pos0;
    A.nout = nout;
    A.L = p.L;
    A.M = p.M;
    A.T = p.T;
    A.nchan = p.nchan;
    A.tile = resample_tile(p.L, p.M, p.T, &direct);
    A.qstep = TPB * p.M / p.L;
    A.rstep = TPB * p.M % p.L;
    A.rotate = p.rot ? 1u : 0u;
    A.nco_shift = p.rot ? 32u - p.nco_bits : 0u;
    A.scale = fmt.scale;
    if (p.rot)
        for (u32 i = 0; i < 2u * p.nchan; i++) A.rot[i] = p.rot[i];
    const size_t lds = (TAPS_LDS ? (size_t)p.L * (p.T + TAP_PAD) * 4u : 0u) + 4u * COPY * sizeof(float2);
    static_assert(1024u * (16u + TAP_PAD) * 4u + 4u * COPY * sizeof(float2) <= 160u * 1024u, "LDS of a CU");
    // with the table in LDS a workgroup loads it once and strides over the tiles: one workgroup per CU
    u64 cap = MAX_GRID;
    if (TAPS_LDS && !direct) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
        cap = (u64)vit_device_cus(dev);
    }
    const u64 ntiles = ((u64)nout + A.tile - 1u) / A.tile;
    const unsigned grid = (unsigned)(ntiles < cap ? ntiles : cap);
    switch (fmt.format) {
        case VIT_IQ_F32: return launch<VIT_IQ_F32>(direct, grid, lds, stream, A);
        case VIT_IQ_CU8: return launch<VIT_IQ_CU8>(direct, grid, lds, stream, A);
        case VIT_IQ_CS8: return launch<VIT_IQ_CS8>(direct, grid, lds, stream, A);
        case VIT_IQ_CS16: return launch<VIT_IQ_CS16>(direct, grid, lds, stream, A);
        default: return hipErrorInvalidValue;
    }
}
