// vit_ofdm_acq.hip -- from the stream to the coarse starts vit_ofdm_sync_dev reads (include/viterbi_amd.h, "From the
// stream: first acquisition"): the power of every block of B samples, then per frame period the last minimum of
// q = N / R, the power in front of a candidate edge over the power behind it.  Defined bit for bit: every float operation
// is one IEEE binary32 operation (contraction off, plain operators), a block's power is the tree of adjacent pairs, a
// window's sum is serial in ascending order.  Nothing here depends on the launch: no atomics, no scan over the grid.
//
// Two kernels, not one.  The power pass is a stream: it reads every sample once and writes 4 bytes per B samples, and it
// fills the device whatever the number of periods.  The search reads powers only (1/B of the samples, each Ln + Lr
// times, from LDS) and has one workgroup per period; fused into one kernel the stream would be read by as many
// workgroups as there are periods - 1 to 10 in a live receiver, on 256 CUs.
//
//   power   A lane owns chunks of 16 bytes: 2 float32, 4 CS16 or 8 CU8 / CS8 samples, never across a block (B >= 8).  A
//           wavefront owns a tile of 4 rows of 64 chunks, consecutive lanes on consecutive chunks, all 4 loads in flight.
//           The tree of adjacent pairs is taken inside the lane over the chunk, then across the lanes of a row by xor
//           exchanges (DPP up to 8 lanes apart; fl(a+b) = fl(b+a), so the butterfly gives the tree's bits in every lane),
//           then, for a block of more than 64 chunks, across the 2 or 4 rows it spans.  A chunk is one 16-byte load at
//           whatever alignment `first` gives it (8, 4 or 2 bytes): no byte outside [first, first + nblk*B) is touched.
//   search  One workgroup per period, tile by tile: TILE candidates and the Ln + Lr - 1 powers around them in LDS, thread T
//           on candidates T, T + 256, ...: at every step of a window consecutive lanes read consecutive words.  A thread
//           keeps its last minimum (q, j, N, R); the workgroup's is the minimum over (q, -j); its owner writes the period.
#pragma clang fp contract(off)
#include "vit_internal.h"
#include "vit_iq_dev.h"
#include "vit_wave_dev.h"

namespace {

typedef uint32_t u32;
typedef uint64_t u64;

// (the chunk's 16 bytes, TILE_CHUNKS, SEARCH_TILE and WINDOW_MAX stand again in viterbi.dll_amd/__init__.py, ACQ_GEOMETRY: the
// tests take their edges from it)
constexpr u32 ROWS = 4u;             // 16-byte chunks a lane has in flight
constexpr u32 TILE_CHUNKS = 64u * ROWS;  // ACQ_GEOMETRY["tile_chunks"]
constexpr u32 POWER_TPB = 256u;
constexpr u32 POWER_MAX_GRID = 8192u;  // the waves stride over the tiles beyond it

constexpr u32 SEARCH_TPB = 256u;
constexpr u32 SEARCH_TILE = 2048u;   // candidates per LDS tile: ACQ_GEOMETRY["search_tile"]
constexpr u32 WINDOW_MAX = 4096u;    // Ln, Lr at most: ACQ_GEOMETRY["window_max"]
constexpr u32 SEARCH_LDS = SEARCH_TILE + 2u * WINDOW_MAX;  // floats: 40 KiB
constexpr u32 SEARCH_MAX_GRID = 1u << 20;
constexpr u32 NONE = 0xFFFFFFFFu;    // no candidate

struct PowerArgs {
    const char* s0;   // the sample at `first`
    u64 nchunks;      // nblk * B / (samples per chunk)
    u32 lg;           // log2(chunks per block)
    float scale;
    float* power;
};

struct SearchArgs {
    const float* power;
    u64 nblk, first;
    long long offset, nperiods;
    u32 B, Ln, Lr, Pb;
    float thr;
    long long* start_out;
    u32* info;
};

// the power of the V samples of one chunk: e = fl(fl(re*re) + fl(im*im)), then adjacent pairs
template <u32 V>
__device__ __forceinline__ float chunk_power(const float2 (&x)[V]) {
    float e[V];
#pragma unroll
    for (u32 i = 0; i < V; i++) e[i] = x[i].x * x[i].x + x[i].y * x[i].y;
    return vit_wave::pair_tree<V>(e);
}

// the 16 bytes of the chunk at p, which is aligned as a sample of its format is and no more: global loads need no alignment
// on this target, and the load touches the chunk's bytes only
__device__ __forceinline__ void load_chunk(const char* p, uint4& raw) { __builtin_memcpy(&raw, p, 16); }

template <u32 FMT>
__device__ __forceinline__ float raw_power(const uint4& raw, float scale) {
    const u32 w[4] = {raw.x, raw.y, raw.z, raw.w};
    if constexpr (FMT == VIT_IQ_F32) {
        const float2 x[2] = {make_float2(__uint_as_float(w[0]), __uint_as_float(w[1])),
                             make_float2(__uint_as_float(w[2]), __uint_as_float(w[3]))};
        return chunk_power<2>(x);
    } else if constexpr (FMT == VIT_IQ_CS16) {
        float2 x[4];
        vit_iq::iq_convert<4>(w, FMT, scale, x);
        return chunk_power<4>(x);
    } else {
        u32 s[8];
#pragma unroll
        for (u32 i = 0; i < 8; i++) s[i] = w[i / 2u] >> (16u * (i & 1u)) & 0xFFFFu;
        float2 x[8];
        vit_iq::iq_convert<8>(s, FMT, scale, x);
        return chunk_power<8>(x);
    }
}

template <u32 FMT>
__global__ __launch_bounds__(POWER_TPB) void vit_acq_power_kernel(PowerArgs A) {
    const u32 lane = threadIdx.x & 63u;
    const u64 wave = (u64)blockIdx.x * (POWER_TPB / 64u) + (threadIdx.x >> 6);
    const u64 nwaves = (u64)gridDim.x * (POWER_TPB / 64u);
    const u64 ntiles = (A.nchunks + TILE_CHUNKS - 1u) / TILE_CHUNKS;
    for (u64 tile = wave; tile < ntiles; tile += nwaves) {  // uniform over the wavefront: every lane takes part in the exchanges
        const u64 c0 = tile * TILE_CHUNKS + lane;
        uint4 raw[ROWS];
#pragma unroll
        for (u32 r = 0; r < ROWS; r++) {
            raw[r] = make_uint4(0u, 0u, 0u, 0u);
            const u64 c = c0 + 64u * r;
            if (c < A.nchunks) load_chunk(A.s0 + c * 16u, raw[r]);
        }
        // a chunk beyond nchunks lies in a block beyond nblk, whole: what its lane holds meets no block that is written
        float v[ROWS];
#pragma unroll
        for (u32 r = 0; r < ROWS; r++) v[r] = raw_power<FMT>(raw[r], A.scale);
        // the exchange levels inside a row, min(lg, 6) of them: unrolled, so that every level is its own DPP control and
        // what is left of the loop is one uniform branch per level
#pragma unroll
        for (u32 level = 0; level < 6u; level++)
            if (level < A.lg)
#pragma unroll
                for (u32 r = 0; r < ROWS; r++) v[r] = vit_wave::xor_add(v[r], level);
        if (A.lg <= 6u) {
            // lane l of row r holds the sum of its block: chunk c is the first of block c >> lg
            if ((lane & ((1u << A.lg) - 1u)) == 0u)
#pragma unroll
                for (u32 r = 0; r < ROWS; r++) {
                    const u64 c = c0 + 64u * r;
                    if (c < A.nchunks) A.power[c >> A.lg] = v[r];
                }
        } else if (lane == 0 && c0 < A.nchunks) {
            // a block spans 2 or 4 rows: their sums meet in adjacent pairs
            const float a = v[0] + v[1], b = v[2] + v[3];
            if (A.lg == 7u) {
                A.power[2u * tile] = a;
                if (c0 + 128u < A.nchunks) A.power[2u * tile + 1u] = b;
            } else {
                A.power[tile] = a + b;
            }
        }
    }
}

// the better of two last minima: the smaller q, at equal q the later candidate; NONE loses against everything
__device__ __forceinline__ bool later_min(float qa, u32 ja, float qb, u32 jb) {  // b replaces a
    return qb < qa || (qb == qa && jb + 1u > ja + 1u);
}

__global__ __launch_bounds__(SEARCH_TPB) void vit_acq_search_kernel(SearchArgs A) {
    __shared__ float pw[SEARCH_LDS];
    __shared__ float red_q[SEARCH_TPB / 64u];
    __shared__ u32 red_j[SEARCH_TPB / 64u];
    const u32 T = threadIdx.x, lane = T & 63u, wave = T >> 6;
    const u32 Ln = A.Ln, Lr = A.Lr, halo = Ln + Lr - 1u;
    const float inf = __builtin_inff();
    for (long long k = blockIdx.x; k < A.nperiods; k += gridDim.x) {
        // the period's candidates j = Ln + k*Pb + i, i < ncand: those with j + Lr <= nblk
        u64 ncand = 0;
        u64 p0 = 0;  // the first power the period reads: N of its first candidate starts there
        if ((u64)k <= A.nblk / A.Pb) {
            p0 = (u64)k * A.Pb;
            const u64 need = p0 + Ln + Lr;  // the first candidate's last power, + 1
            if (need <= A.nblk) {
                ncand = A.nblk - need + 1u;
                if (ncand > A.Pb) ncand = A.Pb;
            }
        }
        float bq = inf, bn = 0.f, br = 0.f;
        u32 bj = NONE;
        for (u64 t0 = 0; t0 < ncand; t0 += SEARCH_TILE) {
            const u32 nc = ncand - t0 < SEARCH_TILE ? (u32)(ncand - t0) : SEARCH_TILE;
            __syncthreads();  // the tile before has been read
            for (u32 i = T; i < nc + halo; i += SEARCH_TPB) pw[i] = A.power[p0 + t0 + i];  // the last is power p0 + ncand + halo - 1 < nblk
            __syncthreads();
            for (u32 i = T; i < nc; i += SEARCH_TPB) {
                float n = 0.f, r = 0.f;
                for (u32 m = 0; m < Ln; m++) n = n + pw[i + m];
                for (u32 m = 0; m < Lr; m++) r = r + pw[i + Ln + m];
                const float q = r > 0.f ? n / r : inf;
                if (q <= bq) {  // ascending i: the last minimum
                    bq = q;
                    bj = (u32)(t0 + i);
                    bn = n;
                    br = r;
                }
            }
        }
        // the workgroup's last minimum over (q, j); every candidate belongs to one thread
        float wq = bq;
        u32 wj = bj;
#pragma unroll
        for (u32 h = 1; h < 64u; h *= 2) {
            const float oq = __shfl_xor(wq, (int)h);
            const u32 oj = (u32)__shfl_xor((int)wj, (int)h);
            if (later_min(wq, wj, oq, oj)) {
                wq = oq;
                wj = oj;
            }
        }
        __syncthreads();  // the period before has read red_*
        if (lane == 0) {
            red_q[wave] = wq;
            red_j[wave] = wj;
        }
        __syncthreads();
#pragma unroll
        for (u32 i = 0; i < SEARCH_TPB / 64u; i++)
            if (later_min(wq, wj, red_q[i], red_j[i])) {
                wq = red_q[i];
                wj = red_j[i];
            }
        if (wj == NONE ? T == 0 : bj == wj) {
            long long start = -1;
            if (wj != NONE && bq <= A.thr)
                start = (long long)(A.first + ((u64)Ln + (u64)k * A.Pb + wj) * A.B + (u64)A.offset);
            A.start_out[k] = start;
            if (A.info) {
                u32* o = A.info + 4u * (u64)k;
                o[0] = wj;
                o[1] = __float_as_uint(wj == NONE ? inf : bq);
                o[2] = __float_as_uint(wj == NONE ? 0.f : bn);
                o[3] = __float_as_uint(wj == NONE ? 0.f : br);
            }
        }
    }
}

}  // namespace

hipError_t vit_launch_acq_power(const void* d_iq, const vit_iq_format& fmt, uint64_t first, uint32_t B, uint64_t nblk, float* d_power,
                                hipStream_t stream) {
    if (nblk == 0) return hipSuccess;
    const u32 sb = vit_iq::sample_bytes(fmt.format), per_chunk = 16u / sb;
    PowerArgs A = {};
    A.s0 = reinterpret_cast<const char*>(d_iq) + first * sb;
    A.nchunks = nblk * (B / per_chunk);
    A.lg = (u32)__builtin_ctz(B / per_chunk);
    A.scale = fmt.scale;
    A.power = d_power;
    const u64 tiles = (A.nchunks + TILE_CHUNKS - 1u) / TILE_CHUNKS, wgs = (tiles + POWER_TPB / 64u - 1u) / (POWER_TPB / 64u);
    const unsigned grid = (unsigned)(wgs < POWER_MAX_GRID ? wgs : POWER_MAX_GRID);
    switch (fmt.format) {
        case VIT_IQ_F32: hipLaunchKernelGGL(vit_acq_power_kernel<VIT_IQ_F32>, dim3(grid), dim3(POWER_TPB), 0, stream, A); break;
        case VIT_IQ_CU8: hipLaunchKernelGGL(vit_acq_power_kernel<VIT_IQ_CU8>, dim3(grid), dim3(POWER_TPB), 0, stream, A); break;
        case VIT_IQ_CS8: hipLaunchKernelGGL(vit_acq_power_kernel<VIT_IQ_CS8>, dim3(grid), dim3(POWER_TPB), 0, stream, A); break;
        case VIT_IQ_CS16: hipLaunchKernelGGL(vit_acq_power_kernel<VIT_IQ_CS16>, dim3(grid), dim3(POWER_TPB), 0, stream, A); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t vit_launch_acq_search(const float* d_power, uint64_t nblk, const vit_acq_params& p, int64_t nperiods, int64_t* d_start_out,
                                 uint32_t* d_info, hipStream_t stream) {
    if (nperiods <= 0) return hipSuccess;
    static_assert(SEARCH_LDS * 4u + 64u <= 64u * 1024u, "static LDS");
    SearchArgs A = {};
    A.power = d_power;
    A.nblk = nblk;
    A.first = p.first;
    A.offset = p.offset;
    A.nperiods = nperiods;
    A.B = p.B;
    A.Ln = p.null_blocks;
    A.Lr = p.ref_blocks;
    A.Pb = p.period_blocks;
    A.thr = p.thr;
    A.start_out = reinterpret_cast<long long*>(d_start_out);
    A.info = d_info;
    const unsigned grid = (unsigned)(nperiods < (int64_t)SEARCH_MAX_GRID ? nperiods : (int64_t)SEARCH_MAX_GRID);
    hipLaunchKernelGGL(vit_acq_search_kernel, dim3(grid), dim3(SEARCH_TPB), 0, stream, A);
    return hipGetLastError();
}
