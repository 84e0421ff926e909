// vit_ofdm.hip -- from the FFT to soft bytes (include/viterbi_amd.h, "From the FFT"): differential demodulation,
// frequency de-interleaving, QPSK demapping and quantisation of whole transmission frames, the FIC's symbols to d_fic
// and the MSC's to the ring of CIF rows that vit_ti.hip reads.
//
// The result is defined bit for bit, so every float operation below is a single IEEE binary32 operation: this file is
// compiled with contraction off (the pragma; the rest of the library keeps the compiler's default), the arithmetic is
// written with plain operators, and `/` is the compiler's correctly rounded expansion.
//
// One workgroup owns one frame and a run of consecutive data symbols.  A lane owns fixed 16-byte chunks (two bins) of a
// row, in BIN order: row loads are coalesced dwordx4 loads, the previous symbol's values stay in the lane's registers (a
// row is read once per run, plus one row at the run's start), and each chunk of the next row is loaded as soon as the
// chunk of the previous row it replaces has been used: two rows of registers, at most 64 VGPRs, 8 workgroups per CU.  At its start the workgroup inverts d_bins into LDS (bin -> n, 0xFFFF for a bin no carrier uses)
// and every lane keeps a mask of its chunks that carry anything; a chunk whose two bins are unused is never loaded, so the guard
// band and DC cost no traffic and may hold anything.  The two soft bytes of a carrier go to positions n and n + K of
// a 2K-byte LDS tile and the tile leaves as 16-byte stores of any alignment; two tiles, so one barrier per symbol.
// A table entry >= nfft is ignored and of a repeated entry one n wins: the tile bytes nobody owns keep the erasure
// value the tiles start with.
#pragma clang fp contract(off)
#include "vit_demap_dev.h"

namespace {

using namespace vit_demap;
constexpr u32 UNUSED = 0xFFFFu;  // K <= 8192, so no n reaches it

struct OfdmArgs {
    const float4* fft;         // two carriers per element
    u64 sym_stride2, frame_stride2;  // in float4 elements
    const uint16_t* bins;
    u32 nfft, K, fic_syms, cifs, per;
    u32 lo, hi;      // the data symbols [lo, hi) of every frame are demapped
    u32 run, runs;   // data symbols per workgroup, workgroups per frame
    float gain;
    uint8_t* fic;
    uint8_t* ring;
    u64 row_bytes, nrows, first_row, col;
};

template <u32 TPB, u32 CPL>
struct Row {
    float4 v[CPL];
};

// Chunk j of a lane is float4 element threadIdx.x + j*TPB of a row, addressed as a uniform base plus the lane's 32-bit
// byte offset; `used` bit j: the chunk has a carrier (the others are never loaded).
template <u32 TPB>
__device__ __forceinline__ float4 load_chunk(const float4* row, u32 j, u32 lane_off) {
    return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(row + j * TPB) + lane_off);
}

template <u32 TPB, u32 CPL>
__device__ __forceinline__ void load_row(const float4* row, u32 lane_off, u32 used, Row<TPB, CPL>& r) {
#pragma unroll
    for (u32 j = 0; j < CPL; j++) {
        r.v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (used >> j & 1u) r.v[j] = load_chunk<TPB>(row, j, lane_off);
    }
}

// One data symbol: a = its own row, b = the row before.  Writes the symbol's soft bytes to `tile`; a chunk of b is dead
// once used, and its registers receive the same chunk of `next` (the row after a) if there is one: two rows of registers,
// the loads of the next row in flight during the rest of the arithmetic, the barrier and the tile's stores.
template <u32 TPB, u32 CPL>
__device__ __forceinline__ void demap_symbol(const Row<TPB, CPL>& a, Row<TPB, CPL>& b, const float4* next, u32 lane_off,
                                             u32 used, const u32* inv2, uint8_t* tile, u32 K, float gain) {
#pragma unroll
    for (u32 j = 0; j < CPL; j++) {
        if (!(used >> j & 1u)) continue;
        const u32 ent = inv2[threadIdx.x + j * TPB], n0 = ent & 0xFFFFu, n1 = ent >> 16;  // n of the two bins
        if (n0 != UNUSED) {
            const u32 q = soft_pair(a.v[j].x, a.v[j].y, b.v[j].x, b.v[j].y, gain);
            tile[n0] = (uint8_t)q;
            tile[K + n0] = (uint8_t)(q >> 8);
        }
        if (n1 != UNUSED) {
            const u32 q = soft_pair(a.v[j].z, a.v[j].w, b.v[j].z, b.v[j].w, gain);
            tile[n1] = (uint8_t)q;
            tile[K + n1] = (uint8_t)(q >> 8);
        }
        if (next) b.v[j] = load_chunk<TPB>(next, j, lane_off);
    }
}

// The workgroup's start: the erasure value into the tiles, d_bins inverted into `inv`, the first two rows of the run (the
// one at row0 and the next) into x and y.  Returns `used`.  The lane's chunks are threadIdx.x + j*TPB; their entries (n
// of the two bins, low half first) stay in LDS.
template <u32 TPB, u32 CPL>
__device__ __forceinline__ u32 demap_begin(const OfdmArgs& A, uint8_t* tiles, u32 tb, uint16_t* inv, const float4* row0,
                                           u32 lane_off, Row<TPB, CPL>& x, Row<TPB, CPL>& y) {
    for (u32 i = threadIdx.x; i < A.nfft / 2u; i += TPB) reinterpret_cast<u32*>(inv)[i] = UNUSED | UNUSED << 16;
    for (u32 i = threadIdx.x; i < 2u * tb / 4u; i += TPB) reinterpret_cast<u32*>(tiles)[i] = 0x80808080u;
    __syncthreads();
    for (u32 n = threadIdx.x; n < A.K; n += TPB) {
        const u32 b = A.bins[n];
        if (b < A.nfft) inv[b] = (uint16_t)n;
    }
    __syncthreads();
    const u32* inv2 = reinterpret_cast<const u32*>(inv);
    u32 used = 0;
#pragma unroll
    for (u32 j = 0; j < CPL; j++) {
        const u32 c = threadIdx.x + j * TPB;
        if (2u * c < A.nfft && inv2[c] != 0xFFFFFFFFu) used |= 1u << j;
    }
    load_row(row0, lane_off, used, x);
    load_row(row0 + A.sym_stride2, lane_off, used, y);
    return used;
}

// LDS: two tiles of tb bytes (2K rounded up to 16), then nfft u16 of the inverted table.
template <u32 TPB, u32 CPL>
__global__ __launch_bounds__(TPB) void vit_ofdm_demap_kernel(OfdmArgs A) {
    extern __shared__ uint4 lds_ofdm[];  // no static LDS in this kernel: the base stays 16-byte aligned
    const u32 K = A.K, nb = 2u * K, tb = (nb + 15u) / 16u * 16u;
    uint8_t* tiles = reinterpret_cast<uint8_t*>(lds_ofdm);
    uint16_t* inv = reinterpret_cast<uint16_t*>(tiles + 2u * tb);
    const u64 t = blockIdx.x / A.runs;
    const u32 s0 = A.lo + (u32)(blockIdx.x % A.runs) * A.run, s1 = s0 + A.run < A.hi ? s0 + A.run : A.hi;

    const u32* inv2 = reinterpret_cast<const u32*>(inv);
    const u32 lane_off = threadIdx.x * 16u;
    const float4* frame = A.fft + t * A.frame_stride2;
    Row<TPB, CPL> x, y;  // rows s and s + 1 at even s - s0, rows s + 1 and s at odd
    const u32 used = demap_begin(A, tiles, tb, inv, frame + (u64)s0 * A.sym_stride2, lane_off, x, y);
    for (u32 s = s0; s < s1; s++) {
        uint8_t* tile = tiles + (s & 1u) * tb;
        const float4* next = s + 1u < s1 ? frame + (u64)(s + 2u) * A.sym_stride2 : nullptr;
        if ((s - s0) & 1u)
            demap_symbol(x, y, next, lane_off, used, inv2, tile, K, A.gain);
        else
            demap_symbol(y, x, next, lane_off, used, inv2, tile, K, A.gain);
        __syncthreads();
        // The tile's nb bytes to their place as 16-byte stores of any alignment.  These lines stand in both kernels: as a
        // function both call, they cost the per-symbol kernels two VGPRs (256 x 4: 84 -> 86) and VIT_SOFT_PER_SYMBOL at
        // nfft 2048 0.3 % (0.1615 -> 0.1622 ms for 512 frames, profiles/r19_front_isa_same.txt).
        uint8_t* dst = soft_dst(A, t, s);
        if (nb >= 16u) {
            for (u32 e = threadIdx.x; e < tb / 16u; e += TPB) {
                const u32 want = 16u * e, a = want < nb - 16u ? want : nb - 16u;  // the last chunk ends at the tile's end
                uint4 v;
                if (a == want) {
                    v = *reinterpret_cast<const uint4*>(tile + a);
                } else {
                    u32 w[4] = {0, 0, 0, 0};
#pragma unroll
                    for (u32 k = 0; k < 16; k++) w[k >> 2] |= (u32)tile[a + k] << (8u * (k & 3u));
                    v = make_uint4(w[0], w[1], w[2], w[3]);
                }
                __builtin_memcpy(dst + a, &v, 16);  // unaligned global_store_dwordx4
            }
        } else if (threadIdx.x < nb) {
            dst[threadIdx.x] = tile[threadIdx.x];
        }
    }
}

// ---- VIT_SOFT_PER_SYMBOL (include/viterbi_amd.h, "Channel-state weighting") ------------------------------------------
// A kernel beside the one above, with its start.  A symbol is demapped in two halves around its level S:
//   1. re, im and nrm of the lane's carriers; re and im stay in the lane's registers (0 for an erasure), the term of the
//      sum goes to position n of a float array in LDS; the chunk of b is dead and receives the next row, as above;
//   2. the first A = max(64, nfft/8) threads are the header's accumulators: thread i reads groups i and i + A of 4
//      consecutive n (one 16-byte LDS load each), the wavefronts reduce (vit_csi_dev.h) and leave their totals in LDS;
//   3. every thread finishes the tree, forms s, quantises its carriers into the tile; the tile leaves as above.
// Three barriers per symbol instead of one.  LDS: the kernel above's, then 4*ceil(K/4) floats and CSI_PARTS totals.
struct SoftArgs {
    float* level;  // d_level or nullptr
    u32 nlev;      // its words per frame: nsyms - 1
};

template <u32 TPB, u32 CPL>
struct Prod {
    float4 y[CPL];  // (re, im) of the chunk's two bins
};

template <u32 TPB, u32 CPL>
__device__ __forceinline__ void soft_products(const Row<TPB, CPL>& a, Row<TPB, CPL>& b, const float4* next, u32 lane_off,
                                              u32 used, const u32* inv2, float* term, Prod<TPB, CPL>& p) {
#pragma unroll
    for (u32 j = 0; j < CPL; j++) {
        p.y[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!(used >> j & 1u)) continue;
        const u32 ent = inv2[threadIdx.x + j * TPB], n0 = ent & 0xFFFFu, n1 = ent >> 16;  // n of the two bins
        if (n0 != UNUSED) {
            const float re = a.v[j].x * b.v[j].x + a.v[j].y * b.v[j].y;
            const float im = a.v[j].y * b.v[j].x - a.v[j].x * b.v[j].y;
            const float v = vit_csi::csi_term(__builtin_fabsf(re) + __builtin_fabsf(im));
            term[n0] = v;
            if (v != 0.0f) {
                p.y[j].x = re;
                p.y[j].y = im;
            }
        }
        if (n1 != UNUSED) {
            const float re = a.v[j].z * b.v[j].z + a.v[j].w * b.v[j].w;
            const float im = a.v[j].w * b.v[j].z - a.v[j].z * b.v[j].w;
            const float v = vit_csi::csi_term(__builtin_fabsf(re) + __builtin_fabsf(im));
            term[n1] = v;
            if (v != 0.0f) {
                p.y[j].z = re;
                p.y[j].w = im;
            }
        }
        if (next) b.v[j] = load_chunk<TPB>(next, j, lane_off);
    }
}

// LDS: two tiles of tb bytes, nfft u16 of the inverted table, K4 = 4*ceil(K/4) terms, CSI_PARTS wavefront totals.
template <u32 TPB, u32 CPL>
__global__ __launch_bounds__(TPB) void vit_ofdm_demap_soft_kernel(OfdmArgs A, SoftArgs L) {
    extern __shared__ uint4 lds_ofdm[];
    const u32 K = A.K, nb = 2u * K, tb = (nb + 15u) / 16u * 16u, ngroups = (K + 3u) / 4u;
    const u32 NA = A.nfft / 8u < 64u ? 64u : A.nfft / 8u;  // accumulators: NA <= TPB, whole wavefronts
    uint8_t* tiles = reinterpret_cast<uint8_t*>(lds_ofdm);
    uint16_t* inv = reinterpret_cast<uint16_t*>(tiles + 2u * tb);
    float* term = reinterpret_cast<float*>(tiles + 2u * tb + 2u * A.nfft);  // 16-byte aligned: nfft >= 64
    float* part = term + 4u * ngroups;
    const u64 t = blockIdx.x / A.runs;
    const u32 s0 = A.lo + (u32)(blockIdx.x % A.runs) * A.run, s1 = s0 + A.run < A.hi ? s0 + A.run : A.hi;

    for (u32 i = threadIdx.x; i < 4u * ngroups + vit_csi::CSI_PARTS; i += TPB) term[i] = 0.0f;  // an n nobody owns adds +0
    const u32* inv2 = reinterpret_cast<const u32*>(inv);
    const u32 lane_off = threadIdx.x * 16u;
    const float4* frame = A.fft + t * A.frame_stride2;
    Row<TPB, CPL> x, y;  // rows s and s + 1 at even s - s0, rows s + 1 and s at odd
    const u32 used = demap_begin(A, tiles, tb, inv, frame + (u64)s0 * A.sym_stride2, lane_off, x, y);
    for (u32 s = s0; s < s1; s++) {
        uint8_t* tile = tiles + (s & 1u) * tb;
        const float4* next = s + 1u < s1 ? frame + (u64)(s + 2u) * A.sym_stride2 : nullptr;
        Prod<TPB, CPL> p;
        if ((s - s0) & 1u)
            soft_products(x, y, next, lane_off, used, inv2, term, p);
        else
            soft_products(y, x, next, lane_off, used, inv2, term, p);
        __syncthreads();
        if (threadIdx.x < NA) {  // whole wavefronts
            const u32 g0 = threadIdx.x, g1 = threadIdx.x + NA;
            float acc = 0.0f;
            if (g0 < ngroups) {
                const float4 v = reinterpret_cast<const float4*>(term)[g0];
                acc = vit_csi::csi_group(v.x, v.y, v.z, v.w);
            }
            if (g1 < ngroups) {
                const float4 v = reinterpret_cast<const float4*>(term)[g1];
                acc = acc + vit_csi::csi_group(v.x, v.y, v.z, v.w);
            }
            acc = vit_wave::wave_sum(acc);
            if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = acc;
        }
        __syncthreads();
        const float S = vit_wave::pair_tree<TPB / 64u>(part);
        const float sc = vit_csi::csi_scale(S, A.gain, K);
        if (threadIdx.x == 0 && L.level) L.level[t * L.nlev + s] = S;
#pragma unroll
        for (u32 j = 0; j < CPL; j++) {
            if (!(used >> j & 1u)) continue;
            const u32 ent = inv2[threadIdx.x + j * TPB], n0 = ent & 0xFFFFu, n1 = ent >> 16;
            if (n0 != UNUSED) {
                const u32 q = vit_csi::csi_pair(p.y[j].x, p.y[j].y, sc);
                tile[n0] = (uint8_t)q;
                tile[K + n0] = (uint8_t)(q >> 8);
            }
            if (n1 != UNUSED) {
                const u32 q = vit_csi::csi_pair(p.y[j].z, p.y[j].w, sc);
                tile[n1] = (uint8_t)q;
                tile[K + n1] = (uint8_t)(q >> 8);
            }
        }
        __syncthreads();
        // the tile's nb bytes to their place: the lines of the kernel above, for the reason given there
        uint8_t* dst = soft_dst(A, t, s);
        if (nb >= 16u) {
            for (u32 e = threadIdx.x; e < tb / 16u; e += TPB) {
                const u32 want = 16u * e, a = want < nb - 16u ? want : nb - 16u;  // the last chunk ends at the tile's end
                uint4 v;
                if (a == want) {
                    v = *reinterpret_cast<const uint4*>(tile + a);
                } else {
                    u32 w[4] = {0, 0, 0, 0};
#pragma unroll
                    for (u32 k = 0; k < 16; k++) w[k >> 2] |= (u32)tile[a + k] << (8u * (k & 3u));
                    v = make_uint4(w[0], w[1], w[2], w[3]);
                }
                __builtin_memcpy(dst + a, &v, 16);  // unaligned global_store_dwordx4
            }
        } else if (threadIdx.x < nb) {
            dst[threadIdx.x] = tile[threadIdx.x];
        }
    }
}

template <u32 TPB, u32 CPL>
hipError_t launch(const OfdmArgs& A, const SoftArgs* L, u64 grid, size_t lds, hipStream_t stream) {
    // nfft 8192 with K > 4080: the terms take the per-symbol kernel past the default limit of dynamic LDS
    if (L) return vit_launch_dynamic_lds<&vit_ofdm_demap_soft_kernel<TPB, CPL>>((unsigned)grid, TPB, lds, stream, A, *L);
    return vit_launch_dynamic_lds<&vit_ofdm_demap_kernel<TPB, CPL>>((unsigned)grid, TPB, lds, stream, A);
}

}  // namespace

int64_t vit_freq_bins_host(uint32_t nfft, uint16_t* h_bins) {
    if (!h_bins || (nfft != 256u && nfft != 512u && nfft != 1024u && nfft != 2048u)) return -1;
    int64_t n = 0;
    uint32_t p = 0;
    for (uint32_t i = 1; i < nfft; i++) {
        p = (13u * p + nfft / 4u - 1u) % nfft;
        if (p >= nfft / 8u && p <= 7u * nfft / 8u && p != nfft / 2u) h_bins[n++] = (uint16_t)((p + nfft / 2u) % nfft);  // k mod nfft
    }
    return n;
}

hipError_t vit_launch_ofdm_demap(const float* d_fft, uint64_t sym_stride, uint64_t frame_stride, const uint16_t* d_bins,
                                 const vit_ofdm_shape& shape, float gain, int64_t nframes, uint8_t* d_fic,
                                 const vit_cif_ring* ring, uint64_t col, uint32_t rule, float* d_level, hipStream_t stream) {
    OfdmArgs A = {};
    A.fft = reinterpret_cast<const float4*>(d_fft);
    A.sym_stride2 = sym_stride / 2u;
    A.frame_stride2 = frame_stride / 2u;
    A.bins = d_bins;
    A.nfft = shape.nfft;
    set_outputs(A, shape, gain, d_fic, ring, col);
    const u64 grid = split_runs(A, nframes);
    if (grid == 0) return hipSuccess;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    size_t lds = 2u * (size_t)((2u * A.K + 15u) / 16u * 16u) + 2u * (size_t)A.nfft;
    const SoftArgs soft = {d_level, shape.nsyms - 1u}, *L = rule == VIT_SOFT_PER_SYMBOL ? &soft : nullptr;
    if (L) lds += 4u * (size_t)((A.K + 3u) / 4u * 4u + vit_csi::CSI_PARTS);  // at most 80 KiB + 64 (nfft = K = 8192)
    const u32 chunks = A.nfft / 2u;
    if (chunks <= 256u) return launch<256, 1>(A, L, grid, lds, stream);
    if (chunks <= 512u) return launch<256, 2>(A, L, grid, lds, stream);
    if (chunks <= 1024u) return launch<256, 4>(A, L, grid, lds, stream);
    if (chunks <= 2048u) return launch<1024, 2>(A, L, grid, lds, stream);
    return launch<1024, 4>(A, L, grid, lds, stream);
}
